"""The planner's choice of the lazy instance's hit-queue form (csrc/rl_plan.cc; RaylibAMD_PlanRender) and the scope of its switch: a lazy plan with
maxPathLength >= 1 takes it, RAYLIB_HIT_QUEUE=0 keeps the ray-queue instance and changes nothing else of the plan, and RAYLIB_HIT_QUEUE=1 reaches no render
the lazy instance does not take.  No device needed."""
import ctypes as C
import os

from helpers import scenes


def _plan(lib, ses, max_path=5, w=64, h=48, spp=4):
    from raylib_amd import binding
    st = binding.RendererSettings(w, h, spp, int(max_path), 1e-4, 0)
    p = binding.RenderPlan()
    assert lib.RaylibAMD_PlanRender(ses.scene, C.byref(st), 0, 256, 4, C.byref(p)) == 1
    return p.as_dict()


def test_planner_choice_and_switch_scope(lib, workdir, monkeypatch):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "hit_queue_host"); os.makedirs(d, exist_ok=True)
    for name in ("RAYLIB_HIT_QUEUE", "RAYLIB_LAZY_REFL", "RAYLIB_PLAIN_KERNEL", "RAYLIB_LEAF_LIST", "RAYLIB_LDS_SCENE", "RAYLIB_POOL"):
        monkeypatch.delenv(name, raising=False)
    ses = binding.SceneSession(lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 4 / 3)
    on = _plan(lib, ses)
    assert (on["lds"], on["plain"], on["lazy"], on["hitQueue"]) == (2, 1, 1, 1)          # the default wherever the lazy instance is chosen
    for max_path in (1, 2, 4096):
        assert _plan(lib, ses, max_path=max_path)["hitQueue"] == 1
    # the switch: the ray-queue instance, and nothing else of the plan moves
    monkeypatch.setenv("RAYLIB_HIT_QUEUE", "0")
    off = _plan(lib, ses)
    assert off["hitQueue"] == 0 and off["lazy"] == 1
    assert {k: v for k, v in off.items() if k != "hitQueue"} == {k: v for k, v in on.items() if k != "hitQueue"}
    # asked for, but not where the lazy instance is not taken or a camera ray may not be traced
    monkeypatch.setenv("RAYLIB_HIT_QUEUE", "1")
    assert _plan(lib, ses)["hitQueue"] == 1
    for max_path in (0, -3):
        p = _plan(lib, ses, max_path=max_path)
        assert (p["lazy"], p["hitQueue"]) == (1, 0), max_path                              # the path ends before its first ray
    assert _plan(lib, ses, max_path=4097)["lazy"] == 0 and _plan(lib, ses, max_path=4097)["hitQueue"] == 0
    for name, value in (("RAYLIB_LAZY_REFL", "0"), ("RAYLIB_PLAIN_KERNEL", "0"), ("RAYLIB_LEAF_LIST", "0"), ("RAYLIB_LDS_SCENE", "0"), ("RAYLIB_POOL", "2")):
        monkeypatch.setenv(name, value)
        p = _plan(lib, ses)
        assert (p["lazy"], p["hitQueue"]) == (0, 0), name
        monkeypatch.delenv(name)
    ses.close()
    glass = binding.SceneSession(lib, scenes.cornell(os.path.join(d, "glass.obj"), short_material=scenes.GLASS)[0], (0, 1, 4), (0, 1, -1), 45.0, 4 / 3)
    assert lib.RaylibAMD_SceneLazyRefl(glass.scene) == 0
    p = _plan(lib, glass)
    assert (p["lds"], p["lazy"], p["hitQueue"]) == (2, 0, 0)
    glass.close()


def test_last_hit_queue_is_exported(lib):
    """Callable without a device; 0 until a lazy launch runs the hit-queue form."""
    assert lib.RaylibAMD_LastHitQueue() in (0, 1)
