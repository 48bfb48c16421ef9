"""The scenes of test_gpu_leaf_walk_scenes.py, checked where the builder runs: every soup of leaf_walk_scenes.py has the leaf count written beside its
seed, so the leaf lists of the set have 1 .. 6 records, and the planner gives each scene the leaf-list kernel's lazy-reflectance instance in its hit-queue form.
A change of the builder that moves a count fails here and not silently on the device.  No device needed."""
import ctypes as C
import os

import pytest

import leaf_walk_scenes as L


def _session(lib, obj):
    from raylib_amd import binding
    return binding.SceneSession(lib, obj, L.EYE, L.AT, 45.0, 4 / 3)


def _plan(lib, ses, max_path=5):
    from raylib_amd import binding
    st = binding.RendererSettings(64, 48, 4, int(max_path), 1e-4, 0)
    p = binding.RenderPlan()
    assert lib.RaylibAMD_PlanRender(ses.scene, C.byref(st), 0, 256, 4, C.byref(p)) == 1
    return p.as_dict()


@pytest.fixture(scope="module")
def scene_dir(workdir):
    d = os.path.join(str(workdir), "leaf_walk_host"); os.makedirs(d, exist_ok=True)
    return d


def test_the_soups_cover_every_record_count():
    assert sorted(L.SOUPS) == [1, 2, 3, 4, 5, 6]
    assert [L.records_of(L.SOUPS[r]["leaves"]) for r in sorted(L.SOUPS)] == [1, 2, 3, 4, 5, 6]
    assert L.records_of(L.DENSE["leaves"]) == 6 and L.records_of(L.CORNELL_LEAVES) == 6
    assert [L.records_of(n) for n in (1, 4, 5, 8, 21, 24)] == [1, 1, 2, 2, 6, 6]


@pytest.mark.parametrize("records", sorted(L.SOUPS))
def test_soup_leaf_count(lib, scene_dir, monkeypatch, records):
    for name in ("RAYLIB_HIT_QUEUE", "RAYLIB_LAZY_REFL", "RAYLIB_PLAIN_KERNEL", "RAYLIB_LEAF_LIST", "RAYLIB_LDS_SCENE", "RAYLIB_POOL"):
        monkeypatch.delenv(name, raising=False)
    ses = _session(lib, L.soup_obj(scene_dir, records))
    assert L.leaves_of(lib, ses) == L.SOUPS[records]["leaves"]
    assert lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    p = _plan(lib, ses)
    assert (p["lds"], p["plain"], p["lazy"], p["hitQueue"]) == (2, 1, 1, 1)
    assert (_plan(lib, ses, max_path=0)["lazy"], _plan(lib, ses, max_path=0)["hitQueue"]) == (1, 0)     # k_trace_lazy
    monkeypatch.setenv("RAYLIB_LEAF_LIST", "0")
    assert (_plan(lib, ses)["lds"], _plan(lib, ses)["lazy"]) == (1, 0)                                  # the tree walk the device test compares with
    ses.close()


def test_dense_soup_and_cornell(lib, scene_dir):
    for obj, leaves in ((L.dense_obj(scene_dir), L.DENSE["leaves"]), (L.cornell_obj(scene_dir), L.CORNELL_LEAVES)):
        ses = _session(lib, obj)
        assert L.leaves_of(lib, ses) == leaves
        assert _plan(lib, ses)["lazy"] == 1
        ses.close()
