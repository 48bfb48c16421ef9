"""Batched ray queries (RaylibAMD_TraceRays, include/raylib_amd.h) without a device: the record layouts, the planner's choice of tree
(csrc/rl_plan.cc PlanQuery) with the RAYLIB_QUERY_TREE switch and its fall-backs, and the refusals.  tests/test_gpu_ray_query.py checks the results."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import scenes, ffi

TREE_BVH2, TREE_GRID4, TREE_WIDE8 = 1, 3, 4
POOL8_MAXLEVELS = 16


def _write_soup(path, n_soup, n_chain):
    """As tests/test_render_plan_host.py: n_soup triangles of about the scene's size, then a chain of n_chain ever smaller triangles (a deep BVH2)."""
    rng = np.random.RandomState(3)
    lines, k = ["o soup\n"], 0
    tris = [c + rng.uniform(-1.0, 1.0, (3, 3)) for c in rng.uniform(-1.0, 1.0, (n_soup, 3))]
    for j in range(1, n_chain + 1):
        c = 2.0 ** -j
        tris.append(np.array([[c, 0, 0], [c + c / 2, 0, 0], [c, c / 2, 0]]))
    for p in tris:
        for q in p:
            lines.append("v %.9g %.9g %.9g\n" % tuple(q))
        lines.append("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))
        k += 1
    with open(path, "w") as f:
        f.write("".join(lines))
    return path


@pytest.fixture(scope="module")
def query_scenes(lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "ray_query_host"); os.makedirs(d, exist_ok=True)

    def obj(path):
        return binding.SceneSession(lib, path, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    S = {"cornell": obj(scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
         "soup": obj(_write_soup(os.path.join(d, "soup.obj"), 1000, 0)),
         "deep": obj(_write_soup(os.path.join(d, "deep.obj"), 1000, 72))}
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    S["spheres"] = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)],
                                             [dict(minBounds=(1, 0, 0), maxBounds=(1.5, 0.5, 0.5), timeStartMove=0.0, velocity=(0.0, 0.5, 0.0), material=0)])
    yield S
    for s in S.values():
        s.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _bvh(lib, ses):
    n, d, s = C.c_uint32(), C.c_uint32(), C.c_float()
    lib.RaylibAMD_SceneBVHInfo(ses.scene, C.byref(n), C.byref(d), C.byref(s))
    n4, st4 = C.c_uint32(), C.c_uint32()
    has4 = lib.RaylibAMD_SceneBVH4Info(ses.scene, C.byref(n4), C.byref(st4)) != 0
    n8, lv, s4, s8 = C.c_uint32(0), C.c_uint32(0), C.c_float(0), C.c_float(0)
    has8 = lib.RaylibAMD_SceneBVH8Info(ses.scene, C.byref(n8), C.byref(lv), C.byref(s4), C.byref(s8)) != 0
    return dict(depth=d.value, has4=has4, stack4=st4.value, has8=has8, levels8=lv.value)


def _plan(lib, ses, kind=1):
    from raylib_amd import binding
    rc, p = binding.plan_ray_query(lib, ses.scene, kind)
    assert rc == 1, rc
    return p


def test_record_layouts(lib):
    from raylib_amd import binding
    assert C.sizeof(binding.Ray) == 32 and C.sizeof(binding.HitT) == 16
    assert [getattr(binding.Ray, f).offset for f in ("org", "tMin", "dir", "tMax")] == [0, 12, 16, 28]
    assert [getattr(binding.HitT, f).offset for f in ("t", "prim", "b1", "b2")] == [0, 4, 8, 12]
    assert binding.HITT_DTYPE.itemsize == 16 and binding.SURFACE_DTYPE == ffi.HIT_DTYPE and binding.SURFACE_DTYPE.itemsize == 44
    assert (binding.QUERY_ANY, binding.QUERY_CLOSEST, binding.QUERY_SURFACE) == (0, 1, 2)
    assert (binding.PRIM_SPHERE, binding.PRIM_CUBE) == (0x10000000, 0x20000000)
    for name in ("RaylibAMD_TraceRays", "RaylibAMD_TraceRaysDevice", "RaylibAMD_PlanRayQuery"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


def test_plan_default_trees(lib, query_scenes):
    S = query_scenes
    # the soup carries an 8-wide tree of few levels: walked by every kind
    b = _bvh(lib, S["soup"])
    assert b["has8"] and b["levels8"] <= POOL8_MAXLEVELS, b
    for kind in (0, 1, 2):
        p = _plan(lib, S["soup"], kind)
        assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"], p["prims"]) == (TREE_WIDE8, 8, 80, 2 * POOL8_MAXLEVELS, 0), p
        assert p["early"] == (kind == 0)
    # Cornell has no 8-wide tree (the builder makes one only where rays are expected to take many steps): the grid-4 tree
    b = _bvh(lib, S["cornell"])
    assert not b["has8"] and b["has4"] and b["stack4"] <= 32, b
    for kind in (0, 1, 2):
        p = _plan(lib, S["cornell"], kind)
        assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"], p["prims"], p["early"]) == (TREE_GRID4, 4, 64, 32, 0, int(kind == 0)), p
    # spheres and cubes: the binary tree, and the occlusion query walks to the closest hit (a sphere's interval is open at tMax)
    for kind in (0, 1, 2):
        p = _plan(lib, S["spheres"], kind)
        assert (p["tree"], p["treeWidth"], p["stack"], p["prims"], p["early"]) == (TREE_BVH2, 2, 32, 1, 0), p


def test_plan_forced_trees_and_fallbacks(lib, query_scenes, monkeypatch):
    S = query_scenes
    b = _bvh(lib, S["soup"])
    assert b["has4"] and b["stack4"] <= 64 and b["depth"] <= 32, b
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "4")
    p = _plan(lib, S["soup"])
    assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"]) == (TREE_GRID4, 4, 64, 32 if b["stack4"] <= 32 else 64), p
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "2")
    p = _plan(lib, S["soup"])
    assert (p["tree"], p["treeWidth"], p["stack"]) == (TREE_BVH2, 2, 32), p
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "8")
    assert _plan(lib, S["soup"])["tree"] == TREE_WIDE8
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "5")          # not a tree: the default
    assert _plan(lib, S["soup"])["tree"] == TREE_WIDE8
    # the deep chain: BVH2 deeper than 32 and a 4-wide stack need above 64, but an 8-wide tree of few levels
    b = _bvh(lib, S["deep"])
    assert b["depth"] > 32 and b["stack4"] > 64 and b["levels8"] <= POOL8_MAXLEVELS, b
    monkeypatch.delenv("RAYLIB_QUERY_TREE")
    assert _plan(lib, S["deep"])["tree"] == TREE_WIDE8
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "4")          # no grid tree it could walk: the binary tree, 64 deep
    p = _plan(lib, S["deep"])
    assert (p["tree"], p["treeWidth"], p["stack"]) == (TREE_BVH2, 2, 64), p
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "2")
    assert (_plan(lib, S["deep"])["tree"], _plan(lib, S["deep"])["stack"]) == (TREE_BVH2, 64)
    # Cornell: 8 asked for, no 8-wide tree -- the grid; 2 -- the binary tree
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "8")
    assert _plan(lib, S["cornell"])["tree"] == TREE_GRID4
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "2")
    assert (_plan(lib, S["cornell"])["tree"], _plan(lib, S["cornell"])["stack"]) == (TREE_BVH2, 32)
    # spheres: whatever is asked for, the binary tree
    for v in ("8", "4", "2"):
        monkeypatch.setenv("RAYLIB_QUERY_TREE", v)
        assert _plan(lib, S["spheres"])["tree"] == TREE_BVH2


def test_plan_refusals(lib, query_scenes):
    from raylib_amd import binding
    S = query_scenes
    p = binding.QueryPlan()
    assert lib.RaylibAMD_PlanRayQuery(S["cornell"].scene, 3, C.byref(p)) == 0
    assert lib.RaylibAMD_PlanRayQuery(S["cornell"].scene, -1, C.byref(p)) == 0
    assert lib.RaylibAMD_PlanRayQuery(S["cornell"].scene, 1, None) == 0
    assert lib.RaylibAMD_PlanRayQuery(None, 1, C.byref(p)) == 0
    unfinished = lib.Raylib_CreateScene()
    assert lib.RaylibAMD_PlanRayQuery(unfinished, 1, C.byref(p)) == 0
    lib.Raylib_DestroyScene(unfinished)


def _rays(n):
    r = np.zeros((n, 8), np.float32)
    r[:, 1] = 1.0; r[:, 2] = 4.0; r[:, 6] = -1.0; r[:, 3] = 1e-4; r[:, 7] = 3.4028235e38
    return r


def test_trace_refuses_bad_arguments_before_the_device(lib, query_scenes):
    """Null pointers with n > 0, a negative n, an unknown kind, a ray time that is not finite and an unfinished scene are refused whether or not there is a device, and nothing is written."""
    from raylib_amd import binding
    ses = query_scenes["cornell"]
    rays = _rays(4)
    rp = rays.ctypes.data_as(C.POINTER(binding.Ray))
    out = np.full(4 * 16, 0x5a, np.uint8)
    for fn, extra in ((lib.RaylibAMD_TraceRays, ()), (lib.RaylibAMD_TraceRaysDevice, (None,))):
        assert fn(ses.scene, 1, None, 4, 0.0, out.ctypes.data, None, *extra) == 0
        assert fn(ses.scene, 1, rp, 4, 0.0, None, None, *extra) == 0
        assert fn(ses.scene, 1, rp, -1, 0.0, out.ctypes.data, None, *extra) == 0
        assert fn(ses.scene, 3, rp, 4, 0.0, out.ctypes.data, None, *extra) == 0
        for t in (float("nan"), float("inf"), float("-inf")):           # a ray time that is not finite
            assert fn(query_scenes["spheres"].scene, 1, rp, 4, t, out.ctypes.data, None, *extra) == 0
            assert fn(ses.scene, 1, rp, 4, t, out.ctypes.data, None, *extra) == 0
        assert fn(None, 1, rp, 4, 0.0, out.ctypes.data, None, *extra) == 0
        unfinished = lib.Raylib_CreateScene()
        assert fn(unfinished, 1, rp, 4, 0.0, out.ctypes.data, None, *extra) == 0
        lib.Raylib_DestroyScene(unfinished)
    assert (out == 0x5a).all()
    with pytest.raises(ValueError):
        binding.trace_rays(lib, ses.scene, rays, 7)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-device path: this machine may have a GPU")
def test_trace_without_a_device_returns_0(lib, query_scenes):
    from raylib_amd import binding
    ses = query_scenes["cornell"]
    rays = _rays(4)
    out = np.full(4, 7, np.uint32)
    for kind in (0, 1, 2):
        assert lib.RaylibAMD_TraceRays(ses.scene, kind, rays.ctypes.data_as(C.POINTER(binding.Ray)), 4, 0.0, out.ctypes.data, None) == 0
        assert lib.RaylibAMD_TraceRaysDevice(ses.scene, kind, rays.ctypes.data_as(C.POINTER(binding.Ray)), 4, 0.0, out.ctypes.data, None, None) == 0
    assert (out == 7).all()
    with pytest.raises(RuntimeError):
        binding.trace_rays(lib, ses.scene, rays, binding.QUERY_CLOSEST)
