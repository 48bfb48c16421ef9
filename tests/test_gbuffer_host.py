"""The primary-hit G-buffer (include/raylib_amd.h, statements G1 to G6) where no device is needed: the planner, and every refusal of G6 that is made before the
device is asked for.  A missing export fails these tests (the binding raises on load, and the calls below name the exports themselves).

(A BVH deeper than 64 levels cannot be had from the builder, whose own bound is 61 -- tests/stack_edges.py deepest_triangles --, so that refusal, and
RaylibAMD_PlanGBuffer's -1, are not reachable from here, as in tests/test_ray_query_all_host.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from raylib_amd import binding

SENTINEL = 0xA5
W, H = 37, 21
PLANE_BYTES = {k: 44 if k == "surface" else 16 for k in binding.GBUFFER_PLANES}


@pytest.fixture(scope="module")
def scenes3(lib, workdir):
    """cornell, cornell tess 4 (both wide trees) and the procedural scene (spheres, cubes: the binary tree only)"""
    d = os.path.join(str(workdir), "gbuffer_host"); os.makedirs(d, exist_ok=True)
    cornell = binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "c.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    tess4 = binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "c4.obj"), tess=4)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    mats, sph, cub, cam = helpers.procedural_case()
    proc = binding.ProceduralSession(lib, mats, sph, cub, origin=cam["origin"], look_at=cam["look_at"], fov=cam["fov"], aspect=cam["aspect"], shutter=cam["shutter"])
    yield {"cornell": cornell, "cornell_tess4": tess4, "procedural": proc}
    for s in (cornell, tess4, proc):
        s.close()


@pytest.mark.parametrize("tree", [None, "2", "4", "8"])
def test_plan_is_the_surface_querys(lib, scenes3, monkeypatch, tree):
    if tree is None:
        monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    else:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
    seen = set()
    for name, ses in scenes3.items():
        rc, plan = binding.plan_gbuffer(lib, ses.scene)
        rq, want = binding.plan_ray_query(lib, ses.scene, binding.QUERY_SURFACE)
        assert rc == rq == 1 and plan == want, (name, plan, want)
        assert plan["early"] == 0 and plan["prims"] == int(name == "procedural")
        seen.add((name, plan["treeWidth"]))
    assert ("procedural", 2) in seen                      # spheres and cubes: the binary tree whatever is asked for
    n4, n8 = C.c_uint32(), C.c_uint32()
    t4 = scenes3["cornell_tess4"]
    assert lib.RaylibAMD_SceneBVH4Info(t4.scene, C.byref(n4), C.byref(C.c_uint32())) == 1 and n4.value > 0
    assert lib.RaylibAMD_SceneBVH8Info(t4.scene, C.byref(n8), C.byref(C.c_uint32()), C.byref(C.c_float()), C.byref(C.c_float())) == 1 and n8.value > 0
    assert ("cornell_tess4", {None: 8, "2": 2, "4": 4, "8": 8}[tree]) in seen


def test_plan_refusals(lib, scenes3):
    p = binding.QueryPlan()
    raw = lib.Raylib_CreateScene()
    try:
        assert lib.RaylibAMD_PlanGBuffer(None, C.byref(p)) == 0
        assert lib.RaylibAMD_PlanGBuffer(scenes3["cornell"].scene, None) == 0
        assert lib.RaylibAMD_PlanGBuffer(raw, C.byref(p)) == 0          # not finalized
    finally:
        lib.Raylib_DestroyScene(raw)


def _sentinel_planes(w=W, h=H, names=binding.GBUFFER_PLANES):
    bufs = {k: np.full(w * h * PLANE_BYTES[k], SENTINEL, np.uint8) for k in names}
    return bufs, binding.GBufferPlanes(**{k: v.ctypes.data for k, v in bufs.items()})


def test_refusals_write_nothing(lib, scenes3):
    """G6, the refusals that need no device, through the host entry: 0, and the sentinel-filled planes are untouched."""
    ses = scenes3["cornell"]
    raw = lib.Raylib_CreateScene()
    ok = binding.RendererSettings(W, H, 1, 1, 1e-4, 0)
    bufs, planes = _sentinel_planes()
    none = binding.GBufferPlanes()
    cases = {
        "null settings": (None, ses.scene, ses.camera, C.byref(planes)),
        "null scene": (C.byref(ok), None, ses.camera, C.byref(planes)),
        "null camera": (C.byref(ok), ses.scene, None, C.byref(planes)),
        "null planes": (C.byref(ok), ses.scene, ses.camera, None),
        "no plane asked for": (C.byref(ok), ses.scene, ses.camera, C.byref(none)),
        "W = 0": (C.byref(binding.RendererSettings(0, H, 1, 1, 1e-4, 0)), ses.scene, ses.camera, C.byref(planes)),
        "H = 0": (C.byref(binding.RendererSettings(W, 0, 1, 1, 1e-4, 0)), ses.scene, ses.camera, C.byref(planes)),
        "W * H = 2^31": (C.byref(binding.RendererSettings(1 << 16, 1 << 15, 1, 1, 1e-4, 0)), ses.scene, ses.camera, C.byref(planes)),
        "rayTMin NaN": (C.byref(binding.RendererSettings(W, H, 1, 1, float("nan"), 0)), ses.scene, ses.camera, C.byref(planes)),
        "rayTMin inf": (C.byref(binding.RendererSettings(W, H, 1, 1, float("inf"), 0)), ses.scene, ses.camera, C.byref(planes)),
        "rayTMin -inf": (C.byref(binding.RendererSettings(W, H, 1, 1, float("-inf"), 0)), ses.scene, ses.camera, C.byref(planes)),
        "scene not finalized": (C.byref(ok), raw, ses.camera, C.byref(planes)),
    }
    try:
        for what, args in cases.items():
            assert lib.RaylibAMD_RenderGBuffer(*args) == 0, what
            assert lib.RaylibAMD_RenderGBufferDevice(*args, None) == 0, what
            for k, v in bufs.items():
                assert (v == SENTINEL).all(), (what, k)
    finally:
        lib.Raylib_DestroyScene(raw)


def test_images_entry_refusals(lib, scenes3):
    """G6 on the images entry: both handles 0, the same image twice, a handle that is unknown -- and the images keep their size."""
    ses = scenes3["cornell"]
    st = binding.RendererSettings(W, H, 1, 1, 1e-4, 0)
    a, b = lib.Raylib_CreateImage(5, 3), lib.Raylib_CreateImage(5, 3)
    gone = lib.Raylib_CreateImage(5, 3)
    assert lib.Raylib_DestroyImage(gone) == 1
    try:
        assert lib.RaylibAMD_RenderGuides(C.byref(st), ses.scene, ses.camera, None, None) == 0
        assert lib.RaylibAMD_RenderGuides(C.byref(st), ses.scene, ses.camera, a, a) == 0
        assert lib.RaylibAMD_RenderGuides(C.byref(st), ses.scene, ses.camera, a, gone) == 0
        assert lib.RaylibAMD_RenderGuides(C.byref(st), ses.scene, ses.camera, gone, None) == 0
        assert lib.RaylibAMD_RenderGuides(None, ses.scene, ses.camera, a, b) == 0
        assert lib.RaylibAMD_RenderGuides(C.byref(binding.RendererSettings(W, H, 1, 1, float("nan"), 0)), ses.scene, ses.camera, a, b) == 0
        for img in (a, b):
            w, h = C.c_uint32(), C.c_uint32()
            assert lib.RaylibAMD_ImageSize(img, C.byref(w), C.byref(h)) == 1 and (w.value, h.value) == (5, 3)
    finally:
        lib.Raylib_DestroyImage(a); lib.Raylib_DestroyImage(b)
