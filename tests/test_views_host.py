"""Several views of one scene in one launch (RaylibAMD_RenderViews): the batch's job list and plan through RaylibAMD_PlanViews.  No device needed;
tests/test_gpu_views.py renders the batches."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import scenes

SWITCHES = ("RAYLIB_POOL", "RAYLIB_POOL_MIN_TRIS", "RAYLIB_POOL_SHORT_STACK", "RAYLIB_BVH4", "RAYLIB_BVH8", "RAYLIB_LDS_SCENE", "RAYLIB_LEAF_LIST",
            "RAYLIB_PLAIN_KERNEL", "RAYLIB_SAMPLE_BATCH", "RAYLIB_SAMPLE_BUFFER_GIB", "RAYLIB_JOB_CHUNK", "RAYLIB_JOB_HEADS", "RAYLIB_GUIDED",
            "RAYLIB_BLOCKS_PER_CU", "RAYLIB_CULL_CELLS")
PLAN_KEYS = ("pathTrace", "stack", "prims", "poolK", "tree", "lstack", "lds", "plain", "pathsPerWave", "treeWidth", "nodeBytes", "keepNodes4", "keepNodes4f", "eagerTree")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def view_scenes(lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "views_host"); os.makedirs(d, exist_ok=True)
    S = {}
    S["cornell"] = binding.SceneSession(lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    S["cornell_sun"] = binding.SceneSession(lib, scenes.cornell(os.path.join(d, "cornell_sun.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0,
                                            sun=(9.0, 8.0, 7.0), sun_dir=(-1.0, -1.0, 0.0))
    S["mid"] = binding.SceneSession(lib, scenes.cornell(os.path.join(d, "mid.obj"), tess=24, displace_fraction=0.2)[0], (0, 1, 5), (0, 1, -1), 60.0, 1.5,
                                    sun=(20, 20, 20), sun_dir=(-1.0, -1.0, 0.0))
    yield S
    for s in S.values():
        s.close()


def _bounds(ses):
    tris, _ = ses.export_flat()
    pts = np.concatenate([tris["v0"], tris["v1"], tris["v2"]])
    return np.concatenate([pts.min(0), pts.max(0)]).astype(np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _random_cameras(lib, rng, n, aspect):
    from raylib_amd import binding
    cams = []
    for _ in range(n):
        kind = rng.randint(4)
        if kind == 0:     # far away: most cells miss the room
            origin = (rng.uniform(-3, 3), rng.uniform(0, 3), rng.uniform(9, 20))
        elif kind == 1:   # inside the room
            origin = (rng.uniform(-0.5, 0.5), rng.uniform(0.5, 1.5), rng.uniform(-0.5, 0.8))
        else:
            origin = (rng.uniform(-6, 6), rng.uniform(-2, 5), rng.uniform(2, 8))
        look = (rng.uniform(-0.5, 0.5), rng.uniform(0.5, 1.5), rng.uniform(-1.5, 0.0))
        aperture = rng.choice([0.0, 0.0, 0.01, 0.3])
        cams.append(binding.create_camera(lib, origin, look, rng.uniform(20.0, 80.0), aspect, aperture=aperture, focal=rng.uniform(1.0, 6.0)))
    return cams


def plan_views(lib, ses, cams, w, h, spp, mode=0, sky=False, cus=256, per_cu=4):
    from raylib_amd import binding
    st = binding.RendererSettings(w, h, spp, 5, 1e-4, mode)
    out = binding.RenderPlan()
    cells = ((w + 7) // 8) * ((h + 7) // 8)
    empty = np.full(len(cams) * cells, 7, np.uint8)
    rc = lib.RaylibAMD_PlanViews(ses.scene, C.byref(st), binding.handle_array(cams), len(cams), int(sky), cus, per_cu, C.byref(out),
                                 empty.ctypes.data_as(C.POINTER(C.c_uint8)))
    return rc, out.as_dict(), empty.reshape(len(cams), cells)


def plan_one(lib, ses, w, h, spp, mode=0, sky=False, cus=256, per_cu=4):
    from raylib_amd import binding
    st = binding.RendererSettings(w, h, spp, 5, 1e-4, mode)
    out = binding.RenderPlan()
    assert lib.RaylibAMD_PlanRender(ses.scene, C.byref(st), int(sky), cus, per_cu, C.byref(out)) == 1
    return out.as_dict()


def test_binding_exposes_the_views_calls(lib):
    from raylib_amd import binding
    for name in ("RaylibAMD_RenderViews", "RaylibAMD_RenderViewsDevice", "RaylibAMD_PlanViews"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS, name
        assert hasattr(lib, name), name
    assert binding.MAX_VIEWS == 64
    assert callable(getattr(binding.SceneSession, "render_views", None))


@pytest.mark.parametrize("name", ["cornell", "cornell_sun", "mid"])
def test_dropped_cells_are_each_views_cull(lib, view_scenes, name):
    """The batch's dropped cells, view by view, are what RaylibAMD_CullCells says for that view's camera; the jobs are 64 x samples x listed cells."""
    ses = view_scenes[name]
    bounds = _bounds(ses)
    sun, sd = np.zeros(3, np.float32), np.zeros(3, np.float32)
    lib.RaylibAMD_SceneGetSun(ses.scene, _fp(sun), _fp(sd))
    rng = np.random.RandomState(11 + len(name))
    dropped_somewhere = 0
    for (w, h, spp, n) in ((44, 36, 4, 6), (200, 120, 3, 3), (67, 41, 1, 16)):
        cams = _random_cameras(lib, rng, n, w / h)
        try:
            rc, p, empty = plan_views(lib, ses, cams, w, h, spp)
            assert rc == 1, rc
            cells = ((w + 7) // 8) * ((h + 7) // 8)
            for v, cam in enumerate(cams):
                flags = np.zeros(cells, np.uint8)
                k = lib.RaylibAMD_CullCells(cam, _fp(bounds), _fp(sun), _fp(sd), w, h, flags.ctypes.data_as(C.POINTER(C.c_uint8)), None)
                assert np.array_equal(empty[v], flags), (name, v, w, h)
                assert int(empty[v].sum()) == max(0, k)
            listed = int((empty == 0).sum())
            dropped_somewhere += int(empty.sum() > 0)
            assert p["sampleCount"] == spp and p["batch"] == spp
            assert p["jobs"] == 64 * spp * listed, (p["jobs"], listed)
        finally:
            for c in cams:
                lib.Raylib_DestroyCamera(c)
    assert dropped_somewhere > 0


def test_instance_and_tree_are_the_one_view_plans(lib, view_scenes, monkeypatch):
    """One kernel choice for the batch: the instance and tree of RaylibAMD_PlanRender for the same settings, under the switches of the planner's tests."""
    from raylib_amd import binding
    cases = [dict(), dict(RAYLIB_POOL="0"), dict(RAYLIB_BVH8="1"), dict(RAYLIB_BVH4="0"), dict(RAYLIB_LEAF_LIST="0"), dict(RAYLIB_PLAIN_KERNEL="0"),
             dict(RAYLIB_LDS_SCENE="0"), dict(RAYLIB_POOL="3"), dict(RAYLIB_POOL="4"), dict(RAYLIB_POOL_SHORT_STACK="0"), dict(RAYLIB_POOL_MIN_TRIS="100000"),
             dict(RAYLIB_SAMPLE_BATCH="3"), dict(RAYLIB_JOB_HEADS="1"), dict(RAYLIB_CULL_CELLS="0")]
    for name, ses in view_scenes.items():
        cams = [binding.create_camera(lib, (0, 1, 4), (0, 1, -1), 45.0, 1.0), binding.create_camera(lib, (0.3, 1.2, 9), (0, 1, -1), 30.0, 1.0)]
        try:
            for env in cases:
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                for mode, sky in ((0, False), (0, True), (1, False), (3, False)):
                    rc, pv, _ = plan_views(lib, ses, cams, 64, 64, 8, mode=mode, sky=sky)
                    assert rc == 1
                    p1 = plan_one(lib, ses, 64, 64, 8, mode=mode, sky=sky)
                    assert {k: pv[k] for k in PLAN_KEYS} == {k: p1[k] for k in PLAN_KEYS}, (name, env, mode, sky)
                    if env.get("RAYLIB_SAMPLE_BATCH") == "3" and mode == 0:
                        assert pv["batch"] == 3 and pv["sampleCount"] == 3
                for k in env:
                    monkeypatch.delenv(k)
        finally:
            for c in cams:
                lib.Raylib_DestroyCamera(c)


def test_every_cell_listed_without_the_cull(lib, view_scenes, monkeypatch):
    from raylib_amd import binding
    ses = view_scenes["cornell"]
    cams = [binding.create_camera(lib, (0, 1, 20), (0, 1, -1), 30.0, 1.0) for _ in range(3)]
    try:
        rc, p, empty = plan_views(lib, ses, cams, 44, 36, 2)
        assert rc == 1 and empty.sum() > 0
        monkeypatch.setenv("RAYLIB_CULL_CELLS", "0")
        rc, p, empty = plan_views(lib, ses, cams, 44, 36, 2)
        assert rc == 1 and empty.sum() == 0 and p["jobs"] == 64 * 2 * 3 * 6 * 5
    finally:
        for c in cams:
            lib.Raylib_DestroyCamera(c)


def test_plan_refuses_bad_arguments(lib, view_scenes):
    from raylib_amd import binding
    ses = view_scenes["cornell"]
    st = binding.RendererSettings(44, 36, 2, 5, 1e-4, 0)
    out = binding.RenderPlan()
    cams = [binding.create_camera(lib, (0, 1, 4), (0, 1, -1), 45.0, 1.0) for _ in range(65)]
    try:
        arr = binding.handle_array(cams)
        assert lib.RaylibAMD_PlanViews(ses.scene, C.byref(st), arr, 2, 0, 256, 4, C.byref(out), None) == 1
        assert lib.RaylibAMD_PlanViews(ses.scene, C.byref(st), arr, 64, 0, 256, 4, C.byref(out), None) == 1
        for count in (0, -1, 65):
            assert lib.RaylibAMD_PlanViews(ses.scene, C.byref(st), arr, count, 0, 256, 4, C.byref(out), None) == 0, count
        assert lib.RaylibAMD_PlanViews(None, C.byref(st), arr, 2, 0, 256, 4, C.byref(out), None) == 0
        assert lib.RaylibAMD_PlanViews(ses.scene, None, arr, 2, 0, 256, 4, C.byref(out), None) == 0
        assert lib.RaylibAMD_PlanViews(ses.scene, C.byref(st), None, 2, 0, 256, 4, C.byref(out), None) == 0
        assert lib.RaylibAMD_PlanViews(ses.scene, C.byref(st), arr, 2, 0, 256, 4, None, None) == 0
        assert lib.RaylibAMD_PlanViews(ses.scene, C.byref(st), binding.handle_array([cams[0], 0]), 2, 0, 256, 4, C.byref(out), None) == 0
        assert lib.RaylibAMD_PlanViews(ses.scene, C.byref(st), binding.handle_array([cams[0], 12345]), 2, 0, 256, 4, C.byref(out), None) == 0
        empty_vp = binding.RendererSettings(0, 36, 2, 5, 1e-4, 0)
        assert lib.RaylibAMD_PlanViews(ses.scene, C.byref(empty_vp), arr, 2, 0, 256, 4, C.byref(out), None) == 0
        huge = binding.RendererSettings(16384, 16384, 1, 5, 1e-4, 0)   # 4.2 M cells x 64 views x 64 jobs: beyond the job counter
        assert lib.RaylibAMD_PlanViews(ses.scene, C.byref(huge), arr, 64, 0, 256, 4, C.byref(out), None) == 0
        unfinalized = lib.Raylib_CreateScene()
        assert lib.RaylibAMD_PlanViews(unfinalized, C.byref(st), arr, 2, 0, 256, 4, C.byref(out), None) == 0
        lib.Raylib_DestroyScene(unfinalized)
    finally:
        for c in cams:
            lib.Raylib_DestroyCamera(c)


def test_render_refuses_bad_arguments_without_a_device(lib, view_scenes):
    """The render calls refuse what the plan refuses before they look for a device (these run on the build host too)."""
    from raylib_amd import binding
    ses = view_scenes["cornell"]
    st = binding.RendererSettings(44, 36, 2, 5, 1e-4, 0)
    cams = [binding.create_camera(lib, (0, 1, 4), (0, 1, -1), 45.0, 1.0) for _ in range(2)]
    imgs = [lib.Raylib_CreateImage(4, 4) for _ in range(2)]
    try:
        ca, ia = binding.handle_array(cams), binding.handle_array(imgs)
        assert lib.RaylibAMD_RenderViews(C.byref(st), ses.scene, ca, 0, ia) == 0
        assert lib.RaylibAMD_RenderViews(C.byref(st), ses.scene, ca, 65, ia) == 0
        assert lib.RaylibAMD_RenderViews(C.byref(st), ses.scene, ca, 2, None) == 0
        assert lib.RaylibAMD_RenderViews(C.byref(st), ses.scene, ca, 2, binding.handle_array([imgs[0], imgs[0]])) == 0
        assert lib.RaylibAMD_RenderViews(C.byref(st), ses.scene, binding.handle_array([cams[0], 0]), 2, ia) == 0
        assert lib.RaylibAMD_RenderViewsDevice(C.byref(st), ses.scene, ca, 0, None) == 0
        assert lib.RaylibAMD_RenderViewsDevice(None, ses.scene, ca, 2, None) == 0
        w, h = C.c_uint32(), C.c_uint32()
        for ih in imgs:   # refused: no image touched
            lib.RaylibAMD_ImageSize(ih, C.byref(w), C.byref(h))
            assert (w.value, h.value) == (4, 4)
    finally:
        for c in cams:
            lib.Raylib_DestroyCamera(c)
        for ih in imgs:
            lib.Raylib_DestroyImage(ih)
