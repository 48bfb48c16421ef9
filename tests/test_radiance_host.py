"""Path-traced radiance for caller rays (RaylibAMD_TraceRadiance, include/raylib_amd.h) without a device: the record layouts, the planner's choice of tree
(csrc/rl_plan.cc PlanRadiance) with the RAYLIB_QUERY_TREE switch, the refusals that need no device, and the NumPy PCG32 with which
tests/test_gpu_radiance.py forms the renderer's jitter -- checked here against the scalar restatement and the constants of tests/test_gpu_scatter_edges.py
and against the header's arithmetic, so that a wrong jitter is found here and not on the GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from helpers import scenes, ffi
import radiance_cases as rc
import test_gpu_scatter_edges as edges

TREE_BVH2, TREE_GRID4 = 1, 3
F = np.float32


@pytest.fixture(scope="module")
def rad_scenes(lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "radiance_host"); os.makedirs(d, exist_ok=True)

    def obj(path):
        return binding.SceneSession(lib, path, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    S = {"room": obj(scenes.cornell(os.path.join(d, "room.obj"), tess=6, displace_fraction=0.2)[0]),
         "cornell": obj(scenes.cornell(os.path.join(d, "cornell.obj"))[0])}
    quad = [("o_floor", "white", [scenes._quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1))])]
    S["quad"] = obj(scenes.write_obj(os.path.join(d, "quad.obj"), quad, scenes.CORNELL_MTL)[0])
    mats, sph, cub, c = helpers.procedural_case()
    S["procedural"] = binding.ProceduralSession(lib, mats, sph, cub, c["origin"], c["look_at"], c["fov"], c["aspect"], sun=c["sun"], sun_dir=c["sun_dir"],
                                                aperture=c["aperture"], focal=c["focal"], shutter=c["shutter"])
    yield S
    for s in S.values():
        s.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _plan(lib, ses, **kw):
    from raylib_amd import binding
    code, p = binding.plan_radiance(lib, ses.scene, **kw)
    assert code == 1, code
    return p


def test_record_layouts(lib):
    from raylib_amd import binding
    assert C.sizeof(binding.PathRay) == 32 and C.sizeof(binding.RadianceParams) == 28
    assert [getattr(binding.PathRay, f).offset for f in ("org", "time", "dir", "stream")] == [0, 12, 16, 28]
    assert [getattr(binding.RadianceParams, f).offset for f in ("maxPathLength", "rayTMin", "sampleFirst", "sampleCount", "skipDraws", "timeMin", "timeMax")] == \
        [0, 4, 8, 12, 16, 20, 24]
    for name in ("RaylibAMD_TraceRadiance", "RaylibAMD_TraceRadianceDevice", "RaylibAMD_PlanRadiance"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


def test_plan_trees(lib, rad_scenes, monkeypatch):
    S = rad_scenes
    assert lib.RaylibAMD_SceneNumTriangles(S["room"].scene) > 400 and lib.RaylibAMD_SceneNumTriangles(S["quad"].scene) < 8
    n4, st4 = C.c_uint32(), C.c_uint32()
    assert lib.RaylibAMD_SceneBVH4Info(S["room"].scene, C.byref(n4), C.byref(st4)) != 0 and st4.value <= 64
    # a tessellated room: the grid-4 tree, whatever of 4 and 8 is asked for (the 8-wide walk is not fused with shading); 2: the binary tree
    for env in (None, "4", "8", "5"):
        if env is None:
            monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
        else:
            monkeypatch.setenv("RAYLIB_QUERY_TREE", env)
        for name in ("room", "cornell"):
            p = _plan(lib, S[name])
            assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"], p["prims"], p["early"]) == (TREE_GRID4, 4, 64, 32 if st4.value <= 32 or name == "cornell" else 64, 0, 0), (env, name, p)
        # spheres and cubes, and a scene too small for a wide tree: the binary tree
        p = _plan(lib, S["procedural"])
        assert (p["tree"], p["treeWidth"], p["stack"], p["prims"]) == (TREE_BVH2, 2, 32, 1), (env, p)
        p = _plan(lib, S["quad"])
        assert (p["tree"], p["treeWidth"], p["stack"], p["prims"]) == (TREE_BVH2, 2, 32, 0), (env, p)
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "2")
    for name in ("room", "cornell", "procedural", "quad"):
        p = _plan(lib, S[name])
        assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"]) == (TREE_BVH2, 2, 64, 32), (name, p)


def test_refusals_that_need_no_device(lib, rad_scenes):
    from raylib_amd import binding
    ses = rad_scenes["cornell"]
    good = dict(max_path=5, tmin=1e-4, sample_first=0, sample_count=1, skip_draws=3)
    bad = [dict(sample_count=0), dict(skip_draws=65), dict(tmin=-1e-4), dict(tmin=float("nan")), dict(tmin=float("inf")), dict(max_path=-1),
           dict(max_path=32769)]      # (one workgroup's path stack would not fit its 256 MiB: include/raylib_amd.h)
    assert binding.plan_radiance(lib, ses.scene, **good)[0] == 1
    assert binding.plan_radiance(lib, ses.scene, **dict(good, skip_draws=64, max_path=0, tmin=0.0))[0] == 1
    assert binding.plan_radiance(lib, ses.scene, **dict(good, max_path=32768))[0] == 1
    for b in bad:
        assert binding.plan_radiance(lib, ses.scene, **dict(good, **b))[0] == 0, b
    prm = binding.RadianceParams(5, 1e-4, 0, 1, 3, 0.0, 0.0)
    p = binding.QueryPlan()
    assert lib.RaylibAMD_PlanRadiance(ses.scene, None, C.byref(p)) == 0
    assert lib.RaylibAMD_PlanRadiance(ses.scene, C.byref(prm), None) == 0
    assert lib.RaylibAMD_PlanRadiance(None, C.byref(prm), C.byref(p)) == 0
    unfinished = lib.Raylib_CreateScene()
    assert lib.RaylibAMD_PlanRadiance(unfinished, C.byref(prm), C.byref(p)) == 0
    # the trace entries refuse the same before they look for a device, and write nothing
    rays = np.zeros((4, 8), F); rays[:, 1] = 1.0; rays[:, 2] = 4.0; rays[:, 6] = -1.0
    rp = rays.ctypes.data_as(C.POINTER(binding.PathRay))
    out = np.full((4, 4), 7.0, F)
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    for fn, extra in ((lib.RaylibAMD_TraceRadiance, ()), (lib.RaylibAMD_TraceRadianceDevice, (None,))):
        assert fn(ses.scene, C.byref(prm), None, 4, op, *extra) == 0
        assert fn(ses.scene, C.byref(prm), rp, 4, None, *extra) == 0
        assert fn(ses.scene, C.byref(prm), rp, -1, op, *extra) == 0
        assert fn(ses.scene, None, rp, 4, op, *extra) == 0
        assert fn(None, C.byref(prm), rp, 4, op, *extra) == 0
        assert fn(unfinished, C.byref(prm), rp, 4, op, *extra) == 0
        for b in bad:
            kw = dict(good, **b)
            q = binding.RadianceParams(kw["max_path"], kw["tmin"], kw["sample_first"], kw["sample_count"], kw["skip_draws"], 0.0, 0.0)
            assert fn(ses.scene, C.byref(q), rp, 4, op, *extra) == 0, b
    for t in (float("nan"), float("inf")):                      # the host entry: a time that is not finite
        r = rays.copy(); r[2, 3] = t
        assert lib.RaylibAMD_TraceRadiance(ses.scene, C.byref(prm), r.ctypes.data_as(C.POINTER(binding.PathRay)), 4, op) == 0
    for lo, hi in ((1.0, 0.0), (float("nan"), 0.0), (0.0, float("inf"))):   # the device entry: its time interval
        q = binding.RadianceParams(5, 1e-4, 0, 1, 3, lo, hi)
        assert lib.RaylibAMD_TraceRadianceDevice(ses.scene, C.byref(q), rp, 4, op, None) == 0
    lib.Raylib_DestroyScene(unfinished)
    assert (out == 7.0).all()


def _scalar_draws(seed, pixel, sample, k):
    """The first k floats of the stream (seed, pixel, sample) in Python integers, with the pieces of tests/test_gpu_scatter_edges.py"""
    s = edges._mix64(edges._mix64(seed) ^ ((pixel << 32) | sample))
    out = []
    for _ in range(k):
        out.append((edges._pcg_out(s) >> 8) * 2.0 ** -24)
        s = (s * edges.PCG_A + edges.PCG_C) & edges.M64
    return out


def test_numpy_pcg32_is_the_headers_stream(oracle):
    pixels = np.array([0, 1, 31, 63, 100, 767, 2 ** 31, 2 ** 32 - 1], np.uint64)
    for seed in (0, 1, 12345, 2 ** 64 - 1):
        for sample in (0, 1, 3, 2 ** 32 - 1):
            s = rc.stream_begin(seed, pixels, sample)
            got = []
            for _ in range(6):
                f, s = rc.next_float(s)
                assert f.dtype == np.float32
                got.append(f)
            got = np.stack(got, 1)
            want = np.array([_scalar_draws(seed, int(p), sample, 6) for p in pixels], F)
            assert np.array_equal(got, want), (seed, sample)
            if sample == 0:
                assert np.array_equal(got[:, :3], np.array([edges.stream_draws(seed, int(p), 3) for p in pixels], F))
    # the seeds built to draw exactly 0.5 as their stream's second float
    for i in (0, 31, 63, 100):
        seed = edges.seed_for_half(i, 1)
        s = rc.stream_begin(seed, [i], 0)
        _, s = rc.next_float(s)
        assert rc.next_float(s)[0][0] == F(0.5)
    # ... and the shared header as the oracle compiles it: a camera ray's time is its stream's third draw
    cam = ffi.make_camera((0, 0, 0), (0, 0, -1), 60.0, 1.0, 0.5, 1.0, 0.0, 1.0)
    t = oracle.camera_rays(cam, np.full((5, 2), 0.5, F), seed=777)[:, 6]
    s = rc.stream_begin(777, np.arange(5), 0)
    for _ in range(3):
        f, s = rc.next_float(s)
    assert np.array_equal(t, f)


def test_pixel_uv_is_the_renderers_arithmetic():
    w, h, seed = 32, 24, 1
    uv0 = rc.pixel_uv(w, h)
    assert uv0.dtype == np.float32 and uv0.shape == (w * h, 2)
    assert uv0[w + 5, 0] == F(5) / F(w) and uv0[w + 5, 1] == F(1) / F(h)
    for sample in (1, 3):
        uv = rc.pixel_uv(w, h, seed, sample)
        for p in (0, 37, w * h - 1):
            r0, r1 = [F(x) for x in _scalar_draws(seed, p, sample, 2)]
            x, y = p % w, p // w
            u = F(F(x) / F(w)) + F(F(F(r0 - F(0.5)) * F(2.0)) / F(w))
            v = F(F(y) / F(h)) + F(F(F(r1 - F(0.5)) * F(2.0)) / F(h))
            assert uv[p, 0] == F(u) and uv[p, 1] == F(v), (sample, p)
        assert (np.abs(uv - uv0) <= np.array([1.0 / w, 1.0 / h], F)).all() and (uv != uv0).any()


def test_mean_in_order_is_float32():
    a = np.array([[1e8, 1.0, 0.25, 9.0]], F); b = np.array([[1.0, 1.0, 0.25, 9.0]], F); c = np.array([[-1e8, 1.0, 0.25, 9.0]], F)
    m = rc.mean_in_order([a, b, c])
    assert m.dtype == np.float32 and m[0, 0] == 0.0 and m[0, 1] == F(3.0) * (F(1) / F(3)) and m[0, 3] == 1.0   # (1e8 + 1 rounds to 1e8 in float)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-device path: this machine may have a GPU")
def test_trace_without_a_device_returns_0(lib, rad_scenes):
    from raylib_amd import binding
    ses = rad_scenes["cornell"]
    rays = np.zeros((4, 8), F); rays[:, 1] = 1.0; rays[:, 2] = 4.0; rays[:, 6] = -1.0
    prm = binding.RadianceParams(5, 1e-4, 0, 1, 3, 0.0, 0.0)
    out = np.full((4, 4), 7.0, F)
    rp, op = rays.ctypes.data_as(C.POINTER(binding.PathRay)), out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.RaylibAMD_TraceRadiance(ses.scene, C.byref(prm), rp, 4, op) == 0
    assert lib.RaylibAMD_TraceRadianceDevice(ses.scene, C.byref(prm), rp, 4, op, None) == 0
    assert (out == 7.0).all()
    with pytest.raises(RuntimeError):
        binding.trace_radiance(lib, ses.scene, rays)
