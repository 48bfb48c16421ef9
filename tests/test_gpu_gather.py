"""Irradiance and SH probes gathered at caller points (RaylibAMD_Gather, include/raylib_amd.h) on the device, held to the header's contract statement by
statement: the direction against the Lambertian material's scattering event (RaylibAMD_EvalScatter) and the NumPy restatement (tests/gather_cases.py); the
radiance against RaylibAMD_TraceRadiance along that direction; the value and the result against the restatement -- bit for bit, on every point.  Then the job
space's edges, calls cut into several launches, the device entry, a closed-form estimate that pins the solid angles and the basis constants, and the stats."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch    # before the library is loaded: test_device_entry hands it torch's tensors, and both must run on one HIP runtime

import helpers
from helpers import ffi
import radiance_cases as rc
import gather_cases as gc

pytestmark = pytest.mark.gpu

with open(os.path.join(helpers.ROOT, "software-raytracing_amd", "csrc", "rl_kernels.h")) as _f:
    QUERY_CHUNK = int(re.search(r"^#define RL_QUERY_CHUNK (\d+)u$", _f.read(), re.M).group(1))
F = np.float32
SCENES = ["cornell", "cornell_glass_sun", "cutout_sky", "procedural"]
KINDS = [gc.IRRADIANCE, gc.SH9]
MIN_POINTS = 2 * QUERY_CHUNK + 2


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    eq = helpers.same(got, want).reshape(len(got), -1).all(-1)
    assert eq.all(), "%s: %d of %d records differ (first at %d: %s against %s)" % (what, (~eq).sum(), len(eq), np.nonzero(~eq)[0][0],
                                                                                   got[~eq][0].tolist(), want[~eq][0].tolist())


def _stats(lib):
    from raylib_amd import binding
    st = binding.Stats()
    lib.RaylibAMD_GetLastStats(C.byref(st))
    return st


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    monkeypatch.delenv("RAYLIB_GATHER_BATCH", raising=False)


@pytest.fixture(scope="module")
def procedural(gpu_lib):
    from raylib_amd import binding
    mats, sph, cub, c = helpers.procedural_case()
    ses = binding.ProceduralSession(gpu_lib, mats, sph, cub, c["origin"], c["look_at"], c["fov"], c["aspect"], sun=c["sun"], sun_dir=c["sun_dir"],
                                    aperture=c["aperture"], focal=c["focal"], shutter=c["shutter"])
    yield ses
    ses.close()


@pytest.fixture(scope="module")
def cases(gpu_lib, sessions, procedural):
    """name -> (session, points): the surface points a 16 x 12 frame of the session's camera rays meets (RaylibAMD_TraceRays SURFACE), with the hit's normal, the
    camera ray's time (the procedural session's shutter is open: its cube moves) and the point's index as its stream; repeated, on further streams, up to
    MIN_POINTS points."""
    from raylib_amd import binding
    out = {}
    for name in SCENES:
        ses = procedural if name == "procedural" else sessions[name]
        rays = rc.frame_rays(gpu_lib, ses, 16, 12)
        q = helpers.rays8(rays[:, 0:3], rays[:, 4:7])
        hits = binding.trace_rays(gpu_lib, ses.scene, q, binding.QUERY_SURFACE)
        ok = hits["hit"] != 0
        assert ok.sum() >= 32, (name, int(ok.sum()))
        pos, nrm, time = hits["p"][ok], hits["n"][ok], rays[ok, 3]
        reps = -(-MIN_POINTS // len(pos))
        pts = gc.points(np.tile(pos, (reps, 1)), np.tile(nrm, (reps, 1)), np.tile(time, reps))
        assert len(pts) >= MIN_POINTS and np.isfinite(pts[:, :7]).all()
        out[name] = (ses, pts)
    assert (out["procedural"][1][:, 3] != out["procedural"][1][0, 3]).any()   # per-point times
    return out


@pytest.fixture(scope="module")
def reference(gpu_lib, cases):
    """values(name, tree, kind, sample_index, skip, max_path) -> the per-point sample value of statement 3, from the NumPy direction (the device's sincos),
    RaylibAMD_TraceRadiance along it (skipDraws + 2, one sample) and the NumPy product.  Computed once per key and shared; the caller must have set
    RAYLIB_QUERY_TREE to `tree`."""
    from raylib_amd import binding
    sincos = gc.device_sincos(gpu_lib)
    seed = gpu_lib.RaylibAMD_GetSeed()
    cache = {}

    def values(name, tree, kind, sample_index, skip, max_path, n=None):
        key = (name, tree, kind, sample_index, skip, max_path, n)
        if key not in cache:
            assert os.environ.get("RAYLIB_QUERY_TREE") == tree
            ses, pts = cases[name]
            pts = pts[:n] if n else pts
            wi = gc.directions(seed, pts, kind, sample_index, skip, sincos)
            L = binding.trace_radiance(gpu_lib, ses.scene, gc.path_rays(pts, wi), max_path=max_path, sample_first=sample_index, sample_count=1, skip_draws=skip + 2)
            cache[key] = (gc.sample_values(L, pts, wi, kind), int(_stats(gpu_lib).rays))
        return cache[key]
    return values


def _lambertian(lib, ses, obj_scene):
    mats = np.zeros(lib.RaylibAMD_SceneNumMaterials(ses.scene), ffi.MAT_DTYPE)
    assert mats.dtype.itemsize == 76
    lib.RaylibAMD_SceneExportMaterials(ses.scene, mats.ctypes.data)
    idx = np.nonzero(mats["type"] == ffi.MAT_LAMBERTIAN)[0]
    assert len(idx)
    if obj_scene:
        assert idx[-1] == len(mats) - 1       # an OBJ scene's last material is the fallback Lambertian
    return int(idx[-1])


@pytest.mark.parametrize("name", SCENES)
def test_directions(gpu_lib, cases, name):
    """Statement 1: the host hook's hemisphere direction is the Lambertian scattering event's, and the NumPy restatement with the device's sincos is the host
    hook's -- so the three agree, and the restatement may stand for the kernel's direction in the tests below."""
    from raylib_amd import binding
    ses, pts = cases[name]
    seed = gpu_lib.RaylibAMD_GetSeed()
    rec = np.zeros((len(pts), 16), F)
    rec[:, 3:6] = (0.0, 0.0, -1.0); rec[:, 7] = 1.0; rec[:, 8:11] = pts[:, 0:3]; rec[:, 11:14] = pts[:, 4:7]
    out = np.zeros((len(pts), 16), F)
    assert gpu_lib.RaylibAMD_EvalScatter(ses.scene, _lambertian(gpu_lib, ses, name != "procedural"), rec.ctypes.data_as(C.POINTER(C.c_float)), len(rec), seed,
                                         out.ctypes.data_as(C.POINTER(C.c_float))) == 1
    assert (out[:, 0] == 1).all() and (out[:, 15] == 2).all()
    hook = binding.gather_directions_host(gpu_lib, pts, gc.IRRADIANCE, seed, 0)
    _same_bits(hook, out[:, 4:7], name + ": the host hook against RaylibAMD_EvalScatter")
    sincos = gc.device_sincos(gpu_lib)
    for kind in KINDS:
        for sample in (0, 1, 5):
            for skip in (0, 2):
                _same_bits(gc.directions(seed, pts, kind, sample, skip, sincos), binding.gather_directions_host(gpu_lib, pts, kind, seed, sample, 0, skip),
                           "%s: NumPy against the host hook, kind %d sample %d skip %d" % (name, kind, sample, skip))


@pytest.mark.parametrize("name", SCENES)
def test_one_sample(gpu_lib, cases, reference, monkeypatch, name):
    """Statements 2 - 4 for one sample: the gather equals RaylibAMD_TraceRadiance along the restated direction, put through the restated product and result."""
    from raylib_amd import binding
    ses, pts = cases[name]
    lit = 0
    for tree in ("2", "4"):
        monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
        for first in (0, 3):
            for skip in (0, 2):
                for max_path in (0, 1, 2, 5):
                    for kind in KINDS:
                        v, _ = reference(name, tree, kind, first, skip, max_path)
                        got = binding.gather(gpu_lib, ses.scene, pts, kind, max_path=max_path, sample_first=first, sample_count=1, skip_draws=skip)
                        _same_bits(got, gc.resolve([v], kind), "%s tree %s kind %d first %d skip %d maxPathLength %d" % (name, tree, kind, first, skip, max_path))
                        if max_path == 0:
                            assert (got[:, :3] == 0).all() if kind == gc.IRRADIANCE else (got == 0).all()
                        if kind == gc.IRRADIANCE:
                            assert (got[:, 3] == 1).all()
                        lit += int((got[:, :3] != 0).any()) if max_path else 0
    assert lit > 0, name     # (the comparison is not one of zeros)


@pytest.mark.parametrize("tree", ["2", "4"])
def test_sample_runs(gpu_lib, cases, reference, monkeypatch, tree):
    """A run of samples is the in-order float sum of its samples' values, times float32(1) / float32(count), times the solid angle."""
    from raylib_amd import binding
    monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
    name = "cornell_glass_sun"
    ses, pts = cases[name]
    for kind in KINDS:
        vs = [reference(name, tree, kind, s, 0, 5)[0] for s in range(65)]
        assert (helpers.bits(vs[0]) != helpers.bits(vs[1])).any()
        for count in (2, 7, 64, 65):
            got = binding.gather(gpu_lib, ses.scene, pts, kind, sample_count=count)
            _same_bits(got, gc.resolve(vs[:count], kind), "kind %d, samples 0..%d" % (kind, count - 1))
        got = binding.gather(gpu_lib, ses.scene, pts, kind, sample_first=3, sample_count=4)
        _same_bits(got, gc.resolve(vs[3:7], kind), "kind %d, samples 3..6" % kind)


@pytest.mark.parametrize("kind", KINDS)
def test_job_space_edges(gpu_lib, cases, reference, monkeypatch, kind):
    """n x sampleCount around the wave and the chunk: the first n points alone give the bits they have inside the whole batch, and one point with a long run of
    samples -- a job space as wide as 4 chunks and a bit, one point deep -- gives the restatement's bits."""
    from raylib_amd import binding
    name = "cornell_glass_sun"
    ses, pts = cases[name]
    for count in (1, 3):
        full = binding.gather(gpu_lib, ses.scene, pts, kind, sample_count=count)
        for n in (1, 63, 64, 65, QUERY_CHUNK - 1, QUERY_CHUNK + 1):
            got = binding.gather(gpu_lib, ses.scene, np.ascontiguousarray(pts[:n]), kind, sample_count=count)
            _same_bits(got, full[:n], "kind %d: the first %d points, %d samples" % (kind, n, count))
        for i in (1, 70, len(pts) - 1):
            got = binding.gather(gpu_lib, ses.scene, np.ascontiguousarray(pts[i:i + 1]), kind, sample_count=count)
            _same_bits(got, full[i:i + 1], "kind %d: point %d alone, %d samples" % (kind, i, count))
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "4")
    long_run = 4 * QUERY_CHUNK + 1
    vs = [reference(name, "4", kind, s, 0, 5, n=1)[0] for s in range(long_run)]
    got = binding.gather(gpu_lib, ses.scene, np.ascontiguousarray(pts[:1]), kind, sample_count=long_run)
    _same_bits(got, gc.resolve(vs, kind), "kind %d: one point, %d samples" % (kind, long_run))
    assert _stats(gpu_lib).cameraSamples == long_run
    # n == 0 is a success that writes nothing
    prm = binding.GatherParams(kind, 5, 1e-4, 0, 1, 0, 0.0, 0.0)
    assert gpu_lib.RaylibAMD_Gather(ses.scene, C.byref(prm), None, 0, None) == 1
    assert len(binding.gather(gpu_lib, ses.scene, np.zeros((0, 8), F), kind)) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_several_launches(gpu_lib, cases, monkeypatch, kind):
    """RAYLIB_GATHER_BATCH cuts a call into launches over sample ranges (37, 64: less than one sample of every point, so over point ranges too; 1000: 10 samples
    of the 100 points) down to one (point, sample) pair per launch; the sums carry between them, and the bits are those of the one launch."""
    from raylib_amd import binding
    ses, pts = cases["cutout_sky"]
    pts = np.ascontiguousarray(pts[:100])
    want = binding.gather(gpu_lib, ses.scene, pts, kind, sample_count=33)
    st = _stats(gpu_lib)
    assert st.traceLaunches == 1 and st.cameraSamples == 100 * 33
    assert (want[:, :3] != 0).any()
    for batch, launches in ((1, 3300), (37, 3 * 33), (64, 2 * 33), (1000, 4)):
        monkeypatch.setenv("RAYLIB_GATHER_BATCH", str(batch))
        got = binding.gather(gpu_lib, ses.scene, pts, kind, sample_count=33)
        st = _stats(gpu_lib)
        _same_bits(got, want, "kind %d, RAYLIB_GATHER_BATCH=%d" % (kind, batch))
        assert st.traceLaunches == launches > 1 and st.cameraSamples == 100 * 33, (batch, st.traceLaunches)


@pytest.mark.parametrize("count", [33, 37, 41])
def test_timing_of_many_launches(gpu_lib, cases, monkeypatch, count):
    """RAYLIB_GATHER_BATCH=1 makes 100 x count launches.  Up to RL_GATHER_TIMED = 4096 of them the trace launches are timed apart: their sum lies below the
    whole call's time, which holds the resolves and the gaps between launches too.  A call of more launches reports the whole span as its trace time."""
    from raylib_amd import binding
    ses, pts = cases["cutout_sky"]
    pts = np.ascontiguousarray(pts[:100])
    want = binding.gather(gpu_lib, ses.scene, pts, gc.IRRADIANCE, sample_count=count)
    assert _stats(gpu_lib).traceLaunches == 1
    monkeypatch.setenv("RAYLIB_GATHER_BATCH", "1")
    got = binding.gather(gpu_lib, ses.scene, pts, gc.IRRADIANCE, sample_count=count)
    st = _stats(gpu_lib)
    print("count %d: traceLaunches %d, traceKernelMs %.6f, kernelMs %.6f, wallMs %.6f" % (count, st.traceLaunches, st.traceKernelMs, st.kernelMs, st.wallMs))
    _same_bits(got, want, "%d samples, one pair per launch" % count)
    assert st.traceLaunches == 100 * count and st.cameraSamples == 100 * count
    if 100 * count <= 4096:
        assert 0 < st.traceKernelMs < st.kernelMs <= st.wallMs
    else:
        assert st.traceKernelMs == st.kernelMs > 0


def test_device_entry(gpu_lib, cases):
    """Torch tensors through the device entry: on a stream of torch's and on torch's default stream they give the host entry's bytes; two calls enqueued on two
    streams give the bytes of the same calls one after the other (the event chain orders them on the shared scratch); misaligned and host pointers are refused
    with nothing written."""
    from raylib_amd import binding
    ses, pts = cases["cornell_glass_sun"]
    n = len(pts)
    dev = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    want = {kind: binding.gather(gpu_lib, ses.scene, pts, kind, sample_count=3) for kind in KINDS}
    want9 = binding.gather(gpu_lib, ses.scene, pts, gc.IRRADIANCE, sample_count=9, max_path=8)
    for kind in KINDS:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got = binding.gather(gpu_lib, ses.scene, dev, kind, sample_count=3)
        s.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, gc.OUT_FLOATS[kind])
        assert got.cpu().numpy().tobytes() == want[kind].tobytes()
        # torch's default stream: synchronous, on the library's stream, with stats
        got = binding.gather(gpu_lib, ses.scene, dev, kind, sample_count=3)
        assert _stats(gpu_lib).cameraSamples == 3 * n
        assert got.cpu().numpy().tobytes() == want[kind].tobytes()
    # two calls enqueued on two streams before either is waited for, a radiance call on a third between them
    rays = gc.path_rays(pts, binding.gather_directions_host(gpu_lib, pts, gc.SH9, 1))
    want_rad = binding.trace_radiance(gpu_lib, ses.scene, rays)
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = binding.gather(gpu_lib, ses.scene, dev, gc.IRRADIANCE, sample_count=9, max_path=8)
    with torch.cuda.stream(s3):
        r = binding.trace_radiance(gpu_lib, ses.scene, torch.from_numpy(rays).cuda())
    with torch.cuda.stream(s2):
        b = binding.gather(gpu_lib, ses.scene, dev, gc.SH9, sample_count=3)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == want9.tobytes() and b.cpu().numpy().tobytes() == want[gc.SH9].tobytes()
    assert r.cpu().numpy().tobytes() == want_rad.tobytes()
    # refusals
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    pt_p = lambda p: C.cast(p, C.POINTER(binding.GatherPoint))
    out_p = lambda p: C.cast(p, C.POINTER(C.c_float))
    out = torch.full((n * 27 + 8,), 7.0, dtype=torch.float32, device="cuda")
    big = torch.zeros(n * 8 + 4, dtype=torch.float32, device="cuda")
    host_out = np.full((n, 27), 7.0, F)
    torch.cuda.synchronize()
    fn = gpu_lib.RaylibAMD_GatherDevice
    irr = binding.GatherParams(gc.IRRADIANCE, 5, 1e-4, 0, 3, 0, 0.0, 1.0)
    sh9 = binding.GatherParams(gc.SH9, 5, 1e-4, 0, 3, 0, 0.0, 1.0)
    assert fn(ses.scene, C.byref(irr), pt_p(ptr(dev)), n, out_p(ptr(out, 4)), None) == 0          # IRRADIANCE results are written as 16-byte stores
    assert fn(ses.scene, C.byref(sh9), pt_p(ptr(dev)), n, out_p(ptr(out, 2)), None) == 0          # SH9 results as 4-byte stores
    for prm in (irr, sh9):
        assert fn(ses.scene, C.byref(prm), pt_p(ptr(big, 8)), n, out_p(ptr(out)), None) == 0      # points are read as 16-byte loads
        assert fn(ses.scene, C.byref(prm), pts.ctypes.data_as(C.POINTER(binding.GatherPoint)), n, out_p(ptr(out)), None) == 0
        assert fn(ses.scene, C.byref(prm), pt_p(ptr(dev)), n, host_out.ctypes.data_as(C.POINTER(C.c_float)), None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all() and (host_out == 7.0).all()
    assert fn(ses.scene, C.byref(sh9), pt_p(ptr(dev)), n, out_p(ptr(out, 4)), None) == 1          # (4-byte aligned is enough for SH9)
    assert out[1:1 + n * 27].cpu().numpy().tobytes() == want[gc.SH9].tobytes()


def test_estimator_closed_form(gpu_lib):
    """A sun of illuminance I straight overhead, no panorama, and one small far sphere that neither a gather ray nor the sun's shadow ray meets: every sample's L
    is the miss shader's I, whatever its direction.  One point at the origin, normal +y, 4096 samples.
    IRRADIANCE is I * 2 pi * mean(cos) with cos uniform on [0, 1]: pi I, relative standard error (1 / sqrt 12) / (1/2 * 64) = 0.9 %; the bound is 5 of them.
    SH9: coefficient 0 is 4 pi * 0.282095 * I up to the rounding of a 4096-term float sum (relative 1e-4); the others integrate to 0, each sample's term is
    at most of the order of I * sqrt(4 pi) * (an orthonormal function's unit RMS), so 5 standard errors are 5 sqrt(4 pi) / 64 * I.
    The bounds are derived, not tuned: they catch a wrong solid angle or basis constant, which the bit tests against the library's own arithmetic cannot."""
    from raylib_amd import binding
    mats = np.zeros(1, ffi.MAT_DTYPE)
    for k in ("texAlbedo", "texNormal", "texRoughness", "texMetallic", "texEmissive"):
        mats[0][k] = -1
    mats[0]["type"] = ffi.MAT_LAMBERTIAN; mats[0]["albedo"] = (0.5, 0.5, 0.5); mats[0]["transmission"] = (1, 1, 1)
    sph = np.zeros(1, ffi.SPHERE_DTYPE)
    sph[0] = ((3000.0, -4000.0, 1000.0), 0.01, 0)
    I = np.array([2.0, 3.0, 0.5], F)
    ses = binding.ProceduralSession(gpu_lib, mats, sph, (), (0, 0, 3), (0, 0, -1), 45.0, 1.0, sun=tuple(I), sun_dir=(0.0, -1.0, 0.0))
    try:
        pts = gc.points([[0.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]], stream=[17])
        count = 4096
        irr = binding.gather(gpu_lib, ses.scene, pts, gc.IRRADIANCE, sample_count=count)[0]
        st = _stats(gpu_lib)
        assert st.cameraSamples == count and st.shadedHits == 0        # every path is a miss
        sh = binding.gather(gpu_lib, ses.scene, pts, gc.SH9, sample_count=count)[0].reshape(9, 3)
    finally:
        ses.close()
    I64 = I.astype(np.float64)
    rel = np.abs(irr[:3] / (np.pi * I64) - 1.0)
    print("IRRADIANCE / (pi I) - 1:", rel, " SH9 j = 0 rel:", np.abs(sh[0] / (12.566371 * 0.282095 * I64) - 1.0), " SH9 j >= 1 / I:", np.abs(sh[1:] / I64).max(0))
    assert (rel <= 5 * (1 / np.sqrt(12)) / (0.5 * 64)).all() and irr[3] == 1.0
    assert (np.abs(sh[0] / (float(F(12.566371)) * float(F(0.282095)) * I64) - 1.0) <= 1e-4).all()
    assert (np.abs(sh[1:]) <= 5 * np.sqrt(4 * np.pi) / 64 * I64).all()
    assert (sh[1:] != 0).all()


def test_stats(gpu_lib, cases, reference, monkeypatch):
    from raylib_amd import binding
    name = "cornell_glass_sun"
    ses, pts = cases[name]
    for tree, width in (("2", 2), ("4", 4)):
        monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
        for kind in KINDS:
            for count in (1, 3):
                binding.gather(gpu_lib, ses.scene, pts, kind, sample_count=count)
                st = _stats(gpu_lib)
                assert st.cameraSamples == len(pts) * count, st.as_dict()
                assert st.rays == sum(reference(name, tree, kind, s, 0, 5)[1] for s in range(count)), st.as_dict()
                assert st.treeWidth == width == binding.plan_radiance(gpu_lib, ses.scene)[1]["treeWidth"] and st.nodeBytes == 64
                assert st.traceLaunches == 1 and st.nodesVisited > 0 and st.trisTested > 0 and st.shadedHits > 0
                assert 0 < st.traceKernelMs <= st.kernelMs <= st.wallMs
