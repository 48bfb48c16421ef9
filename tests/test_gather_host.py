"""Irradiance and SH probes gathered at caller points (RaylibAMD_Gather, include/raylib_amd.h) without a device: the record layouts, every refusal that needs
no device, and the host hook RaylibAMD_GatherDirectionsHost against the NumPy restatement of the stream (tests/gather_cases.py) in everything that does not
pass through sin and cos: the third component's sign, the hemisphere rule, the unit length, and the sphere's direction being the hemisphere's or its exact
negation."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from helpers import scenes
import gather_cases as gc

F = np.float32


@pytest.fixture(scope="module")
def cornell(lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "gather_host"); os.makedirs(d, exist_ok=True)
    ses = binding.SceneSession(lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    yield ses
    ses.close()


def _points(n=4):
    return gc.points(np.tile([[0.0, 1.0, 0.0]], (n, 1)), np.tile([[0.0, 1.0, 0.0]], (n, 1)))


def test_record_layouts(lib):
    from raylib_amd import binding
    assert C.sizeof(binding.GatherPoint) == 32 and C.sizeof(binding.GatherParams) == 32
    assert [getattr(binding.GatherPoint, f).offset for f in ("pos", "time", "normal", "stream")] == [0, 12, 16, 28]
    assert [getattr(binding.GatherParams, f).offset for f in ("kind", "maxPathLength", "rayTMin", "sampleFirst", "sampleCount", "skipDraws", "timeMin", "timeMax")] == \
        [0, 4, 8, 12, 16, 20, 24, 28]
    for name in ("RaylibAMD_Gather", "RaylibAMD_GatherDevice", "RaylibAMD_GatherDirectionsHost", "RaylibAMD_PlanGatherCut"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)
    assert (binding.GATHER_IRRADIANCE, binding.GATHER_SH9) == (gc.IRRADIANCE, gc.SH9) == (0, 1)


def test_refusals_that_need_no_device(lib, cornell):
    """Every refusal of include/raylib_amd.h returns 0 and writes nothing -- before the call looks for a device."""
    from raylib_amd import binding
    ses = cornell
    pts = _points()
    pp = pts.ctypes.data_as(C.POINTER(binding.GatherPoint))
    out = np.full((4, 27), 7.0, F)
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    good = dict(kind=0, maxPathLength=5, rayTMin=1e-4, sampleFirst=0, sampleCount=1, skipDraws=0, timeMin=0.0, timeMax=0.0)
    prm = lambda **kw: binding.GatherParams(**dict(good, **kw))
    bad = [dict(kind=2), dict(kind=-1), dict(skipDraws=63), dict(skipDraws=65), dict(sampleCount=0), dict(rayTMin=-1e-4), dict(rayTMin=float("nan")),
           dict(rayTMin=float("inf")), dict(maxPathLength=-1), dict(maxPathLength=32769)]
    unfinished = lib.Raylib_CreateScene()
    for fn, extra in ((lib.RaylibAMD_Gather, ()), (lib.RaylibAMD_GatherDevice, (None,))):
        g = prm()
        assert fn(ses.scene, C.byref(g), None, 4, op, *extra) == 0
        assert fn(ses.scene, C.byref(g), pp, 4, None, *extra) == 0
        assert fn(ses.scene, C.byref(g), pp, -1, op, *extra) == 0
        assert fn(ses.scene, None, pp, 4, op, *extra) == 0
        assert fn(None, C.byref(g), pp, 4, op, *extra) == 0
        assert fn(unfinished, C.byref(g), pp, 4, op, *extra) == 0
        for b in bad:
            for kind in ([0, 1] if "kind" not in b else [b["kind"]]):
                q = prm(**dict(b, kind=kind))
                assert fn(ses.scene, C.byref(q), pp, 4, op, *extra) == 0, b
    for t in (float("nan"), float("inf")):                      # the host entry: a point's time that is not finite
        p = pts.copy(); p[2, 3] = t
        assert lib.RaylibAMD_Gather(ses.scene, C.byref(prm()), p.ctypes.data_as(C.POINTER(binding.GatherPoint)), 4, op) == 0
    for lo, hi in ((1.0, 0.0), (float("nan"), 0.0), (0.0, float("inf"))):   # the device entry: its time interval
        assert lib.RaylibAMD_GatherDevice(ses.scene, C.byref(prm(timeMin=lo, timeMax=hi)), pp, 4, op, None) == 0
    lib.Raylib_DestroyScene(unfinished)
    # the host hook: null arguments, the kind, the draws
    dirs = np.full((4, 3), 7.0, F)
    dp = dirs.ctypes.data_as(C.POINTER(C.c_float))
    hook = lib.RaylibAMD_GatherDirectionsHost
    assert hook(None, pp, 4, 1, 0, dp) == 0
    assert hook(C.byref(prm()), None, 4, 1, 0, dp) == 0
    assert hook(C.byref(prm()), pp, 4, 1, 0, None) == 0
    assert hook(C.byref(prm()), pp, -1, 1, 0, dp) == 0
    assert hook(C.byref(prm(kind=2)), pp, 4, 1, 0, dp) == 0
    assert hook(C.byref(prm(skipDraws=63)), pp, 4, 1, 0, dp) == 0
    assert (out == 7.0).all() and (dirs == 7.0).all()
    with pytest.raises(ValueError):
        binding.gather(lib, ses.scene, pts, 2)


def test_no_points_is_a_success_that_writes_nothing(lib, cornell):
    from raylib_amd import binding
    for kind in (0, 1):
        g = binding.GatherParams(kind, 5, 1e-4, 0, 1, 0, 0.0, 0.0)
        assert lib.RaylibAMD_GatherDirectionsHost(C.byref(g), None, 0, 1, 0, None) == 1
        assert binding.gather_directions_host(lib, np.zeros((0, 8), F), kind, 1).shape == (0, 3)
        assert lib.RaylibAMD_Gather(cornell.scene, C.byref(g), None, 0, None) == 1
        assert lib.RaylibAMD_GatherDevice(cornell.scene, C.byref(g), None, 0, None, None) == 1
        assert binding.gather(lib, cornell.scene, np.zeros((0, 8), F), kind).shape == (0, gc.OUT_FLOATS[kind])


def _ulp_distance_from_one(x):
    """|x - 1| in ulps of 1.0f (np.spacing(float32(1)) = 2^-23).  The length is off by the roundings of the length's square root, of its reciprocal and of
    one product per component, each at most 2^-24 relative: under 2 ulp."""
    return np.abs(x.astype(np.float64) - 1.0) / float(np.spacing(F(1)))


@pytest.mark.parametrize("skip", [0, 3])
def test_directions_host(lib, skip):
    from raylib_amd import binding
    n, seed = 256, 12345
    rng = np.random.RandomState(7)
    normals = rng.normal(size=(n, 3)).astype(F)
    normals[:64] = (0.0, 0.0, 1.0)
    pts = gc.points(rng.uniform(-1, 1, (n, 3)), normals, stream=rng.randint(0, 2 ** 31, n))
    for sample in (0, 1, 7):
        for sample_first in (0, 5):
            hemi = binding.gather_directions_host(lib, pts, gc.IRRADIANCE, seed, sample, sample_first, skip)
            sph = binding.gather_directions_host(lib, pts, gc.SH9, seed, sample, sample_first, skip)
            u1, _ = gc.first_draws(seed, pts, sample_first + sample, skip)
            z = (F(1) - (F(2) * u1).astype(F)).astype(F)
            # the sphere's third component carries the sign of z = 1 - 2 u1 (normalising multiplies by a positive number), and vanishes with it
            assert (np.sign(sph[:, 2]) == np.sign(z)).all()
            assert (z != 0).sum() > n // 2
            # the hemisphere rule, in the kernel's own arithmetic: dot(N, Wi) >= 0
            assert (gc.dot3(pts[:, 4:7], hemi) >= 0).all()
            # unit length within 2 ulp
            for d in (hemi, sph):
                assert d.dtype == np.float32 and np.isfinite(d).all()
                assert (_ulp_distance_from_one(np.sqrt((d.astype(np.float64) ** 2).sum(1))) <= 2.0).all()
            # the hemisphere's direction is the sphere's, or its exact negation
            same = (helpers.bits(hemi) == helpers.bits(sph)).all(1)
            neg = (helpers.bits(hemi) == helpers.bits(-sph)).all(1)
            assert (same | neg).all() and neg.any() and same.any()
            # ... negated exactly when dot(w, N) < 0: with N = (0, 0, 1) that is z < 0, which is u1 > 0.5
            assert (neg[:64] == (u1[:64] > F(0.5))).all()
            # another sample, another direction
            other = binding.gather_directions_host(lib, pts, gc.SH9, seed, sample + 1, sample_first, skip)
            assert (helpers.bits(other) != helpers.bits(sph)).any(1).all()
    # the stream's key is sampleFirst + sample
    a = binding.gather_directions_host(lib, pts, gc.SH9, seed, 2, 5, skip)
    b = binding.gather_directions_host(lib, pts, gc.SH9, seed, 7, 0, skip)
    assert a.tobytes() == b.tobytes()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-device path: this machine may have a GPU")
def test_gather_without_a_device_returns_0(lib, cornell):
    from raylib_amd import binding
    pts = _points()
    out = np.full((4, 27), 7.0, F)
    g = binding.GatherParams(0, 5, 1e-4, 0, 1, 0, 0.0, 0.0)
    pp, op = pts.ctypes.data_as(C.POINTER(binding.GatherPoint)), out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.RaylibAMD_Gather(cornell.scene, C.byref(g), pp, 4, op) == 0
    assert lib.RaylibAMD_GatherDevice(cornell.scene, C.byref(g), pp, 4, op, None) == 0
    assert (out == 7.0).all()
    with pytest.raises(RuntimeError):
        binding.gather(lib, cornell.scene, pts, 0)


def _walk(lib, kind, n, count, ks):
    from raylib_amd import binding
    return [binding.plan_gather_cut(lib, kind, n, count, k) for k in ks]


@pytest.mark.parametrize("kind", [0, 1])
def test_the_cut_into_launches_at_the_ends_of_32_bits(lib, monkeypatch, kind):
    """RaylibAMD_PlanGatherCut is the arithmetic DeviceGather's launch loop runs on (csrc/rl_plan.cc).  sampleCount has no upper bound below 2^32 and n none below
    2^31: the launches must cover every (point, sample) pair exactly once, in order, and END -- no range's successor may wrap to 0."""
    from raylib_amd import binding
    monkeypatch.delenv("RAYLIB_GATHER_BATCH", raising=False)
    slots = (256 << 20) // (16 if kind == 0 else 32)
    top = 2 ** 32 - 1
    # one point, every sampleCount about a multiple of the launch's samples and at the top of the range
    for count in (1, slots - 1, slots, slots + 1, 0xFF000000, 0xFF000001, top - slots, top - 1, top):
        c = binding.plan_gather_cut(lib, kind, 1, count)
        ranges = -(-count // slots)
        assert (c["pointsPerLaunch"], c["samplesPerLaunch"], c["pointRanges"], c["sampleRanges"], c["launches"]) == (1, min(count, slots), 1, ranges, ranges), (count, c)
        assert (c["pointFirst"], c["numPoints"], c["sampleBase"], c["first"]) == (0, 1, 0, 1)
        last = binding.plan_gather_cut(lib, kind, 1, count, ranges - 1)
        assert last["last"] == 1 and last["sampleBase"] == (ranges - 1) * slots and last["sampleBase"] + last["numSamples"] == count, (count, last)
        assert binding.plan_gather_cut(lib, kind, 1, count, ranges) is None          # the loop's bound: there is no launch behind the last
        if ranges > 2:
            mid = binding.plan_gather_cut(lib, kind, 1, count, ranges - 2)
            assert (mid["first"], mid["last"], mid["numSamples"], mid["sampleBase"]) == (0, 0, slots, (ranges - 2) * slots)
    # every launch of a call, walked: contiguous, in order, complete
    for n, count, batch in ((1, top, 2 ** 28), (3, top, 2 ** 28), (100, 33, 37), (100, 33, 1000), (100, 33, 1), (2 ** 31 - 1, 3, None), (2 ** 31 - 1, top, None)):
        if batch is None:
            monkeypatch.delenv("RAYLIB_GATHER_BATCH", raising=False)
        else:
            monkeypatch.setenv("RAYLIB_GATHER_BATCH", str(batch))
        c = binding.plan_gather_cut(lib, kind, n, count)
        assert c["pointsPerLaunch"] * c["samplesPerLaunch"] <= (batch or slots) and c["launches"] == c["pointRanges"] * c["sampleRanges"]
        assert c["pointRanges"] == -(-n // c["pointsPerLaunch"]) and c["sampleRanges"] == -(-count // c["samplesPerLaunch"])
        assert c["samplesPerLaunch"] == 1 or c["pointsPerLaunch"] == n                # sample ranges of all the points, or point ranges of one sample
        total = c["launches"]
        ks = range(total) if total <= 4000 else list(range(40)) + list(range(total - 40, total)) + [c["sampleRanges"] - 1, c["sampleRanges"], total // 2]
        for k in ks:
            L = binding.plan_gather_cut(lib, kind, n, count, k)
            pr, sr = divmod(k, c["sampleRanges"])
            assert L["pointFirst"] == pr * c["pointsPerLaunch"] and L["numPoints"] == min(c["pointsPerLaunch"], n - L["pointFirst"]) >= 1, (n, count, k, L)
            assert L["sampleBase"] == sr * c["samplesPerLaunch"] and L["numSamples"] == min(c["samplesPerLaunch"], count - L["sampleBase"]) >= 1, (n, count, k, L)
            assert L["first"] == int(sr == 0) and L["last"] == int(sr == c["sampleRanges"] - 1)
            assert L["numPoints"] * L["numSamples"] <= 2 ** 28
        assert binding.plan_gather_cut(lib, kind, n, count, total) is None
    # refusals
    monkeypatch.delenv("RAYLIB_GATHER_BATCH", raising=False)
    g = binding.GatherParams(kind, 5, 1e-4, 0, 8, 0, 0.0, 0.0)
    c = binding.GatherCut()
    assert lib.RaylibAMD_PlanGatherCut(None, 4, 0, C.byref(c)) == 0 and lib.RaylibAMD_PlanGatherCut(C.byref(g), 4, 0, None) == 0
    assert lib.RaylibAMD_PlanGatherCut(C.byref(g), 0, 0, C.byref(c)) == 0 and lib.RaylibAMD_PlanGatherCut(C.byref(g), -1, 0, C.byref(c)) == 0
    assert binding.plan_gather_cut(lib, kind, 4, 0) is None and binding.plan_gather_cut(lib, 2, 4, 8) is None
    assert C.sizeof(binding.GatherCut) == 56
