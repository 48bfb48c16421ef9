"""The adaptive gather (RaylibAMD_GatherAdaptive, include/raylib_amd.h statements A1 to A5) without a device: the host oracle RaylibAMD_GatherAdaptiveDecideHost
against the NumPy restatement (tests/gather_adaptive_cases.py) on synthetic keys, every refusal of the adaptive parameters, and the refusals the ABI makes before
it looks for a device."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers  # noqa: F401  (sys.path)
from helpers import scenes
import gather_cases as gc
import gather_adaptive_cases as ga

F = np.float32


def _decide(lib, keys, threshold, min_samples, pass_samples, cap=None):
    from raylib_amd import binding
    return binding.gather_adaptive_decide_host(lib, keys, threshold, min_samples, pass_samples, cap)


def _both(lib, keys, threshold, min_samples, pass_samples):
    got = _decide(lib, keys, threshold, min_samples, pass_samples)
    want = ga.decide(keys, threshold, min_samples, pass_samples)
    assert got is not None
    assert got.dtype == np.uint32 and got.tolist() == want.tolist(), (threshold, min_samples, pass_samples, got.tolist(), want.tolist())
    return got


def _keys(rng, count, cap):
    """keys with a spread of variances: a per-point level times (1 + noise of a per-point width), non-negative"""
    level = (rng.rand(count, 1, 3) * 4).astype(F)
    width = (rng.rand(count, 1, 1) ** 3).astype(F)
    return np.ascontiguousarray(np.abs(level * (1 + width * rng.randn(count, cap, 3))).astype(F))


def test_record_layout_and_exports(lib):
    from raylib_amd import binding
    assert C.sizeof(binding.GatherAdaptiveParams) == 12
    assert [getattr(binding.GatherAdaptiveParams, f).offset for f in ("threshold", "minSamples", "passSamples")] == [0, 4, 8]
    for name in ("RaylibAMD_GatherAdaptive", "RaylibAMD_GatherAdaptiveDevice", "RaylibAMD_GatherAdaptiveDecideHost", "RaylibAMD_GatherCompactTest",
                 "RaylibAMD_BakeLightmapAdaptive", "RaylibAMD_BakeLightmapAdaptiveDevice"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


@pytest.mark.parametrize("cap,pass_samples", [(24, 4), (23, 4), (24, 24), (24, 32), (7, 1), (64, 5)])
def test_oracle_matches_numpy_on_random_keys(lib, cap, pass_samples):
    rng = np.random.RandomState(cap * 97 + pass_samples)
    keys = _keys(rng, 300, cap)
    s1, s2 = ga.moments(keys)
    n8 = min(cap, 8)
    errs = np.sort(ga.error(s1[:, n8 - 1], s2[:, n8 - 1], n8))
    spread = set()
    for threshold in (0.0, float(errs[len(errs) // 4]), float(errs[len(errs) // 2]), float(errs[-1]) * 2, 3e38):
        for min_samples in (2, 4, 9):
            spread |= set(_both(lib, keys, threshold, min_samples, pass_samples).tolist())
    assert cap in spread and (len(ga.pass_counts(cap, pass_samples)) == 1 or len(spread) >= 2), spread


def test_oracle_edges(lib):
    cap = 24
    const = np.tile(np.array([0.3, 0.5, 0.2], F), (5, cap, 1))
    # constant keys: the error is 0 up to the rounding of S2 - S1 * S1 / n, which max(0, .) and the restatement share; stop at the first n_p >= minSamples
    for min_samples, n in ((2, 4), (4, 4), (5, 8), (9, 12), (24, 24)):
        assert _both(lib, const, 1e-3, min_samples, 4).tolist() == [n] * 5
    # all-zero keys: y = 0 / 1 = 0, error exactly 0
    zero = np.zeros((3, cap, 3), F)
    assert _both(lib, zero, 1e-30, 4, 4).tolist() == [4] * 3
    assert _both(lib, zero, 0.0, 4, 4).tolist() == [cap] * 3          # threshold 0: never early (0 < 0 is false)
    # alternating keys: y alternates between 0 and 0.5, standard error sqrt(0.0625 n / (n - 1) / n) >= 0.05 for n <= 24: never below 0.05
    alt = np.zeros((2, cap, 3), F)
    alt[:, 1::2] = 1.0                                                   # lum = 0.2126 + 0.7152 + 0.0722 = 1 (to rounding), y = 0.5
    assert _both(lib, alt, 0.05, 4, 4).tolist() == [cap] * 2
    assert _both(lib, alt, 0.2, 4, 4).tolist() == [4] * 2              # (and it does stop once the threshold is above: se(4) = sqrt(1/12 / 4) = 0.144)
    # a key that is not finite at sample 0: S1 is not finite ever after, the error +inf, n = cap whatever the threshold
    for badv in (np.inf, -np.inf, np.nan):
        k = const.copy()
        k[1, 0, 1] = badv
        got = _both(lib, k, 3e38, 2, 4)
        assert got.tolist() == [4, cap, 4, 4, 4], (badv, got)
    # lum = -1: y = -1 / 0 = -inf
    k = const.copy(); k[2, 0] = (0.0, F(-1) / F(0.7152), 0.0)
    _both(lib, k, 3e38, 2, 4)
    # minSamples above the cap: n = cap; cap not a multiple of passSamples: the last pass is short; passSamples >= cap: one pass
    assert _both(lib, const, 1.0, 25, 4).tolist() == [cap] * 5
    assert _both(lib, const[:, :23], 1.0, 21, 4).tolist() == [23] * 5
    assert _both(lib, const[:, :23], 1.0, 20, 4).tolist() == [20] * 5
    assert _both(lib, const, 1.0, 2, 24).tolist() == [cap] * 5
    assert _both(lib, const, 1.0, 2, 32).tolist() == [cap] * 5
    assert _both(lib, const, 1.0, 2, 0xffffffff).tolist() == [cap] * 5
    # the threshold is strict: y = 0, 0, 0, about 1/2 -> an error e of about 1/8 after 4 samples; a threshold of e does not stop the point, the next float does
    k = np.zeros((1, 4, 3), F); k[0, 3] = (0.0, F(1) / F(0.7152), 0.0)
    e = ga.error(*[m[:, 3] for m in ga.moments(k)], 4)[0]
    assert abs(float(e) - 0.125) < 1e-6
    assert _both(lib, np.concatenate([k, k], 1), float(e), 4, 4).tolist() == [8]
    assert _both(lib, np.concatenate([k, k], 1), float(np.nextafter(e, F(1))), 4, 4).tolist() == [4]
    # no points
    assert _decide(lib, np.zeros((0, cap, 3), F), 0.1, 4, 4).tolist() == []


def test_oracle_refusals(lib):
    from raylib_amd import binding
    fn = lib.RaylibAMD_GatherAdaptiveDecideHost
    keys = np.zeros((2, 24, 3), F)
    out = np.full(2, 7, np.uint32)
    kp, op = keys.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_uint32))
    A = lambda t=0.1, m=4, p=4: C.byref(binding.GatherAdaptiveParams(t, m, p))
    assert fn(A(), 24, kp, 2, op) == 1 and out.tolist() == [4, 4]
    out[:] = 7
    assert fn(None, 24, kp, 2, op) == 0
    assert fn(A(), 24, None, 2, op) == 0
    assert fn(A(), 24, kp, 2, None) == 0
    assert fn(A(), 24, kp, -1, op) == 0
    assert fn(A(), 0, kp, 2, op) == 0
    for t in (-1e-6, float("nan"), float("inf"), float("-inf")):
        assert fn(A(t=t), 24, kp, 2, op) == 0, t
    assert fn(A(m=1), 24, kp, 2, op) == 0 and fn(A(m=0), 24, kp, 2, op) == 0
    assert fn(A(p=0), 24, kp, 2, op) == 0
    assert fn(A(p=1), 4097, kp, 0, op) == 0                  # 4097 passes
    assert fn(A(p=1), 4096, None, 0, None) == 1              # 4096 passes, no points
    assert fn(A(p=2), 8192, None, 0, None) == 1 and fn(A(p=2), 8193, None, 0, None) == 0
    assert out.tolist() == [7, 7]


@pytest.fixture(scope="module")
def cornell(lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "gather_adaptive_host"); os.makedirs(d, exist_ok=True)
    ses = binding.SceneSession(lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    yield ses
    ses.close()


def test_abi_refusals_that_need_no_device(lib, cornell):
    """Everything RaylibAMD_Gather refuses and every refusal of the adaptive parameters returns 0 with nothing written, before the call looks for a device; no points
    are a success without one."""
    from raylib_amd import binding
    ses = cornell
    pts = gc.points(np.tile([[0.0, 1.0, 0.0]], (4, 1)), np.tile([[0.0, 1.0, 0.0]], (4, 1)))
    pp = pts.ctypes.data_as(C.POINTER(binding.GatherPoint))
    out = np.full((4, 27), 7.0, F)
    cnt = np.full(4, 7, np.uint32)
    op, cp = out.ctypes.data_as(C.POINTER(C.c_float)), cnt.ctypes.data_as(C.POINTER(C.c_uint32))
    good = dict(kind=0, maxPathLength=5, rayTMin=1e-4, sampleFirst=0, sampleCount=24, skipDraws=0, timeMin=0.0, timeMax=0.0)
    prm = lambda **kw: C.byref(binding.GatherParams(**dict(good, **kw)))
    A = lambda t=0.1, m=4, p=4: C.byref(binding.GatherAdaptiveParams(t, m, p))
    bad_gather = [dict(kind=2), dict(kind=-1), dict(skipDraws=63), dict(sampleCount=0), dict(rayTMin=-1e-4), dict(rayTMin=float("nan")), dict(maxPathLength=-1),
                  dict(maxPathLength=32769)]
    bad_adaptive = [dict(t=-1.0), dict(t=float("nan")), dict(t=float("inf")), dict(m=1), dict(m=0), dict(p=0)]
    unfinished = lib.Raylib_CreateScene()
    for fn, extra in ((lib.RaylibAMD_GatherAdaptive, ()), (lib.RaylibAMD_GatherAdaptiveDevice, (None,))):
        assert fn(ses.scene, prm(), A(), None, 4, op, cp, *extra) == 0
        assert fn(ses.scene, prm(), A(), pp, 4, None, cp, *extra) == 0
        assert fn(ses.scene, prm(), A(), pp, -1, op, cp, *extra) == 0
        assert fn(ses.scene, None, A(), pp, 4, op, cp, *extra) == 0
        assert fn(ses.scene, prm(), None, pp, 4, op, cp, *extra) == 0
        assert fn(None, prm(), A(), pp, 4, op, cp, *extra) == 0
        assert fn(unfinished, prm(), A(), pp, 4, op, cp, *extra) == 0
        for b in bad_gather:
            assert fn(ses.scene, prm(**b), A(), pp, 4, op, cp, *extra) == 0, b
        for b in bad_adaptive:
            assert fn(ses.scene, prm(), A(**b), pp, 4, op, cp, *extra) == 0, b
            assert fn(ses.scene, prm(), A(**b), None, 0, None, None, *extra) == 0, b      # ... with no points too
        assert fn(ses.scene, prm(sampleCount=4097), A(p=1), pp, 4, op, cp, *extra) == 0    # more than 4096 passes
    p = pts.copy(); p[2, 3] = float("nan")                        # the host entry: a point's time that is not finite
    assert lib.RaylibAMD_GatherAdaptive(ses.scene, prm(), A(), p.ctypes.data_as(C.POINTER(binding.GatherPoint)), 4, op, cp) == 0
    assert lib.RaylibAMD_GatherAdaptiveDevice(ses.scene, prm(timeMin=1.0, timeMax=0.0), A(), pp, 4, op, cp, None) == 0
    lib.Raylib_DestroyScene(unfinished)
    assert (out == 7.0).all() and (cnt == 7).all()
    # n == 0: 1, with or without a device, nothing touched
    assert lib.RaylibAMD_GatherAdaptive(ses.scene, prm(), A(), None, 0, None, None) == 1
    v, n = binding.gather_adaptive(lib, ses.scene, np.zeros((0, 8), F), gc.IRRADIANCE, 0.1, sample_count=24)
    assert v.shape == (0, 4) and n.shape == (0,)
    # the bake: the adaptive refusals beside the bake's own
    lp = binding.lightmap_params(8, 8, sample_count=24)
    atlas = np.full((8, 8, 4), 7.0, F)
    ap = atlas.ctypes.data_as(C.POINTER(C.c_float))
    for fn, extra in ((lib.RaylibAMD_BakeLightmapAdaptive, ()), (lib.RaylibAMD_BakeLightmapAdaptiveDevice, (None,))):
        assert fn(ses.scene, C.byref(lp), None, None, ap, None, None, *extra) == 0
        assert fn(ses.scene, C.byref(lp), A(), None, None, None, None, *extra) == 0
        assert fn(ses.scene, None, A(), None, ap, None, None, *extra) == 0
        for b in bad_adaptive:
            assert fn(ses.scene, C.byref(lp), A(**b), None, ap, None, None, *extra) == 0, b
        assert fn(ses.scene, C.byref(binding.lightmap_params(8, 8, sample_count=4097)), A(p=1), None, ap, None, None, *extra) == 0
        assert fn(ses.scene, C.byref(binding.lightmap_params(0, 8, sample_count=24)), A(), None, ap, None, None, *extra) == 0
    assert (atlas == 7.0).all()
    # the compaction hook's argument refusals need no device either
    hook = lib.RaylibAMD_GatherCompactTest
    u32 = C.POINTER(C.c_uint32)
    live = np.array([0, 2, 3], np.uint32); stopped = np.zeros(4, np.uint8)
    ol = np.full(3, 7, np.uint32); opnt = np.full((3, 8), 7.0, F); oc = np.full(1, 7, np.uint32)
    base = dict(live=live.ctypes.data_as(u32), n=3, stopped=stopped.ctypes.data_as(C.POINTER(C.c_uint8)), pts=pp, np_=4, ol=ol.ctypes.data_as(u32),
                op=opnt.ctypes.data_as(C.POINTER(binding.GatherPoint)), oc=oc.ctypes.data_as(u32))
    args = lambda **kw: [dict(base, **kw)[k] for k in ("live", "n", "stopped", "pts", "np_", "ol", "op", "oc")]
    for k in ("live", "stopped", "pts", "ol", "op", "oc"):
        assert hook(*args(**{k: None})) == 0, k
    assert hook(*args(n=5)) == 0 and hook(*args(np_=3)) == 0         # more live entries than points; an entry >= numPoints
    for bad_live in ([0, 2, 2], [2, 0, 3], [0, 1, 4]):
        b = np.array(bad_live, np.uint32)
        assert hook(*args(live=b.ctypes.data_as(u32))) == 0, bad_live
    assert (ol == 7).all() and (opnt == 7.0).all() and oc[0] == 7
