"""The variance-guided filter where no device is needed (include/raylib_amd.h, statements S1 to S7): the two host oracles, RaylibAMD_TemporalAccumulateMomentsHost
and RaylibAMD_FilterVarianceHost, against float32 restatements byte for byte (tests/variance_cases.py), the properties the statements promise, and every refusal
that is made before the device is asked for.  A missing export fails these tests (the binding raises on load)."""
import ctypes as C

import numpy as np
import pytest

import helpers
import temporal_cases as tc
import variance_cases as vc
from raylib_amd import binding

F = np.float32
W, H = vc.W, vc.H


def _same(got, want, what, names=("outColour", "outVariance")):
    for g, w_, n in zip(got, want, names):
        assert g.tobytes() == w_.tobytes(), "%s: %s differs in %d values" % (what, n, (helpers.bits(g) != helpers.bits(w_)).sum())


@pytest.fixture(scope="module")
def crafted():
    return vc.crafted_filter()


# ---- the restatement ----
@pytest.mark.parametrize("k", [3, 6])
def test_filter_host_is_the_restatement(lib, crafted, k):
    """Byte for byte on the crafted planes at K = 3, with every wanted branch reached; and at K = 6, where only the centre tap is left at the largest step."""
    census = {}
    prm = dict(iterations=k, history_length=2.5)
    want = vc.filter_f32(*crafted, params=prm, census=census)
    wanted = vc.WANTED_BRANCHES + (vc.WANTED_AT_K6 if k == 6 else ())
    missing = [b for b in wanted if not census.get(b)]
    assert not missing, "the crafted planes do not reach: %s (reached: %s)" % (missing, census)
    got = binding.filter_variance(lib, *crafted, params=prm, host=True)
    _same(got, want, "crafted planes, K = %d" % k)
    assert (got[0][..., 3] == 1).all() and (got[1] >= 0).all() and np.isfinite(got[0]).all()


def test_defaults_are_the_null_params(lib, crafted):
    a = binding.filter_variance(lib, *crafted, params=None, host=True)
    b = binding.filter_variance(lib, *crafted, params=dict(vc.DEFAULTS), host=True)
    _same(a, b, "NULL params against 5, 4, 0.35, 0.1, 4")


def test_moments_host_is_the_restatement(lib):
    colour, hit, motion, history = vc.moments_history()
    want = vc.accumulate_moments_f32(colour, hit, motion, history, tc.TOL, tc.CAP)
    got = binding.temporal_accumulate_moments(lib, colour, hit, motion, history, tc.TOL, tc.CAP, host=True)
    _same(got, want, "crafted planes", ("outColour", "outLength", "outMoments"))
    first = binding.temporal_accumulate_moments(lib, colour, hit, motion, None, tc.TOL, tc.CAP, host=True)
    _same(first, vc.accumulate_moments_f32(colour, hit, motion, None, tc.TOL, tc.CAP), "no history", ("outColour", "outLength", "outMoments"))


# ---- S2 ----
def test_colour_and_length_are_the_plain_accumulations(lib):
    colour, hit, motion, history = vc.moments_history()
    for hist in (history, None):
        got = binding.temporal_accumulate_moments(lib, colour, hit, motion, hist, tc.TOL, tc.CAP, host=True)
        want = binding.temporal_accumulate(lib, colour, hit, motion, None if hist is None else hist[:3], tc.TOL, tc.CAP, host=True)
        _same(got[:2], want, "history" if hist else "no history", ("outColour", "outLength"))


# ---- the running mean ----
def test_four_frames_of_identity_motion_are_the_running_moments(lib):
    rng = np.random.RandomState(11)
    ys, xs = np.mgrid[0:H, 0:W]
    hit = np.zeros((H, W), binding.HITT_DTYPE); hit["t"] = 1.5; hit["prim"] = (xs + ys) % 3 - 1          # surfaces and sky
    motion = np.zeros((H, W), binding.MOTION_DTYPE)
    motion["prevX"], motion["prevY"] = xs, ys
    motion["prevT"] = np.where(hit["prim"] >= 0, 1.5, 0); motion["status"] = np.where(hit["prim"] >= 0, binding.MOTION_SURFACE, binding.MOTION_SKY)
    lum = np.vectorize(vc.luminance, otypes=[F])
    history, mean = None, None
    for k in range(1, 5):
        frame = rng.uniform(0, 8, (H, W, 4)).astype(F); frame[..., 3] = 1
        out_c, out_l, out_m = binding.temporal_accumulate_moments(lib, frame, hit, motion, history, 0.0, 32, host=True)
        y = lum(frame[..., 0], frame[..., 1], frame[..., 2])
        m = np.stack([y, (y * y).astype(F)], -1)
        mean = m.copy() if mean is None else (mean + (m - mean) / F(k)).astype(F)      # the incremental means of Y and Y^2, in float32
        assert helpers.bits(out_m).tobytes() == helpers.bits(mean).tobytes(), "frame %d" % k
        assert (out_l == k).all()
        history = (out_c, hit, out_l, out_m)


# ---- the properties ----
def test_no_bleed_across_perpendicular_surfaces(lib):
    """sigmaNormal 0.1: a tap on the other surface has dn = 2 / 0.01 = 200 and expf(-200) == 0, so each side filters only itself: the 0 side stays exactly 0, and on
    the 1 side sum(w * 1) and sum(w) are the same floats, so the quotient is exactly 1."""
    assert vc._expf(F(-200)) == 0
    colour, moments, length, hit, surface, left = vc.no_bleed_planes()
    for k in (1, 5):
        out, var = binding.filter_variance(lib, colour, moments, length, hit, surface, params=dict(iterations=k, sigma_normal=0.1), host=True)
        assert (helpers.bits(out[left][:, :3]) == 0).all(), "the 0 side is +0 after %d iterations" % k
        assert (out[~left][:, :3] == 1).all(), "the 1 side is 1 after %d iterations" % k
        assert (out[..., 3] == 1).all() and (helpers.bits(var) == 0).all()


def test_sky_passes_through(lib, crafted):
    colour, moments, length, hit, surface = crafted
    out, var = binding.filter_variance(lib, *crafted, host=True)
    sky = hit["prim"] == -1
    assert sky.sum() > 20 and (~sky).sum() > 20
    want = np.where(np.isfinite(colour), colour, F(0))
    assert helpers.bits(out[sky][:, :3]).tobytes() == helpers.bits(want[sky][:, :3]).tobytes() and (out[sky][:, 3] == 1).all()
    assert (helpers.bits(var[sky]) == 0).all(), "a sky pixel's variance is +0"
    # a frame of sky alone
    allsky = hit.copy(); allsky["prim"] = -1
    out, var = binding.filter_variance(lib, colour, moments, length, allsky, surface, host=True)
    assert helpers.bits(out[..., :3]).tobytes() == helpers.bits(want[..., :3]).tobytes() and (helpers.bits(var) == 0).all()


def test_colour_does_not_depend_on_the_variance_plane(lib, crafted):
    with_v = binding.filter_variance(lib, *crafted, variance=True, host=True)
    without = binding.filter_variance(lib, *crafted, variance=False, host=True)
    assert without[1] is None and with_v[0].tobytes() == without[0].tobytes()


def test_one_pixel_frame(lib):
    one = lambda a: np.ascontiguousarray(a[:1, :1])
    colour, moments, length, hit, surface = (one(a) for a in vc.crafted_filter())
    hit["prim"] = 5
    for ln in (0, 8):
        length[...] = ln
        _same(binding.filter_variance(lib, colour, moments, length, hit, surface, params=dict(iterations=6), host=True),
              vc.filter_f32(colour, moments, length, hit, surface, params=dict(iterations=6)), "1 x 1, length %d" % ln)


# ---- the refusals ----
def test_filter_refusals_write_nothing(lib, crafted):
    colour, moments, length, hit, surface = crafted
    out_c, out_v = np.full((H, W, 4), 7, F), np.full((H, W), 7, F)
    ptr = dict(colour=colour.ctypes.data, moments=moments.ctypes.data, length=length.ctypes.data, hit=hit.ctypes.data, surface=surface.ctypes.data)
    planes = lambda **kw: C.byref(binding.VarianceFilterPlanes(**dict(ptr, **kw)))
    P = lambda k=5, sl=4.0, sn=0.35, sp=0.1, hl=4.0: C.byref(binding.VarianceFilterParams(k, sl, sn, sp, hl))
    oc, ov = out_c.ctypes.data, out_v.ctypes.data
    cases = {"null planes": (W, H, P(), None, oc, ov), "null outColour": (W, H, P(), planes(), None, ov),
             "W = 0": (0, H, P(), planes(), oc, ov), "H = 0": (W, 0, P(), planes(), oc, ov), "W * H = 2^31": (1 << 16, 1 << 15, P(), planes(), oc, ov),
             "0 iterations": (W, H, P(k=0), planes(), oc, ov), "7 iterations": (W, H, P(k=7), planes(), oc, ov),
             "historyLength < 1": (W, H, P(hl=0.5), planes(), oc, ov), "historyLength NaN": (W, H, P(hl=float("nan")), planes(), oc, ov),
             "historyLength inf": (W, H, P(hl=float("inf")), planes(), oc, ov),
             "outColour is colour": (W, H, P(), planes(colour=oc), oc, ov)}
    for k in ptr:
        cases["null " + k] = (W, H, P(), planes(**{k: None}), oc, ov)
    for name in ("sl", "sn", "sp"):
        for what, v in (("below 1e-3", 5e-4), ("above 1e3", 2e3), ("NaN", float("nan")), ("inf", float("inf")), ("negative", -1.0)):
            cases["%s %s" % (name, what)] = (W, H, P(**{name: v}), planes(), oc, ov)
    for what, args in cases.items():
        assert lib.RaylibAMD_FilterVarianceHost(*args) == 0, what
        assert lib.RaylibAMD_FilterVariance(*args) == 0, what
        assert lib.RaylibAMD_FilterVarianceDevice(*args, None) == 0, what
    assert (out_c == 7).all() and (out_v == 7).all()
    # the range's ends are inside it, and the variance plane is optional
    assert lib.RaylibAMD_FilterVarianceHost(W, H, P(k=1, sl=1e-3, sn=1e3, sp=1e-3, hl=1.0), planes(), oc, None) == 1
    assert (out_v == 7).all() and (out_c[..., 3] == 1).all()


def test_moments_refusals_write_nothing(lib):
    colour, hit, motion, history = vc.moments_history()
    out_c, out_l, out_m = np.full((H, W, 4), 7, F), np.full((H, W), 7, F), np.full((H, W, 2), 7, F)
    ptr = dict(colour=history[0].ctypes.data, hit=history[1].ctypes.data, length=history[2].ctypes.data, moments=history[3].ctypes.data)
    fr = lambda **kw: C.byref(binding.TemporalMomentsFrame(**dict(ptr, **kw)))
    P = lambda tol=0.02, cap=32.0: C.byref(binding.TemporalParams(tol, cap))
    c_, h_, m_, oc, ol, om = colour.ctypes.data, hit.ctypes.data, motion.ctypes.data, out_c.ctypes.data, out_l.ctypes.data, out_m.ctypes.data
    cases = {"null params": (W, H, None, c_, h_, m_, fr(), oc, ol, om), "null colour": (W, H, P(), None, h_, m_, fr(), oc, ol, om),
             "null hit": (W, H, P(), c_, None, m_, fr(), oc, ol, om), "null motion": (W, H, P(), c_, h_, None, fr(), oc, ol, om),
             "null outColour": (W, H, P(), c_, h_, m_, fr(), None, ol, om), "null outLength": (W, H, P(), c_, h_, m_, fr(), oc, None, om),
             "null outMoments": (W, H, P(), c_, h_, m_, fr(), oc, ol, None), "null outMoments, no history": (W, H, P(), c_, h_, m_, None, oc, ol, None),
             "W = 0": (0, H, P(), c_, h_, m_, fr(), oc, ol, om), "H = 0": (W, 0, P(), c_, h_, m_, fr(), oc, ol, om),
             "W * H = 2^31": (1 << 16, 1 << 15, P(), c_, h_, m_, fr(), oc, ol, om),
             "depthTolerance < 0": (W, H, P(tol=-0.01), c_, h_, m_, fr(), oc, ol, om), "depthTolerance NaN": (W, H, P(tol=float("nan")), c_, h_, m_, fr(), oc, ol, om),
             "maxLength < 1": (W, H, P(cap=0.5), c_, h_, m_, fr(), oc, ol, om), "maxLength inf": (W, H, P(cap=float("inf")), c_, h_, m_, fr(), oc, ol, om),
             "outColour is the history's colour": (W, H, P(), c_, h_, m_, fr(colour=oc), oc, ol, om),
             "outLength is the history's length": (W, H, P(), c_, h_, m_, fr(length=ol), oc, ol, om),
             "outMoments is the history's moments": (W, H, P(), c_, h_, m_, fr(moments=om), oc, ol, om)}
    for k in ptr:
        cases["a history without " + k] = (W, H, P(), c_, h_, m_, fr(**{k: None}), oc, ol, om)
    for what, args in cases.items():
        assert lib.RaylibAMD_TemporalAccumulateMomentsHost(*args) == 0, what
        assert lib.RaylibAMD_TemporalAccumulateMoments(*args) == 0, what
        assert lib.RaylibAMD_TemporalAccumulateMomentsDevice(*args, None) == 0, what
    assert (out_c == 7).all() and (out_l == 7).all() and (out_m == 7).all()
