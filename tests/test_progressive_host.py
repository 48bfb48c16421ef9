"""Progressive rendering without a device: the stopping rule (RaylibAMD_ProgressiveDecideHost, csrc/rl_progressive.h) against a NumPy
restatement of include/raylib_amd.h, and the argument checks of the session exports."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers  # noqa: F401  (sys.path)
from raylib_amd import binding


def decide_numpy(w, h, n_cell, s1, s2, threshold, min_samples):
    """include/raylib_amd.h in float32: se = sqrt(max(0, (S2 - S1*S1/n) / (n - 1)) / n), +inf when S1, S2 or se is not finite; a cell's error is the max over its
    valid pixels; it stops when n >= minSamples and error < threshold."""
    cy, cx = (h + 7) // 8, (w + 7) // 8
    n_px = np.repeat(np.repeat(n_cell, 8, 0), 8, 1)[:h, :w].astype(np.float32)
    with np.errstate(all="ignore"):
        v = (s2 - s1 * s1 / n_px) / (n_px - np.float32(1))
        v = np.maximum(np.float32(0), v)           # (NaN propagates)
        se = np.sqrt(v / n_px).astype(np.float32)
    se = np.where(np.isfinite(se) & np.isfinite(s1) & np.isfinite(s2), se, np.float32(np.inf))
    pad = np.zeros((cy * 8, cx * 8), np.float32)
    pad[:h, :w] = se
    err = pad.reshape(cy, 8, cx, 8).max(axis=(1, 3))
    return (n_cell >= min_samples) & (err < np.float32(threshold))


def _random_case(rng, w, h, n_max=64):
    cy, cx = (h + 7) // 8, (w + 7) // 8
    n = rng.randint(0, n_max + 1, size=(cy, cx)).astype(np.uint32)
    n_px = np.repeat(np.repeat(n, 8, 0), 8, 1)[:h, :w].astype(np.float32)
    # sums of y in [0, 1): S1 <= n, S2 <= S1, with a spread of variances (and some exactly constant pixels)
    mean = rng.rand(h, w).astype(np.float32)
    var = (rng.rand(h, w).astype(np.float32) ** 3) * mean * (1 - mean)
    s1 = (mean * n_px).astype(np.float32)
    s2 = ((var + mean * mean) * n_px).astype(np.float32)
    const = rng.rand(h, w) < 0.1
    s2[const] = (s1[const] * s1[const] / np.maximum(n_px[const], 1)).astype(np.float32)
    return n, s1, s2


@pytest.mark.parametrize("w,h", [(64, 64), (37, 21), (8, 8), (1, 1), (130, 9)])
@pytest.mark.parametrize("threshold", [0.0, 1e-3, 0.01, 0.05, 1.0])
def test_host_rule_matches_numpy_on_random_inputs(lib, w, h, threshold):
    rng = np.random.RandomState(w * 131 + h)
    for min_samples in (2, 4, 17):
        n, s1, s2 = _random_case(rng, w, h)
        got = binding.progressive_decide_host(lib, w, h, n, s1, s2, threshold, min_samples)
        want = decide_numpy(w, h, n, s1, s2, threshold, min_samples)
        assert got is not None and got.shape == want.shape
        assert np.array_equal(got, want), (w, h, threshold, min_samples, np.argwhere(got != want)[:5])
        if threshold == 0.0:
            assert not got.any()


def test_host_rule_edges(lib):
    w, h = 20, 12                       # 3 x 2 cells; the right column and the bottom row are partial
    cy, cx = 2, 3
    # constant pixels (se = 0) everywhere: every cell with n >= minSamples stops at any threshold > 0, none at threshold 0
    n = np.array([[1, 2, 3], [4, 8, 64]], np.uint32)
    n_px = np.repeat(np.repeat(n, 8, 0), 8, 1)[:h, :w].astype(np.float32)
    s1 = (np.float32(0.25) * n_px).astype(np.float32)
    s2 = (np.float32(0.0625) * n_px).astype(np.float32)
    for ms in (2, 3, 8):
        got = binding.progressive_decide_host(lib, w, h, n, s1, s2, 1e-6, ms)
        assert np.array_equal(got, n >= ms), ms
        assert np.array_equal(got, decide_numpy(w, h, n, s1, s2, 1e-6, ms))
    assert not binding.progressive_decide_host(lib, w, h, n, s1, s2, 0.0, 2).any()
    assert not binding.progressive_decide_host(lib, w, h, n, s1, s2, None).any()   # no params: uniform
    # NaN / inf sums in one pixel keep their cell from stopping (error +inf), and only that cell
    for bad in (np.nan, np.inf, -np.inf):
        b1 = s1.copy(); b1[3, 17] = bad           # cell (0, 2)
        b2 = s2.copy(); b2[10, 4] = bad           # cell (1, 0)
        got = binding.progressive_decide_host(lib, w, h, n, b1, b2, 10.0, 2)
        want = decide_numpy(w, h, n, b1, b2, 10.0, 2)
        assert np.array_equal(got, want)
        assert not got[0, 2] and not got[1, 0] and got[1, 1] and got[1, 2] and got[0, 1]
    # only the valid pixels of a partial cell count: garbage beyond the frame does not exist in the W*H arrays -- a noisy pixel inside does
    noisy1, noisy2 = s1.copy(), s2.copy()
    noisy2[11, 19] = noisy1[11, 19] * 3       # bottom-right valid pixel of cell (1, 2): variance > 0
    got = binding.progressive_decide_host(lib, w, h, n, noisy1, noisy2, 1e-3, 2)
    assert np.array_equal(got, decide_numpy(w, h, n, noisy1, noisy2, 1e-3, 2)) and not got[1, 2] and got[1, 1]
    # n < minSamples never stops, whatever the error
    assert not binding.progressive_decide_host(lib, w, h, n, s1, s2, 1e30, 65).any()


def test_host_rule_threshold_is_strict(lib):
    # one pixel, n = 4, y = 0, 0, 0, 1: S1 = 1, S2 = 1 -> var = (1 - 1/4) / 3 = 0.25, se = sqrt(0.25 / 4) = 0.25 exactly
    n = np.array([[4]], np.uint32)
    s1 = np.full((1, 1), 1.0, np.float32)
    s2 = np.full((1, 1), 1.0, np.float32)
    assert not binding.progressive_decide_host(lib, 1, 1, n, s1, s2, 0.25, 2)[0, 0]
    assert binding.progressive_decide_host(lib, 1, 1, n, s1, s2, np.nextafter(np.float32(0.25), np.float32(1)), 2)[0, 0]


def test_host_rule_argument_checks(lib):
    n = np.zeros((1, 1), np.uint32)
    s = np.zeros((8, 8), np.float32)
    out = np.zeros(1, np.uint8)
    P = binding.ProgressiveParams
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    nptr, sptr, optr = n.ctypes.data_as(u32p), binding._fp(s), out.ctypes.data_as(u8p)
    assert lib.RaylibAMD_ProgressiveDecideHost(8, 8, nptr, sptr, sptr, C.byref(P(0.1, 2)), optr) == 1
    for bad in (P(0.1, 1), P(0.1, 0), P(-0.1, 2), P(float("nan"), 2), P(float("inf"), 2)):
        assert lib.RaylibAMD_ProgressiveDecideHost(8, 8, nptr, sptr, sptr, C.byref(bad), optr) == 0
    assert lib.RaylibAMD_ProgressiveDecideHost(8, 8, None, sptr, sptr, None, optr) == 0
    assert lib.RaylibAMD_ProgressiveDecideHost(8, 8, nptr, None, sptr, None, optr) == 0
    assert lib.RaylibAMD_ProgressiveDecideHost(8, 8, nptr, sptr, None, None, optr) == 0
    assert lib.RaylibAMD_ProgressiveDecideHost(8, 8, nptr, sptr, sptr, None, None) == 0


def test_session_exports_refuse_unknown_handles(lib):
    for h in (0, 12345, 0xdeadbeef0):
        assert lib.RaylibAMD_ProgressiveStep(h, 4) == -1
        assert lib.RaylibAMD_ProgressiveExport(h, None, None, None, None) == 0
        assert lib.RaylibAMD_EndProgressive(h) == 0


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-device path: this machine may have a GPU")
def test_begin_without_a_device_returns_0(lib, tmp_path):
    from raylib_amd import scenes
    obj, _ = scenes.cornell(str(tmp_path / "c.obj"))
    ses = binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    try:
        st = ses.settings(16, 16, 4)
        img = lib.Raylib_CreateImage(16, 16)
        assert lib.RaylibAMD_BeginProgressive(C.byref(st), ses.scene, ses.camera, img, None) == 0
        assert lib.RaylibAMD_BeginProgressive(C.byref(st), ses.scene, ses.camera, img, C.byref(binding.ProgressiveParams(0.01, 4))) == 0
        lib.Raylib_DestroyImage(img)
    finally:
        ses.close()


def test_begin_refuses_bad_arguments_before_the_device(lib, tmp_path):
    """Null arguments, an AOV mode, out-of-range params, an empty viewport and an unfinalized scene are refused whether or not there is a device."""
    from raylib_amd import scenes
    obj, _ = scenes.cornell(str(tmp_path / "c.obj"))
    ses = binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    img = lib.Raylib_CreateImage(16, 16)
    try:
        st = ses.settings(16, 16, 4)
        P = binding.ProgressiveParams
        assert lib.RaylibAMD_BeginProgressive(None, ses.scene, ses.camera, img, None) == 0
        assert lib.RaylibAMD_BeginProgressive(C.byref(st), None, ses.camera, img, None) == 0
        assert lib.RaylibAMD_BeginProgressive(C.byref(st), ses.scene, None, img, None) == 0
        assert lib.RaylibAMD_BeginProgressive(C.byref(st), ses.scene, ses.camera, None, None) == 0
        aov = ses.settings(16, 16, 4, mode=binding.RENDERMODE_ALBEDO)
        assert lib.RaylibAMD_BeginProgressive(C.byref(aov), ses.scene, ses.camera, img, None) == 0
        for bad in (P(0.1, 1), P(-1.0, 2), P(float("nan"), 2)):
            assert lib.RaylibAMD_BeginProgressive(C.byref(st), ses.scene, ses.camera, img, C.byref(bad)) == 0
        empty = ses.settings(0, 16, 4)
        assert lib.RaylibAMD_BeginProgressive(C.byref(empty), ses.scene, ses.camera, img, None) == 0
        unfinalized = lib.Raylib_CreateScene()
        assert lib.RaylibAMD_BeginProgressive(C.byref(st), unfinalized, ses.camera, img, None) == 0
        lib.Raylib_DestroyScene(unfinalized)
    finally:
        lib.Raylib_DestroyImage(img)
        ses.close()
