"""The denoiser's host restatement (RaylibAMD_DenoiseHost, csrc/rl_denoise.hip) and the ABI around it, without a device:
a NumPy statement of the filter's definition, the properties a denoiser must have, argument checks and the opt-in switch."""
import ctypes as C
import numpy as np
import pytest

import helpers  # noqa: F401  (sets sys.path)
from raylib_amd import binding  # noqa: E402

KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)
DEFAULTS = (5, 2.0, 0.3, 0.05)   # csrc/rl_abi.cc kDenoiseDefaults


def fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def params(K, sc, sn, sa):
    return binding.DenoiseParams(int(K), float(sc), float(sn), float(sa))


def host(lib, color, hdr=1, albedo=None, normal=None, p=None):
    h, w = color.shape[:2]
    out = np.full((h, w, 4), -7.0, np.float32)
    ok = lib.RaylibAMD_DenoiseHost(w, h, fp(color), hdr, fp(albedo), fp(normal), C.byref(p) if p is not None else None, fp(out))
    assert ok == 1
    return out


def numpy_denoise(color, albedo, normal, hdr, K, sc, sn, sa):
    """The definition of include/raylib_amd.h / csrc/rl_denoise.hip in float32 NumPy (np.exp for expf)."""
    f = np.float32
    fin = lambda x: np.where(np.isfinite(x), x, f(0)).astype(f)
    H, W = color.shape[:2]
    with np.errstate(all="ignore"):
        a = np.where(fin(albedo[..., :3]) > f(1e-3), fin(albedo[..., :3]), f(1)).astype(f) if albedo is not None else np.ones((H, W, 3), f)
        I = fin(fin(color[..., :3]) / a)
    n = (f(2) * fin(normal[..., :3]) - f(1)).astype(f) if normal is not None else None
    A = fin(albedo[..., :3]) if albedo is not None else None

    def g(x):
        if not hdr:
            return x
        c = np.maximum(x, f(0))
        return (c / (f(1) + c)).astype(f)

    def d2(u, v):
        d = (u - v).astype(f)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(f)

    invN, invA = f(1) / (f(sn) * f(sn)), f(1) / (f(sa) * f(sa))
    ys, xs = np.arange(H), np.arange(W)
    for i in range(K):
        s, invC = 1 << i, f(4 ** i) / (f(sc) * f(sc))
        G = g(I)
        sw, acc = np.zeros((H, W), f), np.zeros((H, W, 3), f)
        for dy in range(-2, 3):
            qy = ys + s * dy
            vy = (qy >= 0) & (qy < H)
            qy = np.clip(qy, 0, H - 1)
            for dx in range(-2, 3):
                qx = xs + s * dx
                vx = (qx >= 0) & (qx < W)
                qx = np.clip(qx, 0, W - 1)
                take = lambda X: X[qy][:, qx]
                e = (d2(take(G), G) * invC).astype(f)
                if n is not None:
                    e = (e + d2(take(n), n) * invN).astype(f)
                if A is not None:
                    e = (e + d2(take(A), A) * invA).astype(f)
                w = (KERNEL[dx + 2] * KERNEL[dy + 2] * np.exp(-e)).astype(f)
                w = np.where(vy[:, None] & vx[None, :], w, f(0)).astype(f)
                sw = (sw + w).astype(f)
                acc = (acc + w[..., None] * take(I)).astype(f)
        I = (acc / sw[..., None]).astype(f)
    out = np.ones((H, W, 4), f)
    out[..., :3] = I * a
    return out


def synthetic(w, h, seed, miss=True):
    """A noisy frame with its two guides: two albedo regions (a vertical step), two normal regions (a horizontal crease), optionally missed pixels."""
    rng = np.random.RandomState(seed)
    albedo = np.zeros((h, w, 4), np.float32)
    albedo[:, : w // 2, :3] = (0.2, 0.3, 0.25)
    albedo[:, w // 2:, :3] = (0.8, 0.7, 0.75)
    normal = np.zeros((h, w, 4), np.float32)
    normal[: h // 2, :, :3] = (0.5, 0.5, 1.0)
    normal[h // 2:, :, :3] = (0.5, 1.0, 0.5)
    light = 1.0 + 0.5 * rng.standard_normal((h, w, 1)).astype(np.float32)
    color = np.ones((h, w, 4), np.float32)
    color[..., :3] = np.abs(albedo[..., :3] * light * (2.0 + rng.rand(h, w, 3).astype(np.float32)))
    if miss and w > 4 and h > 4:   # a missed corner: black guides, sky colour
        albedo[:2, :2] = 0.0; normal[:2, :2] = 0.0; color[:2, :2, :3] = 3.0
    return color, albedo, normal


SIZES = [(1, 1), (2, 3), (7, 5), (67, 41), (40, 9), (23, 64)]   # (40, 9): W < 5 * 2^(K-1) for every K >= 5; (7, 5) and (2, 3) for all K > 1


@pytest.mark.parametrize("w,h", SIZES)
def test_host_filter_matches_numpy_definition(lib, w, h):
    color, albedo, normal = synthetic(w, h, seed=w * 131 + h)
    rng = np.random.RandomState(w + h)
    for K in range(1, 9):
        for hdr in (0, 1):
            for use_a, use_n in ((1, 1), (1, 0), (0, 1), (0, 0)):
                if rng.rand() > 0.5 and not (K in (1, 5, 8)):
                    continue   # every K and every combination is covered over the sizes, without 64 runs per size
                sc, sn, sa = (0.5, 0.3, 0.1) if K % 2 else (2.0, 0.7, 0.05)
                a, n = (albedo if use_a else None), (normal if use_n else None)
                got = host(lib, color, hdr, a, n, params(K, sc, sn, sa))
                want = numpy_denoise(color, a, n, hdr, K, sc, sn, sa)
                np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7, err_msg="%dx%d K=%d hdr=%d albedo=%d normal=%d" % (w, h, K, hdr, use_a, use_n))


def test_null_params_are_the_defaults(lib):
    color, albedo, normal = synthetic(33, 20, seed=3)
    got = host(lib, color, 1, albedo, normal, None)
    want = host(lib, color, 1, albedo, normal, params(*DEFAULTS))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_output_may_alias_the_input(lib):
    color, albedo, normal = synthetic(19, 13, seed=4)
    want = host(lib, color, 1, albedo, normal)
    buf = color.copy()
    assert lib.RaylibAMD_DenoiseHost(19, 13, fp(buf), 1, fp(albedo), fp(normal), None, fp(buf)) == 1
    assert np.array_equal(buf.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("hdr", [0, 1])
def test_constant_image_stays_constant(lib, hdr):
    for value in (0.37, 5.5):
        color = np.full((24, 31, 4), value, np.float32)
        albedo = np.full((24, 31, 4), 0.5, np.float32)
        normal = np.full((24, 31, 4), 0.75, np.float32)
        for K in (1, 5, 8):
            out = host(lib, color, hdr, albedo, normal, params(K, 0.5, 0.3, 0.1))
            assert (out[..., 3] == 1.0).all()
            assert np.abs(out[..., :3] - np.float32(value)).max() <= 4 * np.spacing(np.float32(value)), (value, K)


def test_edges_survive_and_flat_regions_lose_their_noise(lib):
    """A two-albedo step under noisy light: the noise in each flat region falls by >= 4x, and neither side's mean moves towards the other by 1 %."""
    w, h = 128, 64
    rng = np.random.RandomState(7)
    albedo = np.zeros((h, w, 4), np.float32)
    albedo[:, : w // 2, :3] = 0.2
    albedo[:, w // 2:, :3] = 0.8
    normal = np.zeros((h, w, 4), np.float32); normal[..., :3] = (0.5, 0.5, 1.0)
    light = 1.0 + 0.3 * rng.standard_normal((h, w, 3)).astype(np.float32)
    color = np.ones((h, w, 4), np.float32)
    color[..., :3] = albedo[..., :3] * light
    out = host(lib, color, 1, albedo, normal)
    gap = 0.8 - 0.2
    for cols in (slice(0, w // 2), slice(w // 2, w)):
        before, after = color[:, cols, :3], out[:, cols, :3]
        inner = slice(4, -4)
        assert after[:, inner].var() * 4 <= before[:, inner].var(), (before.var(), after.var())
        side = 0.2 if cols.start == 0 else 0.8
        moved = (after.mean() - before.mean()) * (1 if side == 0.2 else -1)   # towards the other side
        assert moved < 0.01 * gap, (side, before.mean(), after.mean())


def test_nonfinite_input_does_not_spread(lib):
    color, albedo, normal = synthetic(37, 29, seed=9)
    bad = color.copy()
    bad[10, 12, 0] = np.nan; bad[20, 3, 1] = np.inf; bad[5, 30, 2] = -np.inf; bad[0, 0, :3] = np.nan
    zeroed = bad.copy()
    zeroed[..., :3][~np.isfinite(bad[..., :3])] = 0.0
    for hdr in (0, 1):
        got = host(lib, bad, hdr, albedo, normal)
        assert np.isfinite(got).all()
        want = host(lib, zeroed, hdr, albedo, normal)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))   # a non-finite channel is exactly a 0 channel


def test_host_argument_checks_leave_out_untouched(lib):
    color, albedo, normal = synthetic(8, 6, seed=1)
    out = np.full((6, 8, 4), 42.0, np.float32)
    bad_params = [params(0, 0.5, 0.3, 0.1), params(9, 0.5, 0.3, 0.1), params(5, 0.0, 0.3, 0.1), params(5, 0.5, -1.0, 0.1),
                  params(5, 0.5, 0.3, float("nan")), params(5, float("inf"), 0.3, 0.1)]
    for p in bad_params:
        assert lib.RaylibAMD_DenoiseHost(8, 6, fp(color), 1, fp(albedo), fp(normal), C.byref(p), fp(out)) == 0
    assert lib.RaylibAMD_DenoiseHost(8, 6, None, 1, fp(albedo), fp(normal), None, fp(out)) == 0
    assert lib.RaylibAMD_DenoiseHost(8, 6, fp(color), 1, None, None, None, None) == 0
    assert (out == 42.0).all()


def test_device_entry_checks_arguments_before_anything_else(lib):
    """Mismatched guides, out-of-range params and null handles: 0, and the output image keeps its size and pixels."""
    color, albedo, normal = synthetic(8, 6, seed=2)
    m = lib.RaylibAMD_CreateImageFromData(8, 6, fp(color))
    a = lib.RaylibAMD_CreateImageFromData(8, 6, fp(albedo))
    small = lib.RaylibAMD_CreateImageFromData(4, 6, fp(np.ascontiguousarray(normal[:, :4])))
    out = lib.Raylib_CreateImage(3, 2)
    try:
        assert lib.RaylibAMD_Denoise(m, 1, a, small, out, None) == 0
        assert lib.RaylibAMD_Denoise(m, 1, small, None, out, None) == 0
        assert lib.RaylibAMD_Denoise(m, 1, a, None, out, C.byref(params(9, 0.5, 0.3, 0.1))) == 0
        assert lib.RaylibAMD_Denoise(None, 1, a, None, out, None) == 0
        assert lib.RaylibAMD_Denoise(m, 1, a, None, None, None) == 0
        w, h = C.c_uint32(), C.c_uint32()
        assert lib.RaylibAMD_ImageSize(out, C.byref(w), C.byref(h)) == 1 and (w.value, h.value) == (3, 2)
        px = np.full(3 * 2 * 4, 5.0, np.float32)
        lib.RaylibAMD_DumpImageRGBA(out, fp(px))
        assert (px == 0.0).all()
    finally:
        for i in (m, a, small, out):
            assert lib.Raylib_DestroyImage(i) == 1


def test_denoiser_switch_is_off_by_default(lib):
    """Raylib_IsDenoiserSupported / Raylib_Denoise keep the reference's no-OIDN answers unless the switch is turned on; on a machine without a
    device the switch on still answers 0 (RaylibAMD_DeviceAvailable)."""
    color = np.ones((4, 4, 4), np.float32)
    m = lib.RaylibAMD_CreateImageFromData(4, 4, fp(color))
    out = lib.Raylib_CreateImage(4, 4)
    try:
        assert lib.Raylib_IsDenoiserSupported() == 0
        assert lib.Raylib_Denoise(m, 1, None, None, out) == 0
        lib.RaylibAMD_EnableDenoiser(1)
        have = lib.RaylibAMD_DeviceAvailable()
        assert lib.Raylib_IsDenoiserSupported() == have
        assert lib.Raylib_Denoise(m, 1, None, None, out) == have
        lib.RaylibAMD_EnableDenoiser(0)
        assert lib.Raylib_IsDenoiserSupported() == 0
        assert lib.Raylib_Denoise(m, 1, None, None, out) == 0
    finally:
        lib.RaylibAMD_EnableDenoiser(0)
        lib.Raylib_DestroyImage(m); lib.Raylib_DestroyImage(out)
