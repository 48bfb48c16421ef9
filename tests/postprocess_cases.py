"""Images for Raylib_PostProcess against oracle.postprocess, shared by the host suite (tests/test_host_logic.py: PostProcessHost) and the device suite
(tests/test_gpu_frame_kernels.py: k_pp_max / k_pp_map).

k_pp_max launches min(ceil(n / 256), 2048) workgroups of 256 threads and strides: thread i reads the pixels i, i + STRIDE, i + 2 * STRIDE, ...; one lane per
wave raises the white point with an atomic, and only when its wave found a luminance above 1.  The variants put the pixel that decides the white point where
each of those steps alone can lose it, and the values of the second pass (the cut at 1e-4, the clamp below 1, powf) at their edges.

Every comparison is of float32 bits (a NaN meets a NaN of any sign and payload: helpers.same); the alpha channel must come back untouched."""
import ctypes as C
import functools

import numpy as np

import helpers

STRIDE = 2048 * 256
SMALL = (1, 63, 64, 65, 255, 256, 257)
LARGE = (STRIDE, STRIDE + 1, 3 * STRIDE + 77)
FRAME = (1445, 723)
_WEIGHTS = np.array([0.2126, 0.7152, 0.0722], np.float32)
_F = np.float32


def lum32(rgb):
    """dot(rgb, weights) in float32, in the reference's order (core/vec3.h:117-119)"""
    rgb = np.asarray(rgb, np.float32)
    return (rgb[..., 0] * _WEIGHTS[0] + rgb[..., 1] * _WEIGHTS[1]) + rgb[..., 2] * _WEIGHTS[2]


def shape_for(n):
    """(w, h) with w * h == n, as square as n's divisors allow"""
    d = int(np.sqrt(n))
    while n % d:
        d -= 1
    return n // d, d


def with_luminance(target):
    """an (r, g, b) near grey whose float32 luminance is exactly `target`"""
    target = _F(target)
    greys = [target]
    for step in (np.inf, -np.inf):
        g = target
        for _ in range(64):
            g = np.nextafter(g, _F(step))
            greys.append(g)
    for g in greys:
        if lum32([g, g, g]) == target:
            return (g, g, g)
    for g in greys:
        for b in greys:
            if lum32([g, g, b]) == target:
                return (g, g, b)
    raise AssertionError("no near-grey pixel has the luminance %r" % target)


@functools.lru_cache(maxsize=None)
def base(n):
    """(n, 4) float32, read-only: rgb drawn as gamma(1.0, 0.8) (tests/test_host_logic.py test_postprocess_matches_oracle), alpha anything"""
    rng = np.random.RandomState(1000 + n % 9973)
    img = np.empty((n, 4), np.float32)
    img[:, :3] = rng.gamma(1.0, 0.8, (n, 3)).astype(np.float32)
    img[:, 3] = rng.uniform(-2.0, 2.0, n).astype(np.float32)
    img.setflags(write=False)
    return img


def bright_positions(n):
    """name -> index of the one pixel that decides the white point"""
    last_wave = (n - 1) // 64 * 64                      # its first index; the wave is partial unless n is a multiple of 64
    pos = {"first": 0, "last": n - 1, "last_wave": last_wave + (n - 1 - last_wave) // 2}
    if n > STRIDE:
        pos["second_stride"] = STRIDE + min(n - STRIDE - 1, 12345)
    if n > 2 * STRIDE:
        pos["third_stride"] = 2 * STRIDE + min(n - 2 * STRIDE - 1, 54321)
    distinct = {}
    for name, i in pos.items():                         # (a small image has one index under several names: each index once)
        if i not in distinct.values():
            distinct[name] = i
    return distinct


@functools.lru_cache(maxsize=None)
def edge_pixels():
    cut, nan, inf = _F(0.0001), _F(np.nan), _F(np.inf)
    up, down = np.nextafter(cut, _F(1)), np.nextafter(cut, _F(0))
    finite = [
        ("grey 1e-4", (cut,) * 3), ("grey 1.0001e-4", (_F(1.0001e-4),) * 3), ("grey below 1e-4", (down,) * 3),
        ("luminance 1e-4", with_luminance(cut)), ("luminance above 1e-4", with_luminance(up)), ("luminance below 1e-4", with_luminance(down)),
        ("zero", (0.0,) * 3), ("minus zero", (-0.0,) * 3), ("negative grey", (-0.5,) * 3), ("small negative grey", (-1e-5,) * 3),
        ("denormal", (1e-45,) * 3), ("largest denormal", (1.1754942e-38,) * 3),
        ("negative red", (-1.0, 2.0, 0.1)), ("negative green", (5.0, -0.5, 0.3)), ("negative blue", (0.5, 0.5, -0.25)),
        ("nan red", (nan, 0.5, 0.5)), ("nan green", (0.5, nan, 0.5)), ("nan blue", (0.5, 0.5, nan)), ("nan all", (nan,) * 3),
    ]
    infinite = [("plus inf", (0.5, inf, 0.5)), ("minus inf", (-inf, 0.5, 0.5))]
    return finite, infinite


def _planted(img, pixels):
    """copies of img with the pixels planted from the first index to the last; more than one copy only when img is smaller than the list"""
    n = len(img)
    for k in range(0, len(pixels), n):
        group = pixels[k:k + n]
        out = img.copy()
        at = np.linspace(0, n - 1, len(group)).astype(np.int64)
        assert len(set(at.tolist())) == len(group)
        for i, (_, rgb) in zip(at, group):
            out[i, :3] = rgb
        yield out


def variants(n):
    """(name, (n, 4) float32) for n pixels"""
    b = base(n)
    for name, i in bright_positions(n).items():
        img = b.copy()
        img[i, :3] = (700.0, 900.0, 400.0)
        assert lum32(img[:, :3]).argmax() == i
        yield "bright " + name, img
    # every luminance at most 1: the white point stays 1 and no wave runs its atomic; then exactly one wave does
    dim = b.copy()
    dim[:, :3] *= _F(0.99) / lum32(b[:, :3]).max()
    one, above = with_luminance(1.0), with_luminance(np.nextafter(_F(1), _F(2)))
    dim[n // 2, :3] = one
    assert lum32(dim[:, :3]).max() == 1.0
    yield "dim", dim
    if n > 1:
        ulp = dim.copy()
        ulp[n // 3, :3] = above
        assert lum32(ulp[:, :3]).max() == np.nextafter(_F(1), _F(2))
        yield "dim but one ulp", ulp
    finite, infinite = edge_pixels()
    for k, img in enumerate(_planted(b, finite)):
        yield "edges %d" % k, img
    if n <= max(SMALL):                                 # (the second pass is per pixel: a large image adds nothing to this one)
        for k, img in enumerate(_planted(dim, finite)):
            yield "edges in a dim image %d" % k, img
    for k, img in enumerate(_planted(b, finite + infinite)):
        yield "edges with infinities %d" % k, img
    for grey in (3e38, 1e19):
        img = b.copy()
        img[n // 2, :3] = grey
        yield "grey %g" % grey, img


def post_process(lib, rgba):
    """Raylib_PostProcess of an image made from host pixels (RaylibAMD_CreateImageFromData); rgba: (h, w, 4) float32"""
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    fp = C.POINTER(C.c_float)
    ih = lib.RaylibAMD_CreateImageFromData(w, h, rgba.ctypes.data_as(fp))
    assert ih
    lib.Raylib_PostProcess(ih)
    got = np.full_like(rgba, -7.0)
    lib.RaylibAMD_DumpImageRGBA(ih, got.ctypes.data_as(fp))
    lib.Raylib_DestroyImage(ih)
    return got


def assert_post_processed(got, want, src, what):
    """got is the oracle's image `want` of `src`: rgb bit for bit (NaN for NaN), alpha src's own bits"""
    got, want, src = (np.asarray(a).reshape(-1, 4) for a in (got, want, src))
    assert np.array_equal(helpers.bits(got[:, 3]), helpers.bits(src[:, 3])), "%s: alpha changed" % (what,)
    eq = helpers.same(got[:, :3], want[:, :3]).all(-1)
    if not eq.all():
        i = int(np.nonzero(~eq)[0][0])
        raise AssertionError("%s: %d of %d pixels differ from the oracle, first %d: in %r got %r want %r"
                             % (what, int((~eq).sum()), len(eq), i, src[i, :3].tolist(), got[i, :3].tolist(), want[i, :3].tolist()))


def check_pixel_count(lib, oracle, n):
    """every variant of n pixels through Raylib_PostProcess and the oracle; returns the number of images compared"""
    w, h = shape_for(n)
    count = 0
    for name, img in variants(n):
        src = img.reshape(h, w, 4)
        assert_post_processed(post_process(lib, src), oracle.postprocess(src), src, "%d pixels (%d x %d), %s" % (n, w, h, name))
        count += 1
    return count
