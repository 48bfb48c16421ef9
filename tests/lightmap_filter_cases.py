"""Shared by tests/test_lightmap_filter_host.py and tests/test_gpu_lightmap_filter.py: statement F of include/raylib_amd.h (the lightmap atlas filter)
restated in NumPy float32 -- every operation elementwise in the stated order, expf from the host's libm through ctypes one call per element (as
tests/test_math_exact.py, which holds the library's expf_ to it): the restatement is exact, not approximate.  It works on the atlas, with a coverage mask,
where the library works on the points in compacted form."""
import ctypes as C

import numpy as np

import lightmap_cases as lc

F = np.float32
KERNEL = [F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16)]
CHANNELS = {0: 4, 1: 27}


def _libm_expf():
    m = C.CDLL("libm.so.6")
    m.expf.restype, m.expf.argtypes = C.c_float, [C.c_float]
    return m.expf


_EXPF = _libm_expf()


def expf(x):
    """The host libm's expf of every element of a float32 array."""
    x = np.ascontiguousarray(x, F)
    return np.array([_EXPF(float(v)) for v in x.ravel()], F).reshape(x.shape)


def constants(k, sigma_color, sigma_normal, sigma_position):
    """F4: invC[i], invN, invP[i]."""
    sc, sn, sp = F(sigma_color), F(sigma_normal), F(sigma_position)
    inv_c = [F(F(1 << (2 * i)) / F(sc * sc)) for i in range(k)]
    inv_n = F(F(1) / F(sn * sn))
    inv_p = []
    for i in range(k):
        s = F(sp * F(1 << i))
        inv_p.append(F(F(1) / F(s * s)))
    return inv_c, inv_n, inv_p


def _key(v):
    c = np.where(v > 0, v, F(0)).astype(F)
    return (c / (F(1) + c).astype(F)).astype(F)


def _dist2(a, b):
    d = (a - b).astype(F)
    return (((d[..., 0] * d[..., 0]).astype(F) + (d[..., 1] * d[..., 1]).astype(F)).astype(F) + (d[..., 2] * d[..., 2]).astype(F)).astype(F)


def _shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx], `fill` where that is outside."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        b[yd, xd] = a[ys, xs]
    return b


def filter_atlas(atlas, cov, pos, nrm, filt):
    """Statement F on an atlas (h, w, C) whose texels with cov == 1 take part; pos, nrm (h, w, 3): their gather points.  filt: (K, sigmaColor, sigmaNormal,
    sigmaPosition).  Returns the atlas after the filter: the other texels +0."""
    k, sc, sn, sp = filt
    inv_c, inv_n, inv_p = constants(k, sc, sn, sp)
    h, w, c = atlas.shape
    nf = 3 if c == 4 else c
    on = cov == 1
    with np.errstate(all="ignore"):
        cur = np.where(np.isfinite(atlas[..., :nf]) & on[..., None], atlas[..., :nf], F(0)).astype(F)
        for i in range(k):
            s = 1 << i
            key = _key(cur[..., :3])
            sw = np.zeros((h, w), F)
            acc = np.zeros((h, w, nf), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    valid = on & _shift(on, s * dx, s * dy, False)
                    if not valid.any():
                        continue
                    q = _shift(cur, s * dx, s * dy)
                    dc = _dist2(_shift(key, s * dx, s * dy), key)
                    dn = _dist2(_shift(nrm, s * dx, s * dy), nrm)
                    dp = _dist2(_shift(pos, s * dx, s * dy), pos)
                    arg = (-(((dc * inv_c[i]).astype(F) + (dn * inv_n).astype(F)).astype(F) + (dp * inv_p[i]).astype(F)).astype(F)).astype(F)
                    e = np.zeros((h, w), F)
                    e[valid] = expf(arg[valid])
                    wgt = (F(KERNEL[dx + 2] * KERNEL[dy + 2]) * e).astype(F)
                    sw = np.where(valid, (sw + wgt).astype(F), sw)
                    acc = np.where(valid[..., None], (acc + (wgt[..., None] * q).astype(F)).astype(F), acc)
            cur = np.where(on[..., None], (acc / np.where(on, sw, F(1))[..., None]).astype(F), F(0)).astype(F)
    out = np.zeros((h, w, c), F)
    out[..., :nf] = cur
    if c == 4:
        out[..., 3] = np.where(on, F(1), F(0))
    return out


def planes(points, texel, w, h):
    """The points' positions and normals as (h, w, 3) planes (zeros elsewhere) and the coverage (h, w) uint8."""
    pos = np.zeros((h * w, 3), F); nrm = np.zeros((h * w, 3), F); cov = np.zeros(h * w, np.uint8)
    pos[texel] = points[:, 0:3]; nrm[texel] = points[:, 4:7]; cov[texel] = 1
    return pos.reshape(h, w, 3), nrm.reshape(h, w, 3), cov.reshape(h, w)


def filter_values(values, points, texel, w, h, filt):
    """Statement F in compacted form, through filter_atlas: (n, C) -> (n, C)."""
    atlas, cov = lc.scatter(values, texel, w, h)
    pos, nrm, _ = planes(points, texel, w, h)
    out = filter_atlas(atlas, cov, pos, nrm, filt)
    return np.ascontiguousarray(out.reshape(h * w, -1)[texel])


def synthetic_values(n, kind, seed, signed=None):
    """Values for n points: a smooth part plus noise, positive for IRRADIANCE (alpha 1), signed for SH9."""
    c = CHANNELS[kind]
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)[:, None]
    v = 0.6 + 0.4 * np.sin(t * 0.013 + np.arange(c)[None, :]) + rng.normal(0.0, 0.25, (n, c))
    if (kind == 1) if signed is None else signed:
        v[:, 3:] -= 0.6
    else:
        v = np.abs(v)
    v = v.astype(F)
    if c == 4:
        v[:, 3] = 1
    return v
