"""Shared by tests/test_gather_host.py and tests/test_gpu_gather.py (RaylibAMD_Gather, include/raylib_amd.h): statements 1, 3 and 4 of the header's contract
restated in NumPy float32 on the streams of tests/radiance_cases.py.  Every operation is one float32 operation on float32 arrays, in the header's order; the
sine and cosine of phi are not NumPy's to restate: the caller passes `sincos` (phi -> (sin, cos)), the device's own (RaylibAMD_EvalDeviceMath 9 / 10) on the
GPU.  Statement 2, the radiance along the direction, is RaylibAMD_TraceRadiance's."""
import ctypes as C

import numpy as np

import radiance_cases as rc

F = np.float32
IRRADIANCE, SH9 = 0, 1
OUT_FLOATS = {IRRADIANCE: 4, SH9: 27}
SOLID_ANGLE = {IRRADIANCE: np.array([0x40C90FDB], np.uint32).view(F)[0], SH9: np.array([0x41490FDB], np.uint32).view(F)[0]}   # 6.2831855f, 12.566371f
Y_CONST = [F(0.282095), F(0.488603), F(1.092548), F(0.315392), F(0.546274)]


def points(pos, normal, time=0.0, stream=None):
    """(n, 8) float32 records of RaylibAMDGatherPoint; stream (default: the point's index) goes into the last column's bits."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    n = len(pos)
    p = np.zeros((n, 8), F)
    p[:, 0:3] = pos; p[:, 3] = time; p[:, 4:7] = np.asarray(normal, F).reshape(-1, 3)
    p[:, 7] = (np.arange(n) if stream is None else np.asarray(stream)).astype(np.uint32).view(F)
    return p


def streams_of(pts):
    return np.ascontiguousarray(pts[:, 7]).view(np.uint32)


def first_draws(seed, pts, sample_index, skip_draws):
    """u1, u2 of every point: the draws skip_draws + 1 and skip_draws + 2 of the stream (seed, point's stream, sample_index)."""
    s = rc.stream_begin(seed, streams_of(pts), sample_index)
    for _ in range(int(skip_draws)):
        _, s = rc.next_float(s)
    u1, s = rc.next_float(s)
    u2, s = rc.next_float(s)
    return u1, u2


def dot3(a, b):
    """a.x b.x + a.y b.y + a.z b.z, summed left to right in float32"""
    return ((a[:, 0] * b[:, 0]).astype(F) + (a[:, 1] * b[:, 1]).astype(F) + (a[:, 2] * b[:, 2]).astype(F)).astype(F)


def unit_sphere(u1, u2, sincos):
    """RandomInUnitSphere's vector before it is normalised, (n, 3), and z = 1 - 2 u1"""
    z = (F(1) - (F(2) * u1).astype(F)).astype(F)
    r = np.sqrt(np.maximum(F(0), (F(1) - (z * z).astype(F)).astype(F))).astype(F)
    phi = ((F(2) * F(3.141592)) * u2).astype(F)
    sn, cs = sincos(phi)
    return np.stack([(r * cs).astype(F), (r * sn).astype(F), z], 1).astype(F)


def directions(seed, pts, kind, sample_index, skip_draws, sincos):
    """Statement 1: Wi of every point for the sample whose stream index is sample_index (= sampleFirst + s), (n, 3) float32."""
    u1, u2 = first_draws(seed, pts, sample_index, skip_draws)
    w = unit_sphere(u1, u2, sincos)
    if kind == IRRADIANCE:
        with np.errstate(invalid="ignore"):
            flip = dot3(w, pts[:, 4:7]).astype(np.float64) < 0.0
        w = np.where(flip[:, None], -w, w).astype(F)
    k = (F(1) / np.sqrt(dot3(w, w)).astype(F)).astype(F)
    return (w * k[:, None]).astype(F)


def basis(wi):
    """Y_0 .. Y_8 of statement 3 at the directions wi, (n, 9) float32"""
    x, y, z = wi[:, 0], wi[:, 1], wi[:, 2]
    c0, c1, c2, c3, c4 = Y_CONST
    m = lambda a, b: (a * b).astype(F)
    return np.stack([np.full(len(wi), c0, F), m(c1, y), m(c1, z), m(c1, x), m(c2, m(x, y)), m(c2, m(y, z)),
                     m(c3, (m(F(3), m(z, z)) - F(1)).astype(F)), m(c2, m(x, z)), m(c4, (m(x, x) - m(y, y)).astype(F))], 1).astype(F)


def sample_values(L, pts, wi, kind):
    """Statement 3: (n, 3) for IRRADIANCE, (n, 27) for SH9 (column 3 j + c), from the radiance L (n, >= 3) along wi."""
    L = np.ascontiguousarray(L, F)[:, :3]
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == IRRADIANCE:
            wgt = np.fmax(F(0), dot3(pts[:, 4:7], wi)).astype(F)      # fmaxf: a NaN gives 0
            return (L * wgt[:, None]).astype(F)
        Y = basis(wi)
        return (L[:, None, :] * Y[:, :, None]).astype(F).reshape(len(L), 27)


def resolve(values, kind):
    """Statement 4 on the per-sample values in sample order: the sum from +0, times float32(1) / float32(count), times the solid angle; IRRADIANCE gets alpha 1."""
    acc = np.zeros_like(values[0], dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in values:
            acc = (acc + v).astype(F)
        out = ((acc * (F(1) / F(len(values)))).astype(F) * SOLID_ANGLE[kind]).astype(F)
    if kind == IRRADIANCE:
        out = np.concatenate([out, np.ones((len(out), 1), F)], 1)
    return np.ascontiguousarray(out, F)


def device_sincos(lib):
    """phi -> (sin, cos) by the device's sincos (RaylibAMD_EvalDeviceMath 9 / 10)"""
    def f(phi):
        phi = np.ascontiguousarray(phi, F)
        out = [np.zeros(len(phi), F), np.zeros(len(phi), F)]
        for fn, o in zip((9, 10), out):
            assert lib.RaylibAMD_EvalDeviceMath(fn, phi.ctypes.data_as(C.POINTER(C.c_float)), None, len(phi), o.ctypes.data_as(C.POINTER(C.c_float))) == 1
        return out[0], out[1]
    return f


def path_rays(pts, wi):
    """The RaylibAMDPathRay records (pos, time, Wi, stream) of statement 2"""
    r = np.array(pts, F)
    r[:, 4:7] = wi
    return r
