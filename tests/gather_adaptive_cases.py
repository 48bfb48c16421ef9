"""Shared by tests/test_gather_adaptive_host.py and tests/test_gpu_gather_adaptive.py (RaylibAMD_GatherAdaptive, include/raylib_amd.h): statements A2 and A3
restated in NumPy float32, one float32 operation per statement, over all points at once.  A1's passes are the loop; A4's result is tests/gather_cases.py
resolve on the samples a point took."""
import numpy as np

F = np.float32
LUMA = (F(0.2126), F(0.7152), F(0.0722))


def moments(keys):
    """A2: keys (count, cap, 3) float32 in sample order -> the running S1, S2 after 1 .. cap samples, each (count, cap) float32."""
    keys = np.ascontiguousarray(keys, F)
    count, cap = keys.shape[:2]
    s1 = np.zeros((count, cap), F)
    s2 = np.zeros((count, cap), F)
    a1 = np.zeros(count, F)
    a2 = np.zeros(count, F)
    with np.errstate(all="ignore"):
        for s in range(cap):
            k = keys[:, s]
            lum = ((k[:, 0] * LUMA[0]).astype(F) + (k[:, 1] * LUMA[1]).astype(F)).astype(F)
            lum = (lum + (k[:, 2] * LUMA[2]).astype(F)).astype(F)
            y = (lum / (F(1) + lum).astype(F)).astype(F)
            a1 = (a1 + y).astype(F)
            a2 = (a2 + (y * y).astype(F)).astype(F)
            s1[:, s] = a1
            s2[:, s] = a2
    return s1, s2


def error(s1, s2, n):
    """A3's error after n samples (csrc/rl_progressive.h): sqrt(max(0, (S2 - S1 * S1 / n) / (n - 1)) / n) in float32; +inf when S1, S2 or the value is not finite."""
    nf = F(n)
    with np.errstate(all="ignore"):
        v = (s1 * s1).astype(F)
        v = (v / nf).astype(F)
        v = (s2 - v).astype(F)
        v = (v / F(nf - F(1))).astype(F)
        v = np.where(v < F(0), F(0), v).astype(F)           # (NaN stays NaN)
        se = np.sqrt((v / nf).astype(F)).astype(F)
    return np.where(np.isfinite(se) & np.isfinite(s1) & np.isfinite(s2), se, F(np.inf)).astype(F)


def pass_counts(cap, pass_samples):
    """A1: n_1 .. n_P"""
    out, n = [], 0
    while n < cap:
        n = min(cap, n + int(pass_samples))
        out.append(n)
    return out


def decide(keys, threshold, min_samples, pass_samples, cap=None):
    """A1 to A3: the n at which each point stops, (count,) uint32.  keys (count, >= cap, 3)."""
    keys = np.ascontiguousarray(keys, F)
    cap = keys.shape[1] if cap is None else int(cap)
    s1, s2 = moments(keys[:, :cap])
    out = np.zeros(len(keys), np.uint32)
    for n in pass_counts(cap, pass_samples):
        live = out == 0
        if n == cap:
            stop = live
        else:
            stop = live & (n >= int(min_samples)) & (error(s1[:, n - 1], s2[:, n - 1], n) < F(threshold))
        out[stop] = n
    return out
