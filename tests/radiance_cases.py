"""Shared by tests/test_radiance_host.py and tests/test_gpu_radiance.py (RaylibAMD_TraceRadiance, include/raylib_amd.h): the PCG32 streams of
include/raylib_amd_rng.h restated in NumPy for any (pixel, sample), the renderer's pixel coordinates and jitter (reference render/renderer.cc:233-238) in
float32, and the (n, 8) ray records of RaylibAMDPathRay made from RaylibAMD_EvalCameraRays' output."""
import ctypes as C

import numpy as np

F = np.float32
U64 = np.uint64
_A, _C = U64(6364136223846793005), U64(1442695040888963407)


def mix64(z):
    """raylib_rng_mix64 on a uint64 array (wrapping arithmetic)."""
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def stream_begin(seed, pixel, sample):
    """raylib_rng_begin: the states of the streams (seed, pixel[i], sample) as a uint64 array."""
    pixel = np.asarray(pixel, U64)
    key = (pixel << U64(32)) | U64(int(sample) & 0xFFFFFFFF)
    return mix64(mix64(np.array([int(seed) & ((1 << 64) - 1)], U64)) ^ key)


def next_float(state):
    """raylib_rng_next_float on an array of states: (draws as float32, the states behind them)."""
    old = np.asarray(state, U64)
    with np.errstate(over="ignore"):
        new = old * _A + _C
    xs = (((old >> U64(18)) ^ old) >> U64(27)) & U64(0xFFFFFFFF)
    rot = old >> U64(59)
    out = ((xs >> rot) | (xs << ((U64(32) - rot) & U64(31)))) & U64(0xFFFFFFFF)
    return ((out >> U64(8)).astype(F) * F(1.0 / 16777216.0)).astype(F), new


def pixel_uv(w, h, seed=None, sample=0):
    """(u, v) of every pixel in pixel order as renderer.cc:233-238 forms them in float: x / W, y / H, and for sample >= 1 the two jitter draws
    of the stream (seed, y * W + x, sample).  (n, 2) float32."""
    ys, xs = np.mgrid[0:h, 0:w]
    u = (xs.ravel().astype(F) / F(w)).astype(F)
    v = (ys.ravel().astype(F) / F(h)).astype(F)
    if sample != 0:
        s = stream_begin(seed, np.arange(w * h), sample)
        r0, s = next_float(s)
        r1, s = next_float(s)
        u = (u + (((r0 - F(0.5)) * F(2.0)).astype(F) / F(w)).astype(F)).astype(F)
        v = (v + (((r1 - F(0.5)) * F(2.0)).astype(F) / F(h)).astype(F)).astype(F)
    return np.ascontiguousarray(np.stack([u, v], 1), F)


def camera_rays(lib, camera, uv, seed):
    """RaylibAMD_EvalCameraRays: (n, 7) float32 -- org, dir, time -- ray i on the stream (seed, i, 0)."""
    uv = np.ascontiguousarray(uv, F)
    out = np.zeros((len(uv), 7), F)
    assert lib.RaylibAMD_EvalCameraRays(camera, uv.ctypes.data_as(C.POINTER(C.c_float)), len(uv), int(seed), out.ctypes.data_as(C.POINTER(C.c_float))) == 1
    return out


def path_rays(cam_rays, stream=None):
    """(n, 8) float32 records of RaylibAMDPathRay from (n, 7) camera rays; stream (default: the ray's index) goes into the last column's bits."""
    n = len(cam_rays)
    r = np.zeros((n, 8), F)
    r[:, 0:3] = cam_rays[:, 0:3]; r[:, 3] = cam_rays[:, 6]; r[:, 4:7] = cam_rays[:, 3:6]
    r[:, 7] = (np.arange(n) if stream is None else np.asarray(stream)).astype(np.uint32).view(F)
    return r


def frame_rays(lib, ses, w, h, sample=0):
    """The camera rays Raylib_Render generates for sample `sample` of a w x h frame of session `ses`, as path rays on the pixels' streams.  For sample >= 1 the
    camera must be a pinhole with a closed shutter: the lens and time draws of the hook's stream (seed, i, 0) are then not the render's, and must not enter the ray."""
    seed = lib.RaylibAMD_GetSeed()
    return path_rays(camera_rays(lib, ses.camera, pixel_uv(w, h, seed, sample), seed))


def mean_in_order(samples):
    """The renderer's accumulation of per-sample (n, 4) results: the float32 sum in order from +0, times float32(1) / float32(count); alpha 1."""
    acc = np.zeros((len(samples[0]), 3), F)
    for s in samples:
        acc = (acc + s[:, :3]).astype(F)
    out = np.ones((len(acc), 4), F)
    out[:, :3] = (acc * (F(1) / F(len(samples)))).astype(F)
    return out
