"""The denoiser on the device (RaylibAMD_Denoise / Raylib_Denoise behind the switch, csrc/rl_denoise.hip): bit for bit the host
restatement RaylibAMD_DenoiseHost on synthetic frames and on Cornell renders with their Albedo and MicrosurfaceNormal AOVs, the
reference front-ends' sequence (src/main.cc:456-500), the quality it buys at 16 spp, and its time on a 1080p frame."""
import ctypes as C
import time
import numpy as np
import pytest

import helpers
from helpers import bits
from raylib_amd import binding

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 3), (7, 5), (67, 41), (40, 9), (23, 64)]
GUIDES = ((1, 1), (1, 0), (0, 1), (0, 0))


def fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def params(K, sc, sn, sa):
    return binding.DenoiseParams(int(K), float(sc), float(sn), float(sa))


def pref(p):
    return C.byref(p) if p is not None else None


def dump(lib, img):
    w, h = C.c_uint32(), C.c_uint32()
    assert lib.RaylibAMD_ImageSize(img, C.byref(w), C.byref(h)) == 1
    out = np.zeros((h.value, w.value, 4), np.float32)
    lib.RaylibAMD_DumpImageRGBA(img, fp(out))
    return out


def host(lib, color, hdr, albedo, normal, p):
    h, w = color.shape[:2]
    out = np.zeros((h, w, 4), np.float32)
    assert lib.RaylibAMD_DenoiseHost(w, h, fp(color), hdr, fp(albedo), fp(normal), pref(p), fp(out)) == 1
    return out


def from_data(lib, a):
    a = np.ascontiguousarray(a, np.float32)
    return lib.RaylibAMD_CreateImageFromData(a.shape[1], a.shape[0], fp(a))


def render(lib, ses, w, h, spp, mode=binding.RENDERMODE_DEFAULT, camera=None):
    img = lib.Raylib_CreateImage(w, h)
    st = binding.RendererSettings(w, h, spp, 5, 1e-4, mode)
    lib.Raylib_Render(C.byref(st), ses.scene, camera or ses.camera, img)
    return img


def synthetic(w, h, seed):
    rng = np.random.RandomState(seed)
    albedo = np.zeros((h, w, 4), np.float32)
    albedo[:, : w // 2, :3] = (0.2, 0.3, 0.25)
    albedo[:, w // 2:, :3] = (0.8, 0.7, 0.75)
    normal = np.zeros((h, w, 4), np.float32)
    normal[: h // 2, :, :3] = (0.5, 0.5, 1.0)
    normal[h // 2:, :, :3] = (0.5, 1.0, 0.5)
    color = np.ones((h, w, 4), np.float32)
    color[..., :3] = np.abs(albedo[..., :3] * (1.0 + 0.5 * rng.standard_normal((h, w, 1))) * (2.0 + rng.rand(h, w, 3))).astype(np.float32)
    if w > 4 and h > 4:
        albedo[:2, :2] = 0.0; normal[:2, :2] = 0.0; color[:2, :2, :3] = 3.0
    color[h // 3, w // 3, 0] = np.nan   # counted, read as 0
    return color, albedo, normal


def tone(x):
    x = np.maximum(x[..., :3].astype(np.float64), 0.0)
    return x / (1.0 + x)


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_host_on_host_images(gpu_lib, w, h):
    """Images that only ever lived on the host (RaylibAMD_CreateImageFromData): uploaded, filtered, bit-identical to the host filter, for every K,
    both weight spaces and every guide combination; half of the calls write into main itself, the others into a 0 x 0 image (reallocated)."""
    lib = gpu_lib
    color, albedo, normal = synthetic(w, h, seed=w * 7 + h)
    for K in range(1, 9):
        sc, sn, sa = (2.0, 0.3, 0.05) if K % 2 else (0.5, 0.7, 0.1)
        for hdr in (0, 1):
            for i, (use_a, use_n) in enumerate(GUIDES):
                p = params(K, sc, sn, sa)
                a, n = (albedo if use_a else None), (normal if use_n else None)
                want = host(lib, color, hdr, a, n, p)
                m = from_data(lib, color)
                ah, nh = (from_data(lib, a) if use_a else None), (from_data(lib, n) if use_n else None)
                in_place = (i + K + hdr) % 2 == 0
                out = m if in_place else lib.Raylib_CreateImage(0, 0)
                assert lib.RaylibAMD_Denoise(m, hdr, ah, nh, out, C.byref(p)) == 1
                got = dump(lib, out)
                assert got.shape == (h, w, 4)
                assert np.array_equal(bits(got), bits(want)), "%dx%d K=%d hdr=%d guides=%s in_place=%s: %d words differ" % (
                    w, h, K, hdr, (use_a, use_n), in_place, int((bits(got) != bits(want)).sum()))
                for img in {m, out, ah, nh} - {None}:
                    assert lib.Raylib_DestroyImage(img) == 1


def test_device_equals_host_on_cornell_renders(gpu_lib, sessions):
    """Main image and AOVs rendered on the device (they stay there), all guide combinations and both weight spaces, output into a separate
    image and finally into main itself; Raylib_GetLastStats still reports the render's numbers afterwards."""
    lib = gpu_lib
    ses = sessions["cornell"]
    w, h = 96, 72
    m = render(lib, ses, w, h, 8)
    s0 = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(s0))
    ah = render(lib, ses, w, h, 8, binding.RENDERMODE_ALBEDO)
    nh = render(lib, ses, w, h, 8, binding.RENDERMODE_MICROSURFACE_NORMAL)
    color, albedo, normal = dump(lib, m), dump(lib, ah), dump(lib, nh)
    assert (albedo[..., :3] > 0).any() and (normal[..., :3] > 0).any()
    out = lib.Raylib_CreateImage(w, h)
    try:
        for hdr in (0, 1):
            for use_a, use_n in GUIDES:
                for p in (None, params(3, 0.5, 0.3, 0.1), params(8, 1.0, 0.2, 0.05)):
                    want = host(lib, color, hdr, albedo if use_a else None, normal if use_n else None, p)
                    assert lib.RaylibAMD_Denoise(m, hdr, ah if use_a else None, nh if use_n else None, out, pref(p)) == 1
                    got = dump(lib, out)
                    assert np.array_equal(bits(got), bits(want)), (hdr, use_a, use_n)
        # the render's numbers survive a denoise that follows the render
        m2 = render(lib, ses, w, h, 8)
        assert lib.RaylibAMD_Denoise(m2, 1, ah, nh, out, None) == 1
        s1 = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(s1))
        assert (s1.rays, s1.cameraSamples, s1.pixels) == (s0.rays, s0.cameraSamples, s0.pixels)
        lib.Raylib_DestroyImage(m2)
        # out == main
        want = host(lib, color, 1, albedo, normal, None)
        assert lib.RaylibAMD_Denoise(m, 1, ah, nh, m, None) == 1
        assert np.array_equal(bits(dump(lib, m)), bits(want))
    finally:
        for img in (m, ah, nh, out):
            lib.Raylib_DestroyImage(img)


def test_device_argument_checks_leave_out_untouched(gpu_lib):
    lib = gpu_lib
    color, albedo, normal = synthetic(16, 12, seed=5)
    m, a = from_data(lib, color), from_data(lib, albedo)
    small = from_data(lib, normal[:, :8])
    prev = np.random.RandomState(1).rand(5, 3, 4).astype(np.float32)
    out = from_data(lib, prev)
    try:
        assert lib.RaylibAMD_Denoise(m, 1, a, small, out, None) == 0
        assert lib.RaylibAMD_Denoise(m, 1, small, None, out, None) == 0
        for p in (params(0, 2.0, 0.3, 0.05), params(9, 2.0, 0.3, 0.05), params(5, 0.0, 0.3, 0.05), params(5, 2.0, float("nan"), 0.05)):
            assert lib.RaylibAMD_Denoise(m, 1, a, None, out, C.byref(p)) == 0
        assert lib.RaylibAMD_Denoise(None, 1, a, None, out, None) == 0
        assert lib.RaylibAMD_Denoise(m, 1, a, None, None, None) == 0
        assert np.array_equal(bits(dump(lib, out)), bits(prev))
    finally:
        for img in (m, a, small, out):
            lib.Raylib_DestroyImage(img)


def test_front_end_sequence_with_the_switch_on(gpu_lib, sessions):
    """reference src/main.cc:456-500 through Raylib_* only: Render, the two AOVs with an aperture-0 copy of the camera, Raylib_Denoise into a
    0 x 0 image, Raylib_PostProcess, Raylib_DumpImageData -- equal to the host filter followed by the host post-process."""
    lib = gpu_lib
    ses = sessions["cornell_glass_sun"]   # a lens camera (aperture 0.05, focal 4): the AOVs use the pinhole copy
    w, h = 80, 60
    oracle = helpers.ffi.load_oracle()
    assert lib.Raylib_IsDenoiserSupported() == 0
    lib.RaylibAMD_EnableDenoiser(1)
    debug = lib.Raylib_CreateCamera()
    images = []
    try:
        assert lib.Raylib_IsDenoiserSupported() == 1
        main = render(lib, ses, w, h, 16); images.append(main)
        lib.Raylib_CameraCopy(ses.camera, debug)
        lib.Raylib_CameraSetLens(debug, 0.0, 4.0)
        albedo = render(lib, ses, w, h, 16, binding.RENDERMODE_ALBEDO, camera=debug); images.append(albedo)
        normal = render(lib, ses, w, h, 16, binding.RENDERMODE_MICROSURFACE_NORMAL, camera=debug); images.append(normal)
        raw, A, N = dump(lib, main), dump(lib, albedo), dump(lib, normal)
        out = lib.Raylib_CreateImage(0, 0); images.append(out)
        assert lib.Raylib_Denoise(main, 1, albedo, normal, out) == 1
        lib.Raylib_PostProcess(out)
        final = np.zeros(w * h * 3, np.float32)
        lib.Raylib_DumpImageData(out, fp(final))
        want = oracle.postprocess(host(lib, raw, 1, A, N, None))[..., :3]
        assert np.array_equal(bits(final.reshape(h, w, 3)), bits(want))
        assert np.array_equal(bits(dump(lib, main)), bits(raw))   # main is not touched
    finally:
        lib.RaylibAMD_EnableDenoiser(0)
        lib.Raylib_DestroyCamera(debug)
        for img in images:
            lib.Raylib_DestroyImage(img)
    assert lib.Raylib_IsDenoiserSupported() == 0


# measured with the committed defaults ("Denoiser"): 7.66
QUALITY_FLOOR = 7.0


def test_denoised_16spp_cornell_is_closer_to_1024spp(gpu_lib, sessions):
    """MSE against a 1024-spp frame (another seed) in x / (1 + x) space: the denoised 16-spp frame's is at least QUALITY_FLOOR times below the raw one's."""
    lib = gpu_lib
    ses = sessions["cornell"]
    w = h = 128
    images = []
    try:
        lib.RaylibAMD_SetSeed(1)
        main = render(lib, ses, w, h, 16); images.append(main)
        albedo = render(lib, ses, w, h, 16, binding.RENDERMODE_ALBEDO); images.append(albedo)
        normal = render(lib, ses, w, h, 16, binding.RENDERMODE_MICROSURFACE_NORMAL); images.append(normal)
        lib.RaylibAMD_SetSeed(3)
        ref = render(lib, ses, w, h, 1024); images.append(ref)
        out = lib.Raylib_CreateImage(w, h); images.append(out)
        assert lib.RaylibAMD_Denoise(main, 1, albedo, normal, out, None) == 1
        truth = tone(dump(lib, ref))
        raw = float(((tone(dump(lib, main)) - truth) ** 2).mean())
        den = float(((tone(dump(lib, out)) - truth) ** 2).mean())
        print("Cornell %dx%d 16 spp: MSE raw %.5f, denoised %.5f, ratio %.2f" % (w, h, raw, den, raw / den))
        assert raw >= QUALITY_FLOOR * den, (raw, den)
    finally:
        lib.RaylibAMD_SetSeed(1)
        for img in images:
            lib.Raylib_DestroyImage(img)


def test_denoise_time_1080p(gpu_lib, workdir):
    """A 1920 x 1080 Cornell frame with its two AOVs, K = 5 (the defaults): wall clock around the synchronous call, median of 20 after warm-up."""
    lib = gpu_lib
    obj, c = helpers.build_case("cornell", workdir)
    ses = binding.SceneSession(lib, obj, c["origin"], c["look_at"], c["fov"], 1920 / 1080)
    images = []
    try:
        main = render(lib, ses, 1920, 1080, 4); images.append(main)
        albedo = render(lib, ses, 1920, 1080, 1, binding.RENDERMODE_ALBEDO); images.append(albedo)
        normal = render(lib, ses, 1920, 1080, 1, binding.RENDERMODE_MICROSURFACE_NORMAL); images.append(normal)
        out = lib.Raylib_CreateImage(1920, 1080); images.append(out)
        for _ in range(3):
            assert lib.RaylibAMD_Denoise(main, 1, albedo, normal, out, None) == 1
        times = []
        for _ in range(20):
            t0 = time.perf_counter()
            assert lib.RaylibAMD_Denoise(main, 1, albedo, normal, out, None) == 1
            times.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(times))
        print("denoise 1920x1080 K=5: median %.3f ms, min %.3f ms (wall clock, synchronous call)" % (med, min(times)))
        assert med < 5.0, times
    finally:
        for img in images:
            lib.Raylib_DestroyImage(img)
        ses.close()
