"""Several views of one scene in one megakernel launch (RaylibAMD_RenderViews): every view is, bit for bit, the Raylib_Render of its camera -- on every
schedule the planner can pick, in the debug modes, culled or not -- and the batch is one launch per sample batch for the whole set."""
import ctypes as C

import numpy as np
import pytest

from helpers import bits

W, H = 44, 36   # partial cells on both axes


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def single(lib, ses, cam, w, h, spp, mode=0):
    from raylib_amd import binding
    st = ses.settings(w, h, spp, mode=mode)
    img = lib.Raylib_CreateImage(w, h)
    lib.Raylib_Render(C.byref(st), ses.scene, cam, img)
    out = np.zeros((h, w, 4), np.float32)
    lib.RaylibAMD_DumpImageRGBA(img, _fp(out))
    lib.Raylib_DestroyImage(img)
    return out, ses.stats().as_dict()


def view_set(lib, aspect):
    """A far camera (culled cells), a thin-lens camera, a camera inside the model, and one from the side."""
    from raylib_amd import binding
    return [binding.create_camera(lib, (0.0, 1.0, 14.0), (0.0, 1.0, -1.0), 45.0, aspect),
            binding.create_camera(lib, (0.3, 1.2, 4.0), (0.0, 0.9, -1.0), 45.0, aspect, aperture=0.3, focal=4.0),
            binding.create_camera(lib, (0.0, 1.0, 0.2), (0.3, 0.8, -1.0), 70.0, aspect),
            binding.create_camera(lib, (3.5, 2.5, 6.0), (0.0, 1.0, 0.0), 30.0, aspect)]


def destroy(lib, cams):
    for c in cams:
        lib.Raylib_DestroyCamera(c)


def check_batch(lib, ses, cams, w, h, spp, mode=0):
    got = ses.render_views(cams, w, h, spp, mode=mode)
    bst = ses.stats().as_dict()
    culled = 0
    for i, cam in enumerate(cams):
        want, st1 = single(lib, ses, cam, w, h, spp, mode)
        assert np.array_equal(bits(got[i]), bits(want)), (i, mode)
        culled += st1["culledCells"]
        if mode == 0:
            for k in ("pathsPerWave", "treeWidth", "nodeBytes"):
                assert bst[k] == st1[k], k
    if mode == 0:
        n = len(cams)
        assert bst["cameraSamples"] + bst["culledSamples"] == n * w * h * spp
        assert bst["culledCells"] == culled
    assert bst["pixels"] == len(cams) * w * h
    return bst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cornell", "cutout_sky", "cornell_glass_sun"])
def test_views_equal_single_renders(gpu_lib, sessions, case):
    ses = sessions[case]
    cams = view_set(gpu_lib, W / H) + [ses.camera]
    try:
        bst = check_batch(gpu_lib, ses, cams, W, H, 5)
        if case == "cornell":
            assert gpu_lib.RaylibAMD_LastTracePlain() == 1
            assert bst["culledCells"] > 0
        assert bst["traceLaunches"] == 1
    finally:
        destroy(gpu_lib, cams[:-1])


@pytest.mark.gpu
def test_views_on_tree_and_pool_schedules(gpu_lib, mid_scene, monkeypatch):
    ses, _, _ = mid_scene
    cams = view_set(gpu_lib, W / H)
    try:
        for env, width in ((dict(RAYLIB_POOL="0"), None), (dict(), 4), (dict(RAYLIB_BVH8="1"), 8)):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            bst = check_batch(gpu_lib, ses, cams, W, H, 3)
            if width:
                assert bst["pathsPerWave"] > 64 and bst["treeWidth"] == width, env
            else:
                assert bst["pathsPerWave"] == 64 and bst["treeWidth"] > 0, env
            for k in env:
                monkeypatch.delenv(k)
    finally:
        destroy(gpu_lib, cams)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cornell", "cutout_sky"])
def test_debug_modes(gpu_lib, sessions, case):
    ses = sessions[case]
    cams = view_set(gpu_lib, W / H)
    try:
        for mode in (1, 3):   # Albedo, MicrosurfaceNormal: the denoiser's guides
            check_batch(gpu_lib, ses, cams, W, H, 1, mode=mode)
    finally:
        destroy(gpu_lib, cams)


@pytest.mark.gpu
def test_one_launch_for_the_whole_set(gpu_lib, sessions, monkeypatch):
    ses = sessions["cornell"]
    cams = (view_set(gpu_lib, W / H) * 2)[:6]
    try:
        ses.render_views(cams[:1], W, H, 4)
        assert ses.stats().traceLaunches == 1
        ses.render_views(cams, W, H, 4)
        assert ses.stats().traceLaunches == 1
        monkeypatch.setenv("RAYLIB_SAMPLE_BATCH", "3")
        got = ses.render_views(cams, W, H, 8)
        st = ses.stats().as_dict()
        assert st["traceLaunches"] == 3
        assert st["cameraSamples"] + st["culledSamples"] == 6 * W * H * 8 and st["pixels"] == 6 * W * H
        for i in (0, 1):
            want, _ = single(gpu_lib, ses, cams[i], W, H, 8)
            assert np.array_equal(bits(got[i]), bits(want)), i
    finally:
        destroy(gpu_lib, cams[:4])


@pytest.mark.gpu
def test_one_view_and_interleaving(gpu_lib, sessions):
    from raylib_amd import binding
    ses = sessions["cornell"]
    lib = gpu_lib
    cams = view_set(lib, W / H)
    try:
        got = ses.render_views(cams[1:2], W, H, 4)
        want, _ = single(lib, ses, cams[1], W, H, 4)
        assert np.array_equal(bits(got[0]), bits(want))
        # single -> batch containing that camera -> single -> batch with one camera moved
        a, _ = single(lib, ses, cams[0], W, H, 4)
        b = ses.render_views(cams, W, H, 4)
        c, _ = single(lib, ses, cams[0], W, H, 4)
        assert np.array_equal(bits(a), bits(b[0])) and np.array_equal(bits(a), bits(c))
        lib.Raylib_CameraSetPosition(cams[0], 0.0, 1.0, 9.0)
        b2 = ses.render_views(cams, W, H, 4)
        moved, _ = single(lib, ses, cams[0], W, H, 4)
        assert np.array_equal(bits(b2[0]), bits(moved)) and not np.array_equal(bits(b2[0]), bits(a))
        for i in (1, 2, 3):
            assert np.array_equal(bits(b2[i]), bits(b[i])), i
        # with a progressive session open
        img = lib.Raylib_CreateImage(W, H)
        st = ses.settings(W, H, 4)
        h = lib.RaylibAMD_BeginProgressive(C.byref(st), ses.scene, cams[1], img, None)
        assert h
        assert lib.RaylibAMD_ProgressiveStep(h, 2) >= 0
        b3 = ses.render_views(cams, W, H, 4)
        assert lib.RaylibAMD_ProgressiveStep(h, 2) == 0
        prog = np.zeros((H, W, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, _fp(prog))
        assert np.array_equal(bits(prog), bits(b3[1]))   # (threshold 0: the session's frame is the one-shot frame)
        assert lib.RaylibAMD_EndProgressive(h) == 1
        lib.Raylib_DestroyImage(img)
        assert np.array_equal(bits(b3[0]), bits(moved))
    finally:
        destroy(lib, cams)


@pytest.mark.gpu
def test_device_output_is_view_major(gpu_lib, sessions):
    """RaylibAMD_RenderViewsDevice into device memory of the caller's (the HIP runtime's own allocation, read back with a plain hipMemcpy: the call is
    synchronous): view v's row-major frame at v * W * H."""
    from raylib_amd import binding
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]; hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    ses = sessions["cutout_sky"]
    cams = view_set(gpu_lib, W / H)
    n = len(cams)
    dev = C.c_void_p()
    try:
        st = ses.settings(W, H, 2)
        assert hip.hipMalloc(C.byref(dev), n * W * H * 16) == 0 and hip.hipMemset(dev, 0xff, n * W * H * 16) == 0
        assert gpu_lib.RaylibAMD_RenderViewsDevice(C.byref(st), ses.scene, binding.handle_array(cams), n, dev) == 1
        got = np.zeros((n, H, W, 4), np.float32)
        assert hip.hipMemcpy(got.ctypes.data, dev, n * W * H * 16, 2) == 0
        want = ses.render_views(cams, W, H, 2)
        assert np.array_equal(bits(got), bits(want))
        assert gpu_lib.RaylibAMD_RenderViewsDevice(C.byref(st), ses.scene, binding.handle_array(cams), n, None) == 1
    finally:
        if dev.value:
            hip.hipFree(dev)
        destroy(gpu_lib, cams)


@pytest.mark.gpu
def test_refusals_leave_every_image_alone(gpu_lib, sessions):
    from raylib_amd import binding
    lib = gpu_lib
    ses = sessions["cornell"]
    cams = view_set(lib, W / H)[:2]
    imgs = [lib.Raylib_CreateImage(W, H) for _ in range(2)]
    try:
        st = ses.settings(W, H, 2)
        ca, ia = binding.handle_array(cams), binding.handle_array(imgs)
        assert lib.RaylibAMD_RenderViews(C.byref(st), ses.scene, ca, 2, ia) == 1
        before = []
        for ih in imgs:
            px = np.zeros((H, W, 4), np.float32); lib.RaylibAMD_DumpImageRGBA(ih, _fp(px)); before.append(px)
        unfinalized = lib.Raylib_CreateScene()
        bad = [(C.byref(st), ses.scene, ca, 0, ia), (C.byref(st), ses.scene, ca, 65, ia), (C.byref(st), unfinalized, ca, 2, ia),
               (C.byref(st), ses.scene, binding.handle_array([cams[0], 0]), 2, ia), (C.byref(st), ses.scene, ca, 2, binding.handle_array([imgs[0], imgs[0]])),
               (C.byref(ses.settings(0, H, 2)), ses.scene, ca, 2, ia), (C.byref(ses.settings(W, H, 2, mode=99)), ses.scene, ca, 2, ia),
               (C.byref(st), ses.scene, ca, 2, binding.handle_array([imgs[0], 4242]))]
        for args in bad:
            assert lib.RaylibAMD_RenderViews(*args) == 0
            for ih, px in zip(imgs, before):
                now = np.zeros((H, W, 4), np.float32); lib.RaylibAMD_DumpImageRGBA(ih, _fp(now))
                assert np.array_equal(bits(now), bits(px))
        lib.Raylib_DestroyScene(unfinalized)
    finally:
        destroy(lib, cams)
        for ih in imgs:
            lib.Raylib_DestroyImage(ih)


@pytest.mark.gpu
def test_stereo_pair_full_hd(gpu_lib, config2_scene):
    from raylib_amd import binding
    ses, _, _ = config2_scene
    eye = binding.create_camera(gpu_lib, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 45.0, 1.0)
    exp = np.zeros(19, np.float32)
    gpu_lib.RaylibAMD_CameraExport(ses.camera, _fp(exp))
    o = exp[0:3]
    right = exp[13:16]   # the camera's u axis
    cams = []
    try:
        for s in (-0.03, 0.03):
            c = gpu_lib.Raylib_CreateCamera()
            gpu_lib.Raylib_CameraCopy(ses.camera, c)
            p = o + s * right
            gpu_lib.Raylib_CameraSetPosition(c, float(p[0]), float(p[1]), float(p[2]))
            cams.append(c)
        got = ses.render_views(cams, 1920, 1080, 8)
        for i, c in enumerate(cams):
            want, _ = single(gpu_lib, ses, c, 1920, 1080, 8)
            assert np.array_equal(bits(got[i]), bits(want)), i
    finally:
        destroy(gpu_lib, cams + [eye])
