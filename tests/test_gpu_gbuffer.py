"""The primary-hit G-buffer on the device (include/raylib_amd.h, statements G1 to G6; csrc/rl_k_gbuffer.inl).  Every comparison is bit for bit.

The oracles are existing code: the colour planes against Raylib_Render in the five deterministic debug modes, the hit and surface planes against
RaylibAMD_TraceRays on the camera rays RaylibAMD_EvalCameraRays gives.  The precondition of the second comparison: every surface of these scenes is at least 1e-2
from the camera, so the render's rule for rayTMin (statement G2) and the queries' agree on every pixel; the test asserts the distance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch    # before the library is loaded: the device entry is handed torch's tensors

import helpers
import move_cases as mc
import radiance_cases
from raylib_amd import binding

pytestmark = pytest.mark.gpu

W, H = 37, 21                       # partial cells on both edges
TMIN = 1e-4
COLOUR = {"albedo": binding.RENDERMODE_ALBEDO, "surfaceNormal": binding.RENDERMODE_SURFACE_NORMAL, "microNormal": binding.RENDERMODE_MICROSURFACE_NORMAL,
          "texcoord": binding.RENDERMODE_TEXCOORD, "emission": binding.RENDERMODE_EMISSION}
NAMES = list(helpers.CASES) + ["procedural", "cornell_tess4"]
STILL = [n for n in NAMES if n != "procedural"] + ["procedural_still"]      # the cases without a moving cube
TREES = [None, 2, 4, 8]
WORDS = {k: 11 if k == "surface" else 4 for k in binding.GBUFFER_PLANES}


def _procedural(lib, shutter=None):
    mats, sph, cub, cam = helpers.procedural_case()
    return binding.ProceduralSession(lib, mats, sph, cub, origin=cam["origin"], look_at=cam["look_at"], fov=cam["fov"], aspect=cam["aspect"], sun=cam["sun"],
                                     sun_dir=cam["sun_dir"], aperture=cam["aperture"], focal=cam["focal"], shutter=cam["shutter"] if shutter is None else shutter)


@pytest.fixture(scope="module")
def cases(gpu_lib, sessions, workdir):
    d = os.path.join(str(workdir), "gbuffer"); os.makedirs(d, exist_ok=True)
    own = {"procedural": _procedural(gpu_lib), "procedural_still": _procedural(gpu_lib, (0.0, 0.0)),
           "cornell_tess4": binding.SceneSession(gpu_lib, helpers.scenes.cornell(os.path.join(d, "c4.obj"), tess=4)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)}
    t4 = own["cornell_tess4"]
    n4, n8 = C.c_uint32(), C.c_uint32()
    assert gpu_lib.RaylibAMD_SceneNumTriangles(t4.scene) > 108
    assert gpu_lib.RaylibAMD_SceneBVH4Info(t4.scene, C.byref(n4), C.byref(C.c_uint32())) == 1 and n4.value > 0
    assert gpu_lib.RaylibAMD_SceneBVH8Info(t4.scene, C.byref(n8), C.byref(C.c_uint32()), C.byref(C.c_float()), C.byref(C.c_float())) == 1 and n8.value > 0
    yield dict(sessions, **own)
    for s in own.values():
        s.close()


def _tree(monkeypatch, tree):
    if tree is None:
        monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    else:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))


def gbuffer(lib, ses, w=W, h=H, planes=binding.GBUFFER_PLANES):
    return binding.gbuffer(lib, ses.scene, ses.camera, w, h, TMIN, planes)


_AOV = {}


def aov(name, ses, w=W, h=H, seed=1):
    """Raylib_Render + the RGBA dump in modes 1 to 5, once per (case, frame, seed)"""
    key = (name, w, h, seed)
    if key not in _AOV:
        _AOV[key] = {k: ses.render(w, h, 1, 5, TMIN, mode) for k, mode in COLOUR.items()}
    return _AOV[key]


def camera_query_rays(lib, ses, w, h, seed=1):
    ys, xs = np.mgrid[0:h, 0:w]
    uv = np.stack([np.float32(xs.ravel()) / np.float32(w), np.float32(ys.ravel()) / np.float32(h)], 1).astype(np.float32)
    r = radiance_cases.camera_rays(lib, ses.camera, uv, seed)
    return helpers.rays8(r[:, 0:3], r[:, 3:6], tmin=TMIN, tmax=helpers.F32_MAX)


def assert_colour(got, want, what):
    for k in COLOUR:
        assert got[k].shape == want[k].shape and np.array_equal(helpers.bits(got[k]), helpers.bits(want[k])), \
            "%s: plane %s differs from the AOV render in %d pixels" % (what, k, (helpers.bits(got[k]) != helpers.bits(want[k])).any(-1).sum())
        assert (got[k][..., 3] == 1.0).all(), (what, k)


def assert_queries(lib, ses, got, w, h, what):
    rays = camera_query_rays(lib, ses, w, h)
    closest = binding.trace_rays(lib, ses.scene, rays, binding.QUERY_CLOSEST, 0.0)
    surface, prim = binding.trace_rays(lib, ses.scene, rays, binding.QUERY_SURFACE, 0.0, with_prim=True)
    hit = closest["prim"] >= 0
    assert not hit.any() or closest["t"][hit].min() >= 1e-2, "%s: a surface within 1e-2 of the camera: the precondition of this comparison" % what
    assert got["hit"].reshape(-1).tobytes() == closest.tobytes(), what
    assert got["surface"].reshape(-1).tobytes() == surface.tobytes(), what
    assert np.array_equal(got["hit"]["prim"].reshape(-1), prim), what
    return hit


# ---- 1. the colour planes against the AOV renders ----
@pytest.mark.parametrize("name", NAMES)
def test_colour_planes_are_the_debug_modes(gpu_lib, cases, monkeypatch, name):
    _tree(monkeypatch, None)
    ses = cases[name]
    want = aov(name, ses)
    got = gbuffer(gpu_lib, ses)
    assert_colour(got, want, name)
    st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.cameraSamples == st.pixels == W * H and st.ranks == 1 and st.rays >= W * H and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    assert st.nodesVisited > 0 and st.trisTested > 0 and st.shadedHits > 0, st.as_dict()
    rc, plan = binding.plan_gbuffer(gpu_lib, ses.scene)
    assert rc == 1 and (st.treeWidth, st.nodeBytes) == (plan["treeWidth"], plan["nodeBytes"]), (st.as_dict(), plan)
    assert any((want[k][..., :3] != 0).any() for k in COLOUR)          # the oracle is not a blank frame


@pytest.mark.parametrize("tree", [2, 4, 8])
def test_colour_planes_on_each_tree(gpu_lib, cases, monkeypatch, tree):
    ses = cases["cornell_tess4"]
    want = aov("cornell_tess4", ses)
    _tree(monkeypatch, tree)
    got = gbuffer(gpu_lib, ses)
    st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.treeWidth == tree, st.as_dict()
    assert_colour(got, want, "tree %d" % tree)


def test_mirror_follow_ups_are_counted(gpu_lib, cases, monkeypatch):
    """The albedo plane's second walk runs for mirror-like surfaces and only when the plane is asked for: more rays than pixels with it, exactly the pixels without."""
    _tree(monkeypatch, None)
    ses = cases["pbr_maps"]
    st = binding.Stats()
    gbuffer(gpu_lib, ses, planes=("albedo",)); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.rays > W * H
    gbuffer(gpu_lib, ses, planes=("hit", "surface", "surfaceNormal", "microNormal", "texcoord", "emission")); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.rays == W * H


# ---- 2. the hit and surface planes against the ray queries ----
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", STILL)
def test_hit_and_surface_planes_are_the_ray_queries(gpu_lib, cases, monkeypatch, name, tree):
    _tree(monkeypatch, tree)
    ses = cases[name]
    got = gbuffer(gpu_lib, ses, planes=("hit", "surface"))
    hit = assert_queries(gpu_lib, ses, got, W, H, "%s on tree %s" % (name, tree))
    assert hit.sum() > 50
    if name == "procedural_still":
        kinds = set((got["hit"]["prim"][got["hit"]["prim"] >= 0] >> 28).tolist())
        assert kinds == {1, 2}, kinds            # spheres and cubes, numbered as the queries number them


# ---- 3. subsets ----
def test_each_plane_alone(gpu_lib, cases, monkeypatch):
    _tree(monkeypatch, None)
    for name in ("pbr_maps", "procedural"):
        ses = cases[name]
        whole = gbuffer(gpu_lib, ses)
        for k in binding.GBUFFER_PLANES:
            alone = gbuffer(gpu_lib, ses, planes=(k,))
            assert list(alone) == [k] and alone[k].tobytes() == whole[k].tobytes(), (name, k)


def _guarded(names, w, h, guard=64):
    """Per plane a sentinel-filled tensor of the plane's words and `guard` more, and its leading part as the plane"""
    big = {k: torch.full((w * h * WORDS[k] + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for k in names}
    out = {k: (v[:w * h * WORDS[k]].view(h, w, WORDS[k]) if k in ("hit", "surface") else v[:w * h * 4].view(h, w, 4).view(torch.float32)) for k, v in big.items()}
    torch.cuda.synchronize()        # the fills ran on torch's default stream; the calls run on others
    return big, out


def test_nothing_is_stored_past_a_plane_or_into_one_not_asked_for(gpu_lib, cases, monkeypatch):
    _tree(monkeypatch, None)
    ses = cases["pbr_maps"]
    whole = gbuffer(gpu_lib, ses)
    for asked in (binding.GBUFFER_PLANES, ("hit", "microNormal"), ("surface",)):
        big, out = _guarded(binding.GBUFFER_PLANES, W, H)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            binding.gbuffer_device(gpu_lib, ses.scene, ses.camera, W, H, TMIN, asked, out={k: out[k] for k in asked})
        s.synchronize()
        for k in binding.GBUFFER_PLANES:
            words = big[k].cpu().numpy()
            n = W * H * WORDS[k]
            assert (words[n:] == 0x5A5A5A5A).all(), (asked, k)
            if k in asked:
                assert words[:n].tobytes() == whole[k].tobytes(), (asked, k)
            else:
                assert (words[:n] == 0x5A5A5A5A).all(), (asked, k)


# ---- 4. sizes ----
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (64, 64)])
def test_sizes(gpu_lib, cases, monkeypatch, size):
    _tree(monkeypatch, None)
    w, h = size
    ses = cases["cornell"]
    got = gbuffer(gpu_lib, ses, w, h)
    assert_colour(got, aov("cornell", ses, w, h), "%d x %d" % size)
    assert_queries(gpu_lib, ses, got, w, h, "%d x %d" % size)


# ---- 5. the device entry ----
def _stats(lib):
    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
    return bytes(st)


def test_device_entry(gpu_lib, cases, monkeypatch):
    _tree(monkeypatch, None)
    lib, ses = gpu_lib, cases["cutout_sky"]
    whole = gbuffer(lib, ses)
    ses.render(16, 16, 1)                         # the last call's numbers are now a render's
    before = _stats(lib)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        on_stream = binding.gbuffer_device(lib, ses.scene, ses.camera, W, H, TMIN)
    s.synchronize()
    assert _stats(lib) == before, "a call on a caller's stream leaves the stats alone"
    on_null = binding.gbuffer_device(lib, ses.scene, ses.camera, W, H, TMIN)       # torch's default stream: handle 0, the library's stream, synchronous
    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.cameraSamples == st.pixels == W * H and st.ranks == 1 and st.rays >= W * H and st.kernelMs > 0, st.as_dict()
    for got in (on_stream, on_null):
        for k in binding.GBUFFER_PLANES:
            assert got[k].cpu().numpy().tobytes() == whole[k].tobytes(), k


def test_device_entry_refusals(gpu_lib, cases):
    lib, ses = gpu_lib, cases["cornell"]
    st = binding.RendererSettings(W, H, 1, 1, TMIN, 0)
    big, out = _guarded(("hit", "surface", "albedo"), W, H)
    host = np.full(W * H * 4, 0x5A5A5A5A, np.int32)
    tries = {"a host pointer": binding.GBufferPlanes(hit=out["hit"].data_ptr(), albedo=host.ctypes.data),
             "hit off by 4 bytes": binding.GBufferPlanes(hit=out["hit"].data_ptr() + 4),
             "a colour plane off by 8 bytes": binding.GBufferPlanes(albedo=out["albedo"].data_ptr() + 8),
             "surface off by 2 bytes": binding.GBufferPlanes(surface=out["surface"].data_ptr() + 2, hit=out["hit"].data_ptr())}
    stream = torch.cuda.Stream()
    for what, planes in tries.items():
        for handle in (None, C.c_void_p(stream.cuda_stream)):
            assert lib.RaylibAMD_RenderGBufferDevice(C.byref(st), ses.scene, ses.camera, C.byref(planes), handle) == 0, what
    torch.cuda.synchronize()
    assert (host == 0x5A5A5A5A).all() and all((v.cpu().numpy() == 0x5A5A5A5A).all() for v in big.values())
    ok = binding.GBufferPlanes(surface=out["surface"].data_ptr() + 4)              # 4-byte aligned is enough for the 44-byte records
    assert lib.RaylibAMD_RenderGBufferDevice(C.byref(binding.RendererSettings(W, H - 1, 1, 1, TMIN, 0)), ses.scene, ses.camera, C.byref(ok), None) == 1


# ---- 6. behind a move on the same stream ----
def test_behind_a_move_on_the_callers_stream(gpu_lib, workdir, monkeypatch):
    _tree(monkeypatch, None)
    lib = gpu_lib
    soup = mc.soup_triangles()
    moved = soup.copy(); moved[200:400] += np.asarray((0.35, -0.2, 0.15), mc.F).astype(np.float64)
    ses = mc.soup_session(lib, workdir, "gbuffer_move_a", soup)
    fresh = mc.soup_session(lib, workdir, "gbuffer_move_b", moved.astype(mc.F).astype(np.float64))
    try:
        want = gbuffer(lib, fresh)
        before = gbuffer(lib, ses)                # (the scene and its tree are on the device before it moves)
        assert before["hit"].tobytes() != want["hit"].tobytes()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            rc, first, end = mc.move_to(lib, ses, fresh, device=True)
            got = binding.gbuffer_device(lib, ses.scene, ses.camera, W, H, TMIN)      # straight behind it, on the same stream
        s.synchronize()
        assert (rc, first, end) == (1, 200, 400)
        for k in binding.GBUFFER_PLANES:
            assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        assert (want["hit"]["prim"] >= 200).any() and (want["hit"]["prim"] < 400).any() and (want["hit"]["prim"] == -1).any()
        rc, plan = binding.plan_gbuffer(lib, ses.scene)
        assert plan["treeWidth"] == 8             # a refitted wide tree was walked
    finally:
        ses.close(); fresh.close()


# ---- 7. the denoise pipeline ----
def _image(lib, img, w, h):
    out = np.zeros((h, w, 4), np.float32)
    lib.RaylibAMD_DumpImageRGBA(img, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def test_denoise_pipeline_with_the_guides_from_one_launch(gpu_lib, cases, monkeypatch):
    """INTEGRATION.md section 3a twice: with the two AOV renders, and with RaylibAMD_RenderGuides in their place.  The same denoised bits."""
    _tree(monkeypatch, None)
    lib, ses = gpu_lib, cases["cornell"]
    w = h = 64
    lib.RaylibAMD_EnableDenoiser(1)
    images = [lib.Raylib_CreateImage(w, h) for _ in range(3)] + [lib.Raylib_CreateImage(0, 0) for _ in range(4)]
    main, a1, n1, a2, n2, out1, out2 = images
    try:
        st = ses.settings(w, h, 4, 5, TMIN)
        lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, main)
        for mode, img in ((binding.RENDERMODE_ALBEDO, a1), (binding.RENDERMODE_MICROSURFACE_NORMAL, n1)):
            dbg = ses.settings(w, h, 4, 5, TMIN, mode)
            lib.Raylib_Render(C.byref(dbg), ses.scene, ses.camera, img)
        assert lib.Raylib_Denoise(main, 1, a1, n1, out1) == 1
        assert lib.RaylibAMD_RenderGuides(C.byref(st), ses.scene, ses.camera, a2, n2) == 1          # (resizes the 0 x 0 images; spp and path length are not read)
        assert lib.Raylib_Denoise(main, 1, a2, n2, out2) == 1
        assert np.array_equal(helpers.bits(_image(lib, a2, w, h)), helpers.bits(_image(lib, a1, w, h)))
        assert np.array_equal(helpers.bits(_image(lib, n2, w, h)), helpers.bits(_image(lib, n1, w, h)))
        d1, d2 = _image(lib, out1, w, h), _image(lib, out2, w, h)
        assert np.array_equal(helpers.bits(d1), helpers.bits(d2))
        assert not np.array_equal(helpers.bits(d1), helpers.bits(_image(lib, main, w, h)))
        # one handle alone, then the refusals of the images entry
        assert lib.RaylibAMD_RenderGuides(C.byref(st), ses.scene, ses.camera, None, n2) == 1
        assert np.array_equal(helpers.bits(_image(lib, n2, w, h)), helpers.bits(_image(lib, n1, w, h)))
        assert lib.RaylibAMD_RenderGuides(C.byref(st), ses.scene, ses.camera, None, None) == 0
        assert lib.RaylibAMD_RenderGuides(C.byref(st), ses.scene, ses.camera, a2, a2) == 0
        assert np.array_equal(helpers.bits(_image(lib, a2, w, h)), helpers.bits(_image(lib, a1, w, h)))
    finally:
        lib.RaylibAMD_EnableDenoiser(0)
        for img in images:
            lib.Raylib_DestroyImage(img)


# ---- 8. the seed ----
def test_seed(gpu_lib, cases, monkeypatch):
    _tree(monkeypatch, None)
    lib, ses = gpu_lib, cases["cornell_glass_sun"]          # a thin lens: the rays depend on the pixel's stream
    got = {}
    try:
        for seed in (1, 2):
            lib.RaylibAMD_SetSeed(seed)
            got[seed] = gbuffer(lib, ses)
            assert_colour(got[seed], aov("cornell_glass_sun", ses, seed=seed), "seed %d" % seed)
            rays = camera_query_rays(lib, ses, W, H, seed)
            assert got[seed]["hit"].reshape(-1).tobytes() == binding.trace_rays(lib, ses.scene, rays, binding.QUERY_CLOSEST, 0.0).tobytes(), seed
    finally:
        lib.RaylibAMD_SetSeed(1)
    # the planes of continuous quantities differ for certain (another lens sample, another ray); a normal, an albedo or an emission is constant over a wall
    for k in ("hit", "surface", "texcoord"):
        assert got[1][k].tobytes() != got[2][k].tobytes(), k
