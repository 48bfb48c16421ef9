"""Progressive rendering on the device (include/raylib_amd.h RaylibAMD_BeginProgressive).

P1: after any sequence of passes that brings a cell to n samples, its pixels are those of Raylib_Render at samplesPerPixel = n, bit for bit, under every
    schedule (leaf-list plain and general, k_trace on the tree, the pool kernel on the 4-wide and 8-wide trees), with a sun, a sky and culled cells.
P2: a uniform session ends with the one-shot frame at the cap, whatever the pass split, and whatever else happens between passes.
P3: an adaptive session ends with a mosaic of one-shot frames; the device's stop set is the host rule's on the exported sums; the samples add up.
Refusals leave the image's bits alone; the quality test compares adaptive and uniform passes at the same traced samples."""
import ctypes as C

import numpy as np
import pytest

import helpers
from helpers import bits

pytestmark = pytest.mark.gpu

W, H = 44, 36          # partial cells on the right and at the bottom
BIG = (1445, 723)      # 16 471 cells: three trips of the compaction kernel
STEPS = (1, 2, 5, 8, 48)


def _binding():
    from raylib_amd import binding
    return binding


def _frame_samples(st):
    return st.cameraSamples + st.culledSamples


def _check_uniform_previews(ses, w, h, cap=64, steps=STEPS, what=""):
    P = _binding().Progressive(ses, w, h, cap)
    assert P.handle, what
    n = 0
    try:
        for k in steps:
            live = P.step(k)
            got = P.frame()
            st = ses.stats()
            k = min(k, cap - n)
            n += k
            assert live == (0 if n >= cap else (w // 8 + (w % 8 > 0)) * (h // 8 + (h % 8 > 0))), (what, n, live)
            assert _frame_samples(st) == w * h * k, (what, n)
            want = ses.render(w, h, n)
            assert np.array_equal(bits(got), bits(want)), (what, n, int((bits(got) != bits(want)).any(-1).sum()))
        return st
    finally:
        P.close()


def test_p1_leaf_list_plain_and_general(gpu_lib, sessions, workdir):
    _check_uniform_previews(sessions["cornell"], W, H, what="cornell")
    assert gpu_lib.RaylibAMD_LastTracePlain() == 1          # the plain instance ran the passes
    _check_uniform_previews(sessions["cutout_sky"], W, H, what="cutout_sky")   # textures, cut-outs, sky, sun
    assert gpu_lib.RaylibAMD_LastTracePlain() == 0
    _check_uniform_previews(sessions["cornell_glass_sun"], W, H, what="cornell_glass_sun")   # lens, shutter, glass, sun
    # the same scene from far away: cells outside the silhouette, whose samples the resolve sums from the sky texels and the sun
    far = helpers.session_for_case(gpu_lib, "cutout_sky", workdir)
    gpu_lib.Raylib_CameraSetPosition(far.camera, 0.0, 1.0, 12.0)
    st = _check_uniform_previews(far, W, H, what="cutout_sky far")
    far.close()
    assert st.culledCells > 0 and st.culledSamples > 0 and st.listedCells > 0


def test_p1_tree_and_pool_schedules(gpu_lib, mid_scene, monkeypatch):
    ses = mid_scene[0]
    for env, width in ((dict(), 4), (dict(RAYLIB_BVH8="1"), 8), (dict(RAYLIB_POOL="0"), None)):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        st = _check_uniform_previews(ses, 48, 32, what=str(env))
        if width:
            assert st.pathsPerWave > 64 and st.treeWidth == width, env   # the pool schedule on that tree
        else:
            assert st.pathsPerWave == 64 and st.treeWidth > 0, env       # k_trace on the tree
        assert st.culledCells > 0, env
        for k in env:
            monkeypatch.delenv(k)


def test_p2_pass_splits_give_the_one_shot_frame(gpu_lib, sessions, monkeypatch):
    ses = sessions["cornell"]
    want = bits(ses.render(W, H, 64))
    splits = [(3, 12, 49), (1,) * 8 + (56,), (64,), (10, 100)]
    for split in splits:
        P = _binding().Progressive(ses, W, H, 64)
        for k in split:
            r = P.step(k)
        assert r == 0 and P.step(1) == 0
        assert np.array_equal(bits(P.frame()), want), split
        P.close()
    monkeypatch.setenv("RAYLIB_SAMPLE_BATCH", "3")     # passes that straddle the internal batches
    for split in [(5, 7, 52), (2, 1, 61)]:
        P = _binding().Progressive(ses, W, H, 64)
        for k in split:
            P.step(k)
        assert np.array_equal(bits(P.frame()), want), ("batch 3", split)
        assert ses.stats().traceLaunches == -(-split[-1] // 3)
        P.close()


def test_p2_interleaved_renders_and_post_process(gpu_lib, sessions):
    ses, other = sessions["cornell"], sessions["cutout_sky"]
    want = bits(ses.render(W, H, 32))
    P = _binding().Progressive(ses, W, H, 32)
    Q = _binding().Progressive(other, 24, 16, 8)             # a second session open at the same time
    P.step(4)
    other.render(40, 24, 3)                                  # another scene's render
    Q.step(8)
    gpu_lib.Raylib_PostProcess(P.image)                      # the session's own image post-processed between passes
    P.step(10)
    gpu_lib.Raylib_Render(C.byref(other.settings(W, H, 2)), other.scene, other.camera, P.image)   # ... and rendered into
    assert P.step(100) == 0
    assert np.array_equal(bits(P.frame()), want)
    assert np.array_equal(bits(Q.frame()), bits(other.render(24, 16, 8)))
    P.close(); Q.close()
    assert gpu_lib.RaylibAMD_ProgressiveStep(P.handle or 1, 1) == -1


def _cell_px(w, h):
    cy, cx = (h + 7) // 8, (w + 7) // 8
    px = np.zeros((cy, cx), np.int64)
    for j in range(cy):
        for i in range(cx):
            px[j, i] = min(8, w - 8 * i) * min(8, h - 8 * j)
    return px


def _cell_errors(n, s1, s2):
    """the rule's per-cell error (NumPy, as tests/test_progressive_host.py)"""
    h, w = s1.shape
    n_px = np.repeat(np.repeat(n, 8, 0), 8, 1)[:h, :w].astype(np.float32)
    with np.errstate(all="ignore"):
        v = np.maximum(np.float32(0), (s2 - s1 * s1 / n_px) / (n_px - np.float32(1)))
        se = np.sqrt(v / n_px).astype(np.float32)
    se = np.where(np.isfinite(se), se, np.float32(np.inf))
    pad = np.zeros((n.shape[0] * 8, n.shape[1] * 8), np.float32)
    pad[:h, :w] = se
    return pad.reshape(n.shape[0], 8, n.shape[1], 8).max(axis=(1, 3))


def _threshold_between(ses, w, h, n, quantile):
    """a threshold that the cells' errors after n uniform samples straddle"""
    P = _binding().Progressive(ses, w, h, n)
    P.step(n)
    cn, _, s1, s2 = P.export()
    P.close()
    e = _cell_errors(cn, s1, s2)
    return float(np.quantile(e[np.isfinite(e) & (e > 0)], quantile))   # (cells outside the silhouette have error 0)


def _run_adaptive(lib, ses, w, h, cap, threshold, min_samples, step, passes=None):
    """passes: a list that receives (samples so far, live cells, traced samples, culled samples) of every pass"""
    binding = _binding()
    P = binding.Progressive(ses, w, h, cap, threshold=threshold, min_samples=min_samples)
    assert P.handle
    total, traced, n = 0, 0, 0
    px = _cell_px(w, h)
    was_live = np.ones(px.shape, bool)
    while True:
        live = P.step(step)
        assert live >= 0
        st = ses.stats()
        total += _frame_samples(st); traced += st.cameraSamples
        # the pass sampled exactly the cells that were live before it: the job list and the culled pixel count are the compaction's of the pass before
        assert _frame_samples(st) == int(px[was_live].sum()) * (min(cap, n + step) - n), (n, _frame_samples(st))
        n = min(cap, n + step)
        cn, stopped, s1, s2 = P.export()
        was_live = ~stopped
        if passes is not None:
            passes.append((n, live, int(st.cameraSamples), int(st.culledSamples)))
        # the device's stop set is the host rule's on the exported sums, after every pass
        assert np.array_equal(stopped, binding.progressive_decide_host(lib, w, h, cn, s1, s2, threshold, min_samples)), n
        assert (cn[~stopped] == n).all() and (cn[stopped] <= n).all()
        assert live == (0 if n >= cap else int((~stopped).sum())), (n, live)
        if live == 0:
            break
    # the samples add up: every pass's traced and culled samples are the live cells' valid pixels times the pass
    assert total == int((px * cn).sum())
    frame = P.frame()
    P.close()
    return frame, cn, stopped, traced


def _splitting_threshold(ses, w, h):
    """a threshold that splits the cells: per cell the smallest error a uniform session shows at 4, 8, ... 20 samples; below the median of those the cell
    stops before 24, at or above it the cell reaches the cap (the adaptive session's sums are the uniform one's until the cell stops)"""
    U = _binding().Progressive(ses, w, h, 24)
    m = None
    for n in range(4, 24, 4):
        U.step(4)
        cn, _, s1, s2 = U.export()
        e = _cell_errors(cn, s1, s2)
        m = e if m is None else np.minimum(m, e)
    U.close()
    return float(np.median(m[np.isfinite(m) & (m > 0)]))


def _check_mosaic(ses, frame, cn, w, h, what):
    """every cell is the one-shot frame at its own count"""
    for n in np.unique(cn):
        want = ses.render(w, h, int(n))
        mask = np.repeat(np.repeat(cn == n, 8, 0), 8, 1)[:h, :w]
        assert np.array_equal(bits(frame)[mask], bits(want)[mask]), (what, n)


@pytest.mark.parametrize("scene", ["cornell", "mid"])
def test_p3_adaptive_mosaic(gpu_lib, sessions, mid_scene, scene):
    ses = sessions["cornell"] if scene == "cornell" else mid_scene[0]
    w, h = (W, H) if scene == "cornell" else (48, 32)
    t = _splitting_threshold(ses, w, h)
    frame, cn, stopped, _ = _run_adaptive(gpu_lib, ses, w, h, 24, t, 4, 4)
    assert stopped.any() and (cn < 24).any() and (cn == 24).any(), np.unique(cn)   # some but not all cells stopped early
    _check_mosaic(ses, frame, cn, w, h, scene)
    # threshold 0 is the uniform session
    P = _binding().Progressive(ses, w, h, 12, threshold=0.0, min_samples=2)
    Q = _binding().Progressive(ses, w, h, 12)
    for k in (5, 7):
        P.step(k); Q.step(k)
    assert np.array_equal(bits(P.frame()), bits(Q.frame())) and np.array_equal(bits(P.frame()), bits(ses.render(w, h, 12)))
    P.close(); Q.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("scene", ["cornell", "cutout_sky"])
def test_p3_sessions_of_three_compaction_trips(gpu_lib, workdir, scene):
    """1445 x 723 is 181 x 91 = 16 471 cells, ragged on the right and at the bottom: k_progressive_compact (8192 entries per trip) takes three trips over a
    session's lists, and the offsets it carries from trip to trip decide which cells the next pass renders.  From z = 12 most cells lie outside the silhouette.
    cornell: those cells have error 0 and leave at the first decision, the first trip's entries vanish at once.  cutout_sky: they sample the panorama; where it
    varies they keep an error and stay live, so the culled pixel count of the compaction is used pass after pass (measured: 13 635 cells of flat sky leave at the
    first decision, 2836 cells go on)."""
    w, h = BIG
    px = _cell_px(w, h)
    ses = helpers.session_for_case(gpu_lib, scene, workdir)
    gpu_lib.Raylib_CameraSetPosition(ses.camera, 0.0, 1.0, 12.0)
    try:
        st = _check_uniform_previews(ses, w, h, cap=6, steps=(1, 2, 3), what=scene + " far")
        assert 0 < st.culledCells < px.size and st.listedCells > 0, (st.culledCells, st.listedCells)   # cells outside the silhouette, and inside
        t = _splitting_threshold(ses, w, h)
        passes = []
        frame, cn, stopped, _ = _run_adaptive(gpu_lib, ses, w, h, 24, t, 4, 4, passes)
        print("\nprogressive %s %dx%d (%d cells, %d culled): threshold %.6g, cells by samples %s, passes (samples, live, traced, culled) %s"
              % (scene, w, h, px.size, st.culledCells, t, dict(zip(*[a.tolist() for a in np.unique(cn, return_counts=True)])), passes))
        assert (cn == 4).any() and (cn < 24).any() and (cn == 24).any(), np.unique(cn)   # cells that stopped at the first decision, early, and at the cap
        assert len(passes) == 6 and (cn.reshape(-1)[8192:] > 4).any()                    # cells of the later trips survive the first, three-trip compaction
        if scene == "cornell":
            assert (cn == 4).sum() >= st.culledCells and all(p[3] == 0 for p in passes[1:])   # every cell outside the silhouette left at once
        else:
            assert all(p[3] > 0 for p in passes)                                         # culled samples in every pass: the compaction's pixel count at work
        _check_mosaic(ses, frame, cn, w, h, scene + " far")
    finally:
        ses.close()


def test_refusals_leave_the_image_alone(gpu_lib, sessions, workdir):
    binding = _binding()
    lib = gpu_lib
    ses = sessions["cornell"]
    img = lib.Raylib_CreateImage(W, H)
    aov = ses.settings(W, H, 4, mode=binding.RENDERMODE_SURFACE_NORMAL)
    assert lib.RaylibAMD_BeginProgressive(C.byref(aov), ses.scene, ses.camera, img, None) == 0
    lib.Raylib_DestroyImage(img)

    def dump(P):
        return bits(P.frame()).copy()

    # a scene changed under the session (the sun is set again: the device copy is released and uploaded anew)
    own = helpers.session_for_case(lib, "cornell", workdir)
    P = binding.Progressive(own, W, H, 16)
    assert P.step(4) > 0
    before = dump(P)
    lib.Raylib_SetSunIlluminance(own.scene, 0.0, 0.0, 0.0)
    assert P.step(4) == -1 and np.array_equal(dump(P), before)
    P.close(); own.close()
    # a sky panorama replaced, and one whose pixels changed
    own = helpers.session_for_case(lib, "cutout_sky", workdir)
    P = binding.Progressive(own, W, H, 16)
    assert P.step(2) > 0
    before = dump(P)
    sky = np.ascontiguousarray(helpers.scenes.sky_panorama()[::-1], np.float32)
    ih = lib.RaylibAMD_CreateImageFromData(sky.shape[1], sky.shape[0], binding._fp(sky))
    lib.Raylib_SetSkyPanorama(own.scene, ih)
    assert P.step(2) == -1 and np.array_equal(dump(P), before)
    lib.Raylib_SetSkyPanorama(own.scene, own._images[-1])
    assert P.step(2) > 0                                     # the panorama it began with: on it goes
    lib.Raylib_Render(C.byref(own.settings(8, 8, 1)), own.scene, own.camera, own._images[-1])   # that image's pixels replaced
    before = dump(P)
    assert P.step(2) == -1 and np.array_equal(dump(P), before)
    P.close(); lib.Raylib_DestroyImage(ih); own.close()
    # the image resized under the session
    P = binding.Progressive(ses, W, H, 16)
    assert P.step(2) > 0
    lib.Raylib_Render(C.byref(ses.settings(W + 8, H, 1)), ses.scene, ses.camera, P.image)
    resized = np.zeros((H, W + 8, 4), np.float32)
    lib.RaylibAMD_DumpImageRGBA(P.image, binding._fp(resized))
    assert P.step(2) == -1
    again = np.zeros_like(resized)
    lib.RaylibAMD_DumpImageRGBA(P.image, binding._fp(again))
    assert np.array_equal(bits(again), bits(resized))
    # an ended session
    h = P.handle
    P.close()
    assert lib.RaylibAMD_ProgressiveStep(h, 2) == -1 and lib.RaylibAMD_EndProgressive(h) == 0


def _y(img):
    L = img[..., 0] * 0.2126 + img[..., 1] * 0.7152 + img[..., 2] * 0.0722
    return L / (1.0 + L)


@pytest.mark.parametrize("scene", ["cornell", "mid"])
def test_quality_adaptive_against_uniform_at_equal_traced_samples(gpu_lib, sessions, mid_scene, scene):
    """MSE in y against a 1024-spp frame, adaptive passes (threshold: the median cell error after 16 samples, halved) against one uniform frame with at
    least as many traced samples.  Numbers: DESIGN.md section 2."""
    ses = sessions["cornell"] if scene == "cornell" else mid_scene[0]
    w, h = (256, 256) if scene == "cornell" else (256, 170)
    ref = _y(ses.render(w, h, 1024).astype(np.float64))
    t = 0.5 * _threshold_between(ses, w, h, 16, 0.5)
    frame, cn, stopped, traced = _run_adaptive(gpu_lib, ses, w, h, 256, t, 16, 16)
    one = ses.render(w, h, 1)
    per_spp = ses.stats().cameraSamples                      # traced samples of one uniform sample per pixel (culled cells are not traced)
    spp = -(-traced // per_spp)
    uni = ses.render(w, h, spp)
    mse_a = float(((_y(frame.astype(np.float64)) - ref) ** 2).mean())
    mse_u = float(((_y(uni.astype(np.float64)) - ref) ** 2).mean())
    print("\nprogressive quality %s %dx%d: threshold %.6g, traced %d (uniform %d spp = %d), cells stopped %d of %d, counts %s; MSE(y) adaptive %.4e uniform %.4e ratio %.3f"
          % (scene, w, h, t, traced, spp, spp * per_spp, int(stopped.sum()), stopped.size, np.unique(cn).tolist(), mse_a, mse_u, mse_a / mse_u))
    # measured: Cornell 0.897 -- adaptive wins; the room from outside 1.023 -- it does not; the bounds keep those results
    bound = {"cornell": 0.95, "mid": 1.05}[scene]
    assert one is not None and mse_a <= bound * mse_u, (mse_a, mse_u)
