"""The lit-sample mask of the lazy-reflectance instance (csrc/rl_lit_mask.h): with it a sample that is all zero bits is neither stored nor flagged, and
k_resolve_lit adds a pixel's flagged samples alone.  Every frame must be the unmasked path's (RAYLIB_LIT_MASK=0: every sample stored, k_resolve) bit for bit --
NaN payloads and signs of zero included -- with the same work counters, and RaylibAMD_LastLitMask must say which of the two ran."""
import os

import numpy as np
import pytest

from helpers import scenes
from test_gpu_lazy_refl import COUNTERS, _binding
from test_lazy_refl_host import MTL, box_with

pytestmark = pytest.mark.gpu

W, H = 72, 40
INSIDE = ((0, 1, 0.9), (0, 1, -1))     # from inside the box: every cell sees the scene
OUTSIDE = ((0, 1, 4), (0, 1, -1))      # the usual view of a 9:5 frame: the cells beside the box are culled
AWAY = ((0, 1, 4), (0, 1, 9))          # the box behind the camera: no sample meets it


def aim(ses, view):
    ses.lib.Raylib_CameraSetPosition(ses.camera, *[float(x) for x in view[0]])
    ses.lib.Raylib_CameraSetLookAt(ses.camera, *[float(x) for x in view[1]])


def bits(img):
    return np.ascontiguousarray(img, np.float32).view(np.uint32)


def render_pair(ses, lib, monkeypatch, spp, max_path=5, masked=1, setting=None):
    """The frame with the mask (as `setting` of RAYLIB_LIT_MASK decides: None, not set) and with RAYLIB_LIT_MASK=0: the same bits, the same counters.
    Returns the first render's stats."""
    if setting is None:
        monkeypatch.delenv("RAYLIB_LIT_MASK", raising=False)
    else:
        monkeypatch.setenv("RAYLIB_LIT_MASK", setting)
    a = ses.render(W, H, spp, max_path=max_path)
    ran, lazy, sa = lib.RaylibAMD_LastLitMask(), lib.RaylibAMD_LastTraceLazy(), ses.stats()
    monkeypatch.setenv("RAYLIB_LIT_MASK", "0")
    b = ses.render(W, H, spp, max_path=max_path)
    off, sb = lib.RaylibAMD_LastLitMask(), ses.stats()
    monkeypatch.delenv("RAYLIB_LIT_MASK")
    assert (lazy, ran, off) == (1, masked, 0), (lazy, ran, off)
    differ = (bits(a) != bits(b)).any(-1)
    assert not differ.any(), "%d pixels differ, the first at %s" % (int(differ.sum()), np.argwhere(differ)[0])
    for k in COUNTERS + ("litPaths", "litFoldedInPlace"):
        assert getattr(sa, k) == getattr(sb, k), (k, getattr(sa, k), getattr(sb, k))
    return sa


@pytest.fixture(scope="module")
def cornell(gpu_lib, workdir):
    d = os.path.join(str(workdir), "lit_mask_gpu"); os.makedirs(d, exist_ok=True)
    ses = _binding().SceneSession(gpu_lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0], OUTSIDE[0], OUTSIDE[1], 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    yield ses
    ses.close()


@pytest.fixture(scope="module")
def bright(gpu_lib, workdir):
    """Ceiling, floor and walls all emit (the bright box of test_gpu_lazy_refl.py): nearly every sample that meets the scene is lit."""
    d = os.path.join(str(workdir), "lit_mask_gpu"); os.makedirs(d, exist_ok=True)
    mtl = MTL.replace("Ns 10\nillum 2", "Ns 10\nKe 0.5 0.25 0.125\nillum 2") % dict(kd="0.725 0.71 0.68", ks="0 0 0", ns="10", pr="Ke 0.25 0.5 1")
    obj = scenes.write_obj(os.path.join(d, "bright.obj"), scenes.cornell_objects(scenes.WHITE, scenes.WHITE), mtl)[0]
    ses = _binding().SceneSession(gpu_lib, obj, INSIDE[0], INSIDE[1], 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    yield ses
    ses.close()


# 1: the unjittered sample 0 alone; 31 | 32 | 33 and 64 | 65: either side of a word of the mask; 256 | 257: either side of the most a launch may hold
# (RL_LIT_MASK_MAX_WORDS = 8 words), beyond which the launch keeps the unmasked path
@pytest.mark.parametrize("spp", [1, 31, 32, 33, 64, 65, 256, 257])
@pytest.mark.parametrize("view", ["culled", "all cells"])
def test_sample_counts_cull_and_lit_list(gpu_lib, cornell, monkeypatch, spp, view):
    monkeypatch.setenv("RAYLIB_POOL", "0")
    aim(cornell, OUTSIDE if view == "culled" else INSIDE)
    for entries in (None, "0"):          # the default list (k_fold_lit stores and flags), and every lit path folded in place inside the megakernel
        if entries is not None:
            monkeypatch.setenv("RAYLIB_LIT_LIST", entries)
        st = render_pair(cornell, gpu_lib, monkeypatch, spp, masked=1 if spp <= 256 else 0)
        assert st.traceLaunches == 1 and st.litPaths > 0
        assert (st.culledCells > 0) == (view == "culled"), st.culledCells
        assert (st.litFoldedInPlace == st.litPaths) == (entries == "0")
    monkeypatch.delenv("RAYLIB_LIT_LIST")
    aim(cornell, OUTSIDE)


@pytest.mark.parametrize("batch", ["32", "33", "7"])
def test_several_batches(gpu_lib, cornell, monkeypatch, batch):
    """65 samples in launches of 32 + 32 + 1, 33 + 32 and 7 x 9 + 2: the mask is zeroed and sized per launch, the running sum goes through the accum buffer."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    monkeypatch.setenv("RAYLIB_SAMPLE_BATCH", batch)
    aim(cornell, OUTSIDE)
    st = render_pair(cornell, gpu_lib, monkeypatch, 65)
    assert st.traceLaunches == -(-65 // int(batch))
    one = bits(cornell.render(W, H, 65))
    monkeypatch.delenv("RAYLIB_SAMPLE_BATCH")
    assert (one == bits(cornell.render(W, H, 65))).all()


def test_path_lengths(gpu_lib, cornell, monkeypatch):
    """maxPathLength 1 (every sample that meets a light is the emission itself) and 12 (longer paths than an entry of the lit list holds fold in place)."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    aim(cornell, OUTSIDE)
    for max_path in (1, 12):
        st = render_pair(cornell, gpu_lib, monkeypatch, 8, max_path=max_path)
        assert st.litPaths > 0 and (st.litFoldedInPlace > 0) == (max_path == 12)


def test_negative_emission(gpu_lib, workdir, monkeypatch):
    """A light that takes light away, in a box whose walls emit: lit samples with negative components, sums that cancel and pass through zero."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    d = os.path.join(str(workdir), "lit_mask_gpu"); os.makedirs(d, exist_ok=True)
    mtl = MTL.replace("Ke 17 12 4", "Ke -17 12 -0.0").replace("Ns 10\nillum 2", "Ns 10\nKe 0.5 0 -0.25\nillum 2") % dict(kd="0.725 0.71 0.68", ks="0 0 0", ns="10", pr="Ke 0.25 0.5 -1")
    obj = scenes.write_obj(os.path.join(d, "negative.obj"), scenes.cornell_objects(scenes.WHITE, scenes.WHITE), mtl)[0]
    ses = _binding().SceneSession(gpu_lib, obj, OUTSIDE[0], OUTSIDE[1], 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    for view in (OUTSIDE, INSIDE):
        aim(ses, view)
        render_pair(ses, gpu_lib, monkeypatch, 33)
    img = ses.render(W, H, 33)
    assert (img[..., :3] < 0).any() and (img[..., :3] > 0).any()
    ses.close()


def test_back_to_back_frames(gpu_lib, bright, monkeypatch):
    """A bright view, then a dark one, twice through the same handle: the dark view lists every cell (RAYLIB_CULL_CELLS=0) and none of its samples meets the
    scene, so nothing is stored and nothing flagged -- a mask bit or a sample left from the bright frame would show in it."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    monkeypatch.setenv("RAYLIB_CULL_CELLS", "0")
    monkeypatch.setenv("RAYLIB_LIT_MASK", "0")
    want = {}
    for name, view in (("bright", INSIDE), ("dark", AWAY)):
        aim(bright, view)
        want[name] = bits(bright.render(W, H, 33))
        assert gpu_lib.RaylibAMD_LastLitMask() == 0 and bright.stats().culledCells == 0
    assert want["bright"][..., :3].any(-1).all() and not want["dark"][..., :3].any()
    monkeypatch.delenv("RAYLIB_LIT_MASK")
    for k in range(2):
        for name, view in (("bright", INSIDE), ("dark", AWAY)):
            aim(bright, view)
            got = bits(bright.render(W, H, 33))
            assert gpu_lib.RaylibAMD_LastLitMask() == 1
            assert (got == want[name]).all(), (k, name)
    aim(bright, INSIDE)


def test_bright_box_every_sample_lit(gpu_lib, bright, monkeypatch):
    """Nearly every sample flagged: the mask's words full; and with a list of one chunk, which overflows in mid-launch, so that k_fold_lit and the in-place
    fold both set bits of the same words."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    aim(bright, INSIDE)
    st = render_pair(bright, gpu_lib, monkeypatch, 64)
    assert st.litPaths * 2 > st.cameraSamples and st.litFoldedInPlace == 0
    monkeypatch.setenv("RAYLIB_LIT_LIST", "64")
    st = render_pair(bright, gpu_lib, monkeypatch, 64)
    assert 0 < st.litPaths - st.litFoldedInPlace <= 64


def test_sun(gpu_lib, workdir, monkeypatch):
    """With a sun most samples are lit: the planner keeps the mask off unless RAYLIB_LIT_MASK=1 asks for it; either way the frame is the unmasked one."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    d = os.path.join(str(workdir), "lit_mask_gpu"); os.makedirs(d, exist_ok=True)
    ses = _binding().SceneSession(gpu_lib, scenes.cornell(os.path.join(d, "sun.obj"))[0], (0.3, 1.2, 4), (0, 0.9, -1), 45.0, W / H, sun=(20, 20, 20), sun_dir=(0.2, -0.3, -1.0))
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    render_pair(ses, gpu_lib, monkeypatch, 33, masked=0)
    st = render_pair(ses, gpu_lib, monkeypatch, 33, masked=1, setting="1")
    assert st.litPaths > 0
    ses.close()


def test_progressive_and_views_keep_every_sample(gpu_lib, cornell, monkeypatch):
    """A progressive pass and a batch of views resolve with kernels of their own: no mask, whatever RAYLIB_LIT_MASK says."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    monkeypatch.setenv("RAYLIB_LIT_MASK", "1")
    aim(cornell, OUTSIDE)
    B = _binding()
    P = B.Progressive(cornell, 44, 36, 8)
    P.step(4)
    assert gpu_lib.RaylibAMD_LastTraceLazy() == 1 and gpu_lib.RaylibAMD_LastLitMask() == 0
    P.step(4)
    frame = P.frame()
    P.close()
    assert (bits(frame) == bits(cornell.render(44, 36, 8))).all() and gpu_lib.RaylibAMD_LastLitMask() == 1
    cam = B.create_camera(gpu_lib, OUTSIDE[0], OUTSIDE[1], 45.0, W / H)
    views = cornell.render_views([cam], W, H, 4)
    assert gpu_lib.RaylibAMD_LastLitMask() == 0
    assert (bits(views[0]) == bits(cornell.render(W, H, 4))).all()
    gpu_lib.Raylib_DestroyCamera(cam)
