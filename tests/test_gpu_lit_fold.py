"""The lit list of the lazy-reflectance kernels is folded by the waves that fill it (csrc/rl_dev_litfold.h): a wave that writes the 64th entry of its chunk
folds the chunk, entry `lane` in lane `lane`, and folds its last, partly filled chunk before it leaves; no kernel follows to finish the list.  Every frame of
the hit-queue instance (k_trace_lazy_hitq) and of the ray-queue instance (RAYLIB_HIT_QUEUE=0, k_trace_lazy) must be the eager instance's (RAYLIB_LAZY_REFL=0)
as uint32, with the same work counters -- waveTrips aside, which depends on which wave drew which batch --, the two lazy instances must count the same
litPaths, and litFoldedInPlace keeps its meaning: the lit paths that had no entry (more vertex records than an entry holds, or the list used up).  A path folded
from its entry by its own wave is not one of them.  The cases are the smallest that reach each edge of the fold."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import scenes
from test_lazy_refl_host import MTL

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "nodesVisited", "trisTested", "shadedHits", "texFetches", "cameraSamples", "culledSamples", "culledCells", "listedCells", "pixels", "traceLaunches")
W, H = 64, 48
EYE, AT = (0, 1, 4), (0, 1, -1)
INSIDE = ((0, 1, 0.9), (0, 1, -1))     # from inside the box: every cell sees the scene
KERNELS = (("hit queue", {"RAYLIB_HIT_QUEUE": "1"}, (1, 1)), ("ray queue", {"RAYLIB_HIT_QUEUE": "0"}, (1, 0)), ("eager", {"RAYLIB_LAZY_REFL": "0"}, (0, 0)))
# The most compute units a launch may spread over (an MI355X has 256, no Instinct part more than 304): with RAYLIB_BLOCKS_PER_CU=1 a launch has at most
# 4 * MAX_CUS waves, so a launch that writes more than 2 * 64 * 4 * MAX_CUS entries has a wave that filled two chunks, whichever wave drew what.
MAX_CUS = 320
# A list that holds every job of a 128-sample frame and a partly filled chunk per wave on top: the planner's own size (an entry per 32 jobs and a chunk per
# wave) runs out where most paths are lit, and the rest would fold in place
BIG_LIST = str(W * H * 128 + 64 * 4 * MAX_CUS)


def _binding():
    from raylib_amd import binding
    return binding


def bits(img):
    return np.ascontiguousarray(img, np.float32).view(np.uint32)


def render_three(ses, lib, monkeypatch, w=W, h=H, spp=4, max_path=5, in_place_equal=True):
    """The frame through the hit-queue, the ray-queue and the eager instance: the same uint32 words, the same counters; the lazy two with the same litPaths
    and (unless a list of a few chunks makes it depend on who drew which chunk) the same litFoldedInPlace.  Returns the stats of the two lazy renders."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    got = {}
    for name, env, ran in KERNELS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        img = ses.render(w, h, spp, max_path=max_path)
        assert (lib.RaylibAMD_LastTraceLazy(), lib.RaylibAMD_LastHitQueue()) == ran, name
        got[name] = (bits(img), ses.stats())
        for k in env:
            monkeypatch.delenv(k)
    want, se = got["eager"]
    assert se.litPaths == 0 and se.litFoldedInPlace == 0
    for name in ("hit queue", "ray queue"):
        img, st = got[name]
        differ = (img != want).any(-1)
        assert not differ.any(), "%s: %d pixels differ from the eager frame, the first at %s" % (name, int(differ.sum()), np.argwhere(differ)[0])
        for k in COUNTERS:
            assert getattr(st, k) == getattr(se, k), (name, k, getattr(st, k), getattr(se, k))
        assert st.litFoldedInPlace <= st.litPaths <= st.cameraSamples, (name, st.litFoldedInPlace, st.litPaths)
    a, b = got["hit queue"][1], got["ray queue"][1]
    assert a.litPaths == b.litPaths, (a.litPaths, b.litPaths)
    if in_place_equal:
        assert a.litFoldedInPlace == b.litFoldedInPlace, (a.litFoldedInPlace, b.litFoldedInPlace)
    return a, b


@pytest.fixture(scope="module")
def folder(workdir):
    d = os.path.join(str(workdir), "lit_fold"); os.makedirs(d, exist_ok=True)
    return d


@pytest.fixture(scope="module")
def cornell_obj(folder):
    return scenes.cornell(os.path.join(folder, "cornell.obj"))[0]


@pytest.fixture(scope="module")
def cornell(gpu_lib, cornell_obj):
    """Microfacet walls, a light, and a MIRROR box: the lit paths that meet the tall box carry a record that folds from the material alone."""
    ses = _binding().SceneSession(gpu_lib, cornell_obj, EYE, AT, 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    yield ses
    ses.close()


@pytest.fixture(scope="module")
def bright(gpu_lib, folder):
    """Ceiling, floor and walls all emit (the bright box of test_gpu_lazy_refl.py), seen from inside: nearly every path is lit."""
    mtl = MTL.replace("Ns 10\nillum 2", "Ns 10\nKe 0.5 0.25 0.125\nillum 2") % dict(kd="0.725 0.71 0.68", ks="0 0 0", ns="10", pr="Ke 0.25 0.5 1")
    obj = scenes.write_obj(os.path.join(folder, "bright.obj"), scenes.cornell_objects(scenes.WHITE, scenes.WHITE), mtl)[0]
    ses = _binding().SceneSession(gpu_lib, obj, INSIDE[0], INSIDE[1], 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    yield ses
    ses.close()


def test_several_chunk_rollovers(gpu_lib, bright, monkeypatch):
    """A workgroup per CU and 393 216 jobs, nearly all of them lit: more entries than two chunks for every wave the launch can have, so waves roll over to a
    fresh chunk, several times, and fold the full one each time.  128 samples: four words of the lit-sample mask per slot."""
    monkeypatch.setenv("RAYLIB_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("RAYLIB_LIT_LIST", BIG_LIST)
    a, b = render_three(bright, gpu_lib, monkeypatch, spp=128)
    assert gpu_lib.RaylibAMD_LastLitMask() == 0        # (the eager render ran last)
    for st in (a, b):
        assert st.litFoldedInPlace == 0 and st.litPaths > 2 * 64 * 4 * MAX_CUS, (st.litPaths, st.litFoldedInPlace)


def test_partial_last_chunk(gpu_lib, cornell, monkeypatch):
    """Fewer lit paths in the whole launch than its waves could hold in one chunk each: no chunk fills, every entry is folded at its wave's exit."""
    a, b = render_three(cornell, gpu_lib, monkeypatch, spp=4)
    for st in (a, b):   # (a fiftieth of this scene's paths end lit: one or two of a batch of 64)
        assert 0 < st.litPaths < st.cameraSamples // 10 and st.litFoldedInPlace == 0, (st.litPaths, st.litFoldedInPlace)
    # one batch of 64 jobs, one wave: its few lit paths are a partial chunk
    a, b = render_three(cornell, gpu_lib, monkeypatch, w=8, h=8, spp=1)
    assert a.litFoldedInPlace == 0 and a.litPaths < 64


def test_no_lit_path(gpu_lib, folder, monkeypatch):
    """A dark box: no lane of any wave ever ends lit, no chunk is reserved, nothing is folded -- and nothing of an earlier launch's list is."""
    mtl = MTL.replace("Ke 17 12 4", "Ke 0 0 0") % dict(kd="0.725 0.71 0.68", ks="0 0 0", ns="10", pr="")
    obj = scenes.write_obj(os.path.join(folder, "dark.obj"), scenes.cornell_objects(scenes.WHITE, scenes.WHITE), mtl)[0]
    ses = _binding().SceneSession(gpu_lib, obj, INSIDE[0], INSIDE[1], 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    for mask in ("0", "1"):
        monkeypatch.setenv("RAYLIB_LIT_MASK", mask)
        a, b = render_three(ses, gpu_lib, monkeypatch, spp=8)
        assert a.litPaths == 0 and a.litFoldedInPlace == 0 and a.shadedHits > 0
    assert not bits(ses.render(W, H, 8))[..., :3].any()
    ses.close()


@pytest.mark.parametrize("entries", ["0", "64", "192"])
def test_list_used_up(gpu_lib, bright, monkeypatch, entries):
    """No list, one chunk, three chunks, under far more lit paths: the entries written before the list ran out are folded by their waves (the chunks fill, and
    the wave that holds one when it draws beyond the list folds it), every other lit path in place.  Who gets the chunks depends on the run."""
    monkeypatch.setenv("RAYLIB_LIT_LIST", entries)
    for mask in ("0", "1"):
        monkeypatch.setenv("RAYLIB_LIT_MASK", mask)
        a, b = render_three(bright, gpu_lib, monkeypatch, spp=16, in_place_equal=entries == "0")
        for st in (a, b):
            listed = st.litPaths - st.litFoldedInPlace
            assert st.litPaths > 4 * int(entries), st.litPaths
            assert listed == 0 if entries == "0" else 0 < listed <= int(entries), (listed, entries)


@pytest.mark.parametrize("max_path", [1, 5, 6, 12])
def test_records_at_the_limit(gpu_lib, cornell, monkeypatch, max_path):
    """An entry holds RL_FOLD_PREFETCH = 5 vertex records.  maxPathLength 1: no record, or the one of a last vertex that failed the guard; 5: at most five; 6:
    paths of exactly five records and a last vertex in the registers -- with a sixth record only where that vertex failed the guard, which folds in place; 12:
    paths of more records than an entry holds fold in place, the others from their entries."""
    a, b = render_three(cornell, gpu_lib, monkeypatch, spp=16, max_path=max_path)
    assert a.litPaths > 0
    if max_path <= 5:
        assert a.litFoldedInPlace == 0
    if max_path == 12:
        assert 0 < a.litFoldedInPlace < a.litPaths


@pytest.mark.parametrize("mask", ["0", "1"])
@pytest.mark.parametrize("spp", [8, 70])
def test_lit_sample_mask(gpu_lib, cornell, bright, monkeypatch, mask, spp):
    """The chunk fold stores and flags by the mask's rule (csrc/rl_lit_mask.h); 70 samples are three words per slot."""
    monkeypatch.setenv("RAYLIB_LIT_MASK", mask)
    for ses in (cornell, bright):
        a, b = render_three(ses, gpu_lib, monkeypatch, spp=spp, in_place_equal=not (ses is bright and spp == 70))
        assert a.litPaths > 0
        # (the bright box at 70 samples lights more paths than the planner's list holds: there the waves' folds and the in-place folds set bits of the same words)
        assert a.litFoldedInPlace == 0 or (ses is bright and spp == 70), a.litFoldedInPlace
    monkeypatch.setenv("RAYLIB_HIT_QUEUE", "1")
    cornell.render(16, 16, 1)
    assert (gpu_lib.RaylibAMD_LastLitMask(), gpu_lib.RaylibAMD_LastHitQueue()) == (int(mask), 1)


@pytest.mark.parametrize("env", [{"RAYLIB_LIT_LIST": BIG_LIST}, {"RAYLIB_LIT_LIST": BIG_LIST, "RAYLIB_LIT_MASK": "1"}, {"RAYLIB_LIT_LIST": "64"}])
def test_camera_rays_that_miss_into_a_sun(gpu_lib, cornell_obj, monkeypatch, env):
    """From inside, looking out through the opening at a sun: nearly every camera ray misses the scene in its batch and ends lit there, a path of zero records
    reserved at the hit-queue instance's second site -- up to 64 of them a batch, and with a workgroup per CU and 393 216 jobs more than two chunks' worth for
    every wave the launch can have, so the chunks roll over in the stocking loop."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RAYLIB_BLOCKS_PER_CU", "1")
    ses = _binding().SceneSession(gpu_lib, cornell_obj, (0, 1, 0), (0.2, 1.3, 4), 45.0, W / H, sun=(20, 20, 20), sun_dir=(-0.05, -0.08, -1.0))
    one_chunk = env["RAYLIB_LIT_LIST"] == "64"
    a, b = render_three(ses, gpu_lib, monkeypatch, spp=128, in_place_equal=not one_chunk)
    for st in (a, b):
        assert st.litPaths > 2 * 64 * 4 * MAX_CUS, (st.litPaths, st.cameraSamples)
        assert 0 < st.litPaths - st.litFoldedInPlace <= 64 if one_chunk else st.litFoldedInPlace == 0
    ses.close()


def test_progressive_session_of_two_passes(gpu_lib, bright, monkeypatch):
    """Two passes of a session reach the same enqueue code: each pass's lit list is folded inside its launch, and the session's frame is the one-shot frame."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    frames, stats = {}, {}
    for name, env, ran in KERNELS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        P = _binding().Progressive(bright, W, H, 8)
        assert P.handle
        frames[name], stats[name] = [], []
        for _ in range(2):
            P.step(4)
            assert (gpu_lib.RaylibAMD_LastTraceLazy(), gpu_lib.RaylibAMD_LastHitQueue()) == ran, name
            frames[name].append(bits(P.frame()))
            stats[name].append(bright.stats())
        P.close()
        for k in env:
            monkeypatch.delenv(k)
    for name in ("hit queue", "ray queue"):
        for k in range(2):
            assert (frames[name][k] == frames["eager"][k]).all(), (name, k)
            for c in COUNTERS:
                assert getattr(stats[name][k], c) == getattr(stats["eager"][k], c), (name, k, c)
            assert stats[name][k].litPaths == stats["hit queue"][k].litPaths > 0 and stats[name][k].litFoldedInPlace == 0
    assert (frames["hit queue"][1] == bits(bright.render(W, H, 8))).all()


def test_two_logical_ranks(gpu_lib, cornell_obj, workdir):
    """Raylib_Render over two ranks on one device (tests/hit_queue_rank_child.py): each rank's waves fold its own list; the frame is the one-rank frame, the
    counters are the eager run's, and both lazy instances light the same paths."""
    import hit_queue_rank_child as child
    got = {}
    for name, env, ran in KERNELS:
        out = os.path.join(str(workdir), "lit_fold_ranks_%s.npz" % name.replace(" ", "_"))
        e = dict(os.environ, RAYLIB_NUM_GPUS="2", RAYLIB_GPU_MAP="0,0", RAYLIB_POOL="0", **env)
        e.pop("RAYLIB_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(child.__file__), out, cornell_obj, "96", "54", "4"], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        got[name] = np.load(out)
        assert int(got[name]["ranks"]) == 2 and (int(got[name]["lazy"]), int(got[name]["hitQueue"])) == ran, name
    work = [child.COUNTERS.index(k) for k in child.COUNTERS if not k.startswith("lit")]
    lit, in_place = child.COUNTERS.index("litPaths"), child.COUNTERS.index("litFoldedInPlace")
    want = got["eager"]
    assert int(want["counters"][lit]) == 0
    for name in ("hit queue", "ray queue"):
        g = got[name]
        assert (bits(g["img"]) == bits(want["img"])).all(), name
        assert np.array_equal(g["counters"][work], want["counters"][work]), (name, child.COUNTERS, g["counters"], want["counters"])
        assert int(g["counters"][lit]) == int(got["hit queue"]["counters"][lit]) > 0 and int(g["counters"][in_place]) == 0
    ses = _binding().SceneSession(gpu_lib, cornell_obj, EYE, AT, 45.0, 96 / 54)
    one = ses.render(96, 54, 4)
    assert (bits(got["hit queue"]["img"]) == bits(one)).all()
    assert int(got["hit queue"]["counters"][lit]) == ses.stats().litPaths      # the same paths are lit, however the cells were dealt
    ses.close()
