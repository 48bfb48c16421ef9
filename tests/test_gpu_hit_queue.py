"""The hit-queue form of the leaf-list kernel's lazy-reflectance instance (k_trace_lazy_hitq, csrc/rl_k_trace_hitq.inl): idle lanes take camera rays that have
been traced already.  Every frame must be the ray-queue instance's (RAYLIB_HIT_QUEUE=0, k_trace_lazy) bit for bit, with the same work counters -- waveTrips
aside, which depends on which wave drew which batch -- and RaylibAMD_LastHitQueue must say which of the two ran.  The shapes are the smallest at which the new
loop can still go wrong: one batch, partial cells, several batches per wave, a queue that stays nearly empty, batches in which every ray misses the root."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from helpers import scenes
from test_lazy_refl_host import MTL

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "nodesVisited", "trisTested", "shadedHits", "texFetches", "cameraSamples", "culledSamples", "culledCells", "listedCells", "pixels", "traceLaunches",
            "litPaths")
EYE, AT = (0, 1, 4), (0, 1, -1)


def _binding():
    from raylib_amd import binding
    return binding


def render_both(ses, lib, monkeypatch, w, h, spp, max_path=5, tmin=1e-4, in_place_equal=True):
    """The frame through the hit-queue instance and through the ray-queue one: the same bits, the same counters.  Returns the hit-queue render's stats."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    monkeypatch.setenv("RAYLIB_HIT_QUEUE", "1")
    a = ses.render(w, h, spp, max_path=max_path, tmin=tmin)
    ran_a, sa = (lib.RaylibAMD_LastHitQueue(), lib.RaylibAMD_LastTraceLazy()), ses.stats()
    monkeypatch.setenv("RAYLIB_HIT_QUEUE", "0")
    b = ses.render(w, h, spp, max_path=max_path, tmin=tmin)
    ran_b, sb = (lib.RaylibAMD_LastHitQueue(), lib.RaylibAMD_LastTraceLazy()), ses.stats()
    monkeypatch.delenv("RAYLIB_HIT_QUEUE")
    assert (ran_a, ran_b) == ((1, 1), (0, 1)), (ran_a, ran_b)
    differ = ~helpers.same(a, b)
    assert not differ.any(), "%d pixels differ" % int(differ.any(-1).sum())
    for k in COUNTERS:
        assert getattr(sa, k) == getattr(sb, k), (k, getattr(sa, k), getattr(sb, k))
    if in_place_equal:
        assert sa.litFoldedInPlace == sb.litFoldedInPlace, (sa.litFoldedInPlace, sb.litFoldedInPlace)
    return sa


def _session(lib, obj, eye=EYE, at=AT, aspect=1.0, fov=45.0, **kw):
    return _binding().SceneSession(lib, obj, eye, at, fov, aspect, **kw)


@pytest.fixture(scope="module")
def cornell_obj(workdir):
    d = os.path.join(str(workdir), "hit_queue"); os.makedirs(d, exist_ok=True)
    return scenes.cornell(os.path.join(d, "cornell.obj"))[0]


@pytest.fixture(scope="module")
def cornell(gpu_lib, cornell_obj):
    ses = _session(gpu_lib, cornell_obj, aspect=16 / 9)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    yield ses
    ses.close()


@pytest.mark.parametrize("w,h,spp", [(8, 8, 1), (61, 37, 3), (200, 120, 5), (96, 64, 70)])
def test_frame_sizes(gpu_lib, cornell, monkeypatch, w, h, spp):
    """One batch in one wave; partial cells (batch lanes without a pixel); many batches; more than two words of the lit-sample mask."""
    st = render_both(cornell, gpu_lib, monkeypatch, w, h, spp)
    assert st.cameraSamples + st.culledSamples == w * h * spp and st.shadedHits > 0


def test_every_wave_stocks_several_times(gpu_lib, cornell, monkeypatch):
    """A workgroup per CU: the 6720 batches of the frame go to a quarter of the waves, more than one batch each even on 256 CUs."""
    monkeypatch.setenv("RAYLIB_BLOCKS_PER_CU", "1")
    render_both(cornell, gpu_lib, monkeypatch, 96, 64, 70)


@pytest.mark.parametrize("max_path", [1, 2, 5, 12])
def test_path_lengths(gpu_lib, cornell, monkeypatch, max_path):
    """12 vertices are more than an entry of the lit list holds (RL_FOLD_PREFETCH = 5): those lit paths fold in place, the same ones in both instances."""
    st = render_both(cornell, gpu_lib, monkeypatch, 64, 40, 4, max_path=max_path)
    assert st.litPaths > 0 and (st.litFoldedInPlace > 0) == (max_path == 12)


def test_queue_underflow_and_termination(gpu_lib, cornell_obj, monkeypatch):
    # inside the room, above the boxes, looking out through the open front: every camera ray passes the root test, the middle of the frame misses the scene
    # and only its rim meets the ceiling and the side walls -- batches that queue few hits or none
    ses = _session(gpu_lib, cornell_obj, eye=(0, 1.5, 0), at=(0, 1.5, 4), aspect=1.6, fov=70.0)
    st = render_both(ses, gpu_lib, monkeypatch, 64, 40, 4)
    assert 0 < st.shadedHits and st.culledSamples == 0, (st.shadedHits, st.culledSamples)
    ses.close()
    # the box behind the camera: every ray of every listed cell misses the root (the cull would list no cell at all)
    ses = _session(gpu_lib, cornell_obj, eye=(0, 1, 4), at=(0, 1, 9), aspect=1.6)
    monkeypatch.setenv("RAYLIB_CULL_CELLS", "0")
    st = render_both(ses, gpu_lib, monkeypatch, 64, 40, 3)
    assert st.shadedHits == 0 and st.cameraSamples == 64 * 40 * 3 and st.rays == st.cameraSamples
    monkeypatch.delenv("RAYLIB_CULL_CELLS")
    st = render_both(ses, gpu_lib, monkeypatch, 64, 40, 3)
    assert st.shadedHits == 0 and st.cameraSamples + st.culledSamples == 64 * 40 * 3
    ses.close()


@pytest.mark.parametrize("name,value", [("RAYLIB_CULL_CELLS", "0"), ("RAYLIB_JOB_HEADS", "1"), ("RAYLIB_LIT_MASK", "0"), ("RAYLIB_LIT_MASK", "1"),
                                        ("RAYLIB_LIT_LIST", "0"), ("RAYLIB_LIT_LIST", "64")])
def test_switches(gpu_lib, cornell, monkeypatch, name, value):
    monkeypatch.setenv(name, value)
    # A list of one chunk belongs to the first wave that asks for it, and how many of its 64 entries that wave fills before the launch ends depends on which
    # batches it drew: litFoldedInPlace then varies from run to run in either instance, and only its range is checked.
    one_chunk = (name, value) == ("RAYLIB_LIT_LIST", "64")
    st = render_both(cornell, gpu_lib, monkeypatch, 128, 72, 8, in_place_equal=not one_chunk)
    assert st.litPaths > 64
    if name == "RAYLIB_LIT_LIST":
        listed = st.litPaths - st.litFoldedInPlace
        assert listed == 0 if value == "0" else 0 < listed <= 64
    if name == "RAYLIB_LIT_MASK":
        assert gpu_lib.RaylibAMD_LastLitMask() == int(value)   # (the last render was the ray-queue instance's ...)
        monkeypatch.setenv("RAYLIB_HIT_QUEUE", "1")
        cornell.render(16, 16, 1)
        assert (gpu_lib.RaylibAMD_LastLitMask(), gpu_lib.RaylibAMD_LastHitQueue()) == (int(value), 1)   # (... and the switch is the hit-queue instance's too)


@pytest.mark.parametrize("env", [{}, {"RAYLIB_LIT_LIST": "0"}, {"RAYLIB_LIT_MASK": "1"}, {"RAYLIB_LIT_MASK": "1", "RAYLIB_LIT_LIST": "0"}])
def test_sun_through_the_opening(gpu_lib, cornell_obj, monkeypatch, env):
    """The miss shader's occlusion query runs in the batch (camera rays) and in the trip (bounce rays).  A camera ray that misses into the sun is a lit path of
    zero records: counted in litPaths, and in litFoldedInPlace when there is no list."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ses = _session(gpu_lib, cornell_obj, eye=(0.3, 1.2, 4), at=(0, 0.9, -1), aspect=1.6, sun=(20, 20, 20), sun_dir=(0.2, -0.3, -1.0))
    st = render_both(ses, gpu_lib, monkeypatch, 96, 60, 4)
    assert st.litPaths > 0
    assert (st.litFoldedInPlace == st.litPaths) == (env.get("RAYLIB_LIT_LIST") == "0")
    # from inside, looking out: nearly every camera ray passes the root test, misses the scene and meets the sun or the room's shadow
    inside = _session(gpu_lib, cornell_obj, eye=(0, 1, 0), at=(0.2, 1.3, 4), aspect=1.6, sun=(20, 20, 20), sun_dir=(-0.05, -0.08, -1.0))
    st = render_both(inside, gpu_lib, monkeypatch, 64, 40, 3)
    assert st.litPaths > 0
    inside.close()
    ses.close()


def test_many_candidates(gpu_lib, workdir, monkeypatch):
    """The 24-leaf soup of large overlapping triangles (test_gpu_parity.py test_leaf_list_with_every_leaf_a_candidate) as a frame: many rays meet every leaf's
    box.  Its triangles get an emitting microfacet material, so that the lazy instance takes the scene and paths end lit."""
    d = os.path.join(str(workdir), "hit_queue"); os.makedirs(d, exist_ok=True)
    obj, _ = scenes.soup(os.path.join(d, "soup.obj"), n_tris=103, seed=11, extent=0.6, size=1.8)
    text = open(obj).read()
    with open(obj, "w") as f:
        f.write("mtllib soup.mtl\n" + text.replace("o soup\n", "o soup\nusemtl light\n", 1))
    with open(os.path.join(d, "soup.mtl"), "w") as f:
        f.write(MTL % dict(kd="0.725 0.71 0.68", ks="0 0 0", ns="10", pr=""))
    ses = _binding().SceneSession(gpu_lib, obj, (0, 1, 4), (0, 1, -1), 50.0, 1.5)
    import ctypes as C
    most = C.c_uint32()
    assert gpu_lib.RaylibAMD_SceneLeafListInfo(ses.scene, C.byref(most)) == 24 and gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    for tmin in (0.0, 1e-4):
        st = render_both(ses, gpu_lib, monkeypatch, 96, 64, 2, max_path=9, tmin=tmin)
        assert st.litPaths > 0
    ses.close()


def test_lens_camera(gpu_lib, cornell_obj, monkeypatch):
    """An aperture: the camera rays of a batch start at different points of the lens, and a queue entry carries each ray's own origin."""
    ses = _session(gpu_lib, cornell_obj, aspect=1.6, aperture=0.25, focal=4.0)
    render_both(ses, gpu_lib, monkeypatch, 64, 40, 4)
    ses.close()


def test_progressive_session(gpu_lib, cornell, monkeypatch):
    monkeypatch.setenv("RAYLIB_POOL", "0")
    w, h = 44, 36
    frames, stats = [], []
    for hq in ("1", "0"):
        monkeypatch.setenv("RAYLIB_HIT_QUEUE", hq)
        P = _binding().Progressive(cornell, w, h, 8)
        assert P.handle
        for _ in range(4):
            P.step(2)
            assert (gpu_lib.RaylibAMD_LastHitQueue(), gpu_lib.RaylibAMD_LastTraceLazy()) == (int(hq), 1)
            frames.append(P.frame())
            stats.append(cornell.stats())
        P.close()
    monkeypatch.delenv("RAYLIB_HIT_QUEUE")
    for a, b, sa, sb in zip(frames[:4], frames[4:], stats[:4], stats[4:]):
        assert helpers.same(a, b).all()
        for k in COUNTERS + ("litFoldedInPlace",):
            assert getattr(sa, k) == getattr(sb, k), (k, getattr(sa, k), getattr(sb, k))


def test_two_logical_ranks(gpu_lib, cornell_obj, workdir):
    """Raylib_Render over two ranks on one device (tests/hit_queue_rank_child.py): each rank runs the instance on its cells; the frame and the counters are the
    ray-queue run's."""
    import hit_queue_rank_child as child
    got = {}
    for hq in ("1", "0"):
        out = os.path.join(str(workdir), "hit_queue_ranks_%s.npz" % hq)
        env = dict(os.environ, RAYLIB_NUM_GPUS="2", RAYLIB_GPU_MAP="0,0", RAYLIB_HIT_QUEUE=hq, RAYLIB_POOL="0")
        env.pop("RAYLIB_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(child.__file__), out, cornell_obj, "96", "54", "4"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        got[hq] = np.load(out)
        assert int(got[hq]["ranks"]) == 2 and (int(got[hq]["hitQueue"]), int(got[hq]["lazy"])) == (int(hq), 1)
    a, b = got["1"], got["0"]
    assert np.array_equal(a["counters"], b["counters"]), (child.COUNTERS, a["counters"], b["counters"])
    assert int(a["counters"][child.COUNTERS.index("litPaths")]) > 0
    assert helpers.same(a["img"], b["img"]).all()
