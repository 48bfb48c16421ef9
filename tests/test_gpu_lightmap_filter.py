"""The lightmap atlas filter on the device (RaylibAMD_FilterLightmap, RaylibAMD_BakeLightmapFiltered and their device entries; include/raylib_amd.h statement F)
against the host oracle RaylibAMD_FilterLightmapHost -- which tests/test_lightmap_filter_host.py holds to the NumPy restatement --, scattered and dilated by
tests/lightmap_cases.py, bit for bit on every texel and coverage byte.  Tess-12 Cornell, atlases of at most 128 x 128, 2 samples, maxPathLength 3."""
import ctypes as C
import os

import numpy as np
import pytest
import torch    # before the library is loaded: the device entry takes torch's tensors, and both must run on one HIP runtime

import helpers
from helpers import scenes
import lightmap_cases as lc
import lightmap_filter_cases as fc

pytestmark = pytest.mark.gpu
F = np.float32
MAX_PATH = 3
W, H, SAMPLES = 61, 47, 2
SIGMAS = (0.8, 0.5, 0.05)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    monkeypatch.delenv("RAYLIB_GATHER_BATCH", raising=False)


@pytest.fixture(scope="module")
def cornell(gpu_lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "lightmap_filter_gpu"); os.makedirs(d, exist_ok=True)
    ses = binding.SceneSession(gpu_lib, scenes.cornell(os.path.join(d, "cornell12.obj"), tess=12)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    yield ses, lc.grid_uv(len(lc.scene_triangles(gpu_lib, ses.scene)))
    ses.close()


@pytest.fixture(scope="module")
def points_of(gpu_lib, cornell):
    """(w, h, first, count) -> the oracle's points and texels, once per key."""
    from raylib_amd import binding
    ses, uv = cornell
    cache = {}

    def get(w, h, first=0, count=-1):
        key = (w, h, first, count)
        if key not in cache:
            sub = uv[first:] if count < 0 else uv[first:first + count]
            pts, tex, n = binding.lightmap_points(gpu_lib, ses.scene, w, h, sub, tri_first=first, tri_count=count, host=True)
            assert n == len(tex)
            cache[key] = (pts, tex, sub)
        return cache[key]
    return get


def _stats(lib):
    from raylib_amd import binding
    st = binding.Stats()
    lib.RaylibAMD_GetLastStats(C.byref(st))
    return st.as_dict()


def _synthetic_atlas(w, h, kind, tex, seed):
    """Values at the covered texels and, everywhere else, what the filter must ignore."""
    vals = fc.synthetic_values(len(tex), kind, seed)
    atlas = np.full((h * w, fc.CHANNELS[kind]), 1e30, F)
    atlas[::3] = np.nan
    atlas[tex] = vals
    return vals, np.ascontiguousarray(atlas.reshape(h, w, -1))


def _want(lib, w, h, kind, filt, pts, tex, vals, dilate):
    from raylib_amd import binding
    filtered = binding.filter_lightmap_host(lib, w, h, kind, filt, pts, tex, vals)
    return lc.dilate(*lc.scatter(filtered, tex, w, h), dilate)


def _same(got, got_cov, want, want_cov):
    got, got_cov = [a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in (got, got_cov)]
    assert np.array_equal(got_cov, want_cov)
    assert lc.same_bits(got, want), "%d texels differ" % (got.view(np.uint32) != want.view(np.uint32)).any(-1).sum()


# ---- 1. an atlas the caller has ----
@pytest.mark.parametrize("dilate", [0, 2])
@pytest.mark.parametrize("k", [1, 3, 6])
@pytest.mark.parametrize("kind", [0, 1], ids=["irradiance", "sh9"])
def test_filter_is_the_oracle_scattered_and_dilated(gpu_lib, cornell, points_of, kind, k, dilate):
    from raylib_amd import binding
    ses, _ = cornell
    pts, tex, uv = points_of(W, H)
    assert 500 < len(tex) < W * H                                    # there are gutters
    vals, atlas = _synthetic_atlas(W, H, kind, tex, seed=k)
    filt = (k,) + SIGMAS
    want, want_cov = _want(gpu_lib, W, H, kind, filt, pts, tex, vals, dilate)
    got, got_cov = binding.filter_lightmap(gpu_lib, ses.scene, W, H, atlas, filt, uv, kind, dilate=dilate)
    assert got.shape == (H, W, fc.CHANNELS[kind])
    _same(got, got_cov, want, want_cov)
    assert not lc.same_bits(got.reshape(W * H, -1)[tex], vals)       # it filtered
    st = _stats(gpu_lib)
    assert st["pixels"] == len(tex) and st["rays"] == 0 and st["kernelMs"] > 0


@pytest.mark.parametrize("atlas_size,k", [((128, 128), 6), ((1, 1), 3)], ids=["128x128", "1x1"])
@pytest.mark.parametrize("kind", [0, 1], ids=["irradiance", "sh9"])
def test_filter_steps_across_blocks_and_the_smallest_atlas(gpu_lib, cornell, points_of, kind, atlas_size, k):
    """128 x 128, K = 6: thousands of points in many blocks, taps 32 texels -- several blocks -- away; 1 x 1: one point, or none."""
    from raylib_amd import binding
    ses, _ = cornell
    w, h = atlas_size
    pts, tex, uv = points_of(w, h)
    vals, atlas = _synthetic_atlas(w, h, kind, tex, seed=17)
    filt = (k,) + SIGMAS
    want, want_cov = _want(gpu_lib, w, h, kind, filt, pts, tex, vals, 1)
    got, got_cov = binding.filter_lightmap(gpu_lib, ses.scene, w, h, atlas, filt, uv, kind, dilate=1)
    _same(got, got_cov, want, want_cov)
    if w > 1:
        assert len(tex) > 4 * 256


# ---- 2. the filtered bake ----
@pytest.fixture(scope="module")
def gathered(gpu_lib, cornell, points_of):
    """want(kind, tree, first, count) -> (points, texels, RaylibAMD_Gather's values on them, uv), once per key; the caller has set RAYLIB_QUERY_TREE."""
    from raylib_amd import binding
    ses, _ = cornell
    cache = {}

    def want(kind, tree, first=0, count=-1):
        key = (kind, tree, first, count)
        if key not in cache:
            assert os.environ.get("RAYLIB_QUERY_TREE") == tree
            pts, tex, uv = points_of(W, H, first, count)
            cache[key] = (pts, tex, binding.gather(gpu_lib, ses.scene, pts, kind, max_path=MAX_PATH, sample_count=SAMPLES), uv)
        return cache[key]
    return want


@pytest.mark.parametrize("tree", ["2", "4"])
@pytest.mark.parametrize("kind", [0, 1], ids=["irradiance", "sh9"])
def test_bake_is_gather_filtered_scattered_and_dilated(gpu_lib, cornell, gathered, monkeypatch, kind, tree):
    from raylib_amd import binding
    monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
    ses, _ = cornell
    filt = (4,) + SIGMAS
    args = dict(max_path=MAX_PATH, sample_count=SAMPLES, filter=filt)
    pts, tex, vals, uv = gathered(kind, tree)
    want, want_cov = _want(gpu_lib, W, H, kind, filt, pts, tex, vals, 2)
    got, got_cov = binding.bake_lightmap(gpu_lib, ses.scene, W, H, uv, kind, dilate=2, **args)
    _same(got, got_cov, want, want_cov)
    raw, raw_cov = binding.bake_lightmap(gpu_lib, ses.scene, W, H, uv, kind, dilate=2, max_path=MAX_PATH, sample_count=SAMPLES)
    assert np.array_equal(raw_cov, got_cov) and not lc.same_bits(raw, got)
    # a sub-range of the triangles
    pts, tex, vals, uv = gathered(kind, tree, 1000, 3000)
    want, want_cov = _want(gpu_lib, W, H, kind, filt, pts, tex, vals, 1)
    got, got_cov = binding.bake_lightmap(gpu_lib, ses.scene, W, H, uv, kind, tri_first=1000, tri_count=3000, dilate=1, **args)
    _same(got, got_cov, want, want_cov)


@pytest.mark.parametrize("kind", [0, 1], ids=["irradiance", "sh9"])
def test_bake_cut_into_launches(gpu_lib, cornell, gathered, monkeypatch, kind):
    """The filter sees the gather's values, however the gather was cut."""
    from raylib_amd import binding
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "4")
    ses, _ = cornell
    filt = (3,) + SIGMAS
    pts, tex, vals, uv = gathered(kind, "4")
    want, want_cov = _want(gpu_lib, W, H, kind, filt, pts, tex, vals, 1)
    for slots in (len(tex) + 7, len(tex) // 3):                      # sample ranges; point ranges of one sample each
        monkeypatch.setenv("RAYLIB_GATHER_BATCH", str(slots))
        got, got_cov = binding.bake_lightmap(gpu_lib, ses.scene, W, H, uv, kind, dilate=1, max_path=MAX_PATH, sample_count=SAMPLES, filter=filt)
        assert _stats(gpu_lib)["traceLaunches"] > 1
        _same(got, got_cov, want, want_cov)


# ---- 3. the device entries ----
@pytest.mark.parametrize("kind", [0, 1], ids=["irradiance", "sh9"])
def test_device_entries(gpu_lib, cornell, points_of, kind):
    from raylib_amd import binding
    ses, _ = cornell
    pts, tex, uv = points_of(W, H)
    filt = (3,) + SIGMAS
    vals, atlas = _synthetic_atlas(W, H, kind, tex, seed=23)
    want, want_cov = binding.filter_lightmap(gpu_lib, ses.scene, W, H, atlas, filt, uv, kind, dilate=2)
    baked, baked_cov = binding.bake_lightmap(gpu_lib, ses.scene, W, H, uv, kind, dilate=2, max_path=MAX_PATH, sample_count=SAMPLES, filter=filt)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    src, uv_src = torch.from_numpy(atlas).to(dev), torch.from_numpy(uv).to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        d_atlas, d_uv = src * 1.0, uv_src * 1.0                      # made on the caller's stream: the call is ordered behind them
        got, got_cov = binding.filter_lightmap(gpu_lib, ses.scene, W, H, d_atlas, filt, d_uv, kind, dilate=2)
        same, same_cov = binding.filter_lightmap(gpu_lib, ses.scene, W, H, d_atlas, filt, d_uv, kind, dilate=2, out=d_atlas)   # out is in
        d_baked, d_baked_cov = binding.bake_lightmap(gpu_lib, ses.scene, W, H, d_uv, kind, dilate=2, max_path=MAX_PATH, sample_count=SAMPLES, filter=filt)
    stream.synchronize()
    _same(got, got_cov, want, want_cov)
    assert same is d_atlas
    _same(same, same_cov, want, want_cov)
    _same(d_baked, d_baked_cov, baked, baked_cov)
    # the host entry in place
    work = atlas.copy()
    got, got_cov = binding.filter_lightmap(gpu_lib, ses.scene, W, H, work, filt, uv, kind, dilate=2, out=work)
    assert got is work
    _same(work, got_cov, want, want_cov)
    # a pointer of the host's is refused by the device entry
    prm, flt = binding.lightmap_params(W, H, kind), binding.lightmap_filter_params(filt)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    before = work.copy()
    assert gpu_lib.RaylibAMD_FilterLightmapDevice(ses.scene, C.byref(prm), C.byref(flt), None, fp(atlas), fp(work), None, None) == 0
    assert lc.same_bits(work, before)


# ---- 4. the stats ----
def test_stats(gpu_lib, cornell, points_of, monkeypatch):
    from raylib_amd import binding
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "4")
    ses, _ = cornell
    pts, tex, uv = points_of(W, H)
    args = dict(dilate=1, max_path=MAX_PATH, sample_count=SAMPLES)
    binding.bake_lightmap(gpu_lib, ses.scene, W, H, uv, 0, **args)
    plain = _stats(gpu_lib)
    binding.bake_lightmap(gpu_lib, ses.scene, W, H, uv, 0, filter=(5,) + SIGMAS, **args)
    st = _stats(gpu_lib)
    assert st["pixels"] == plain["pixels"] == len(tex) and st["cameraSamples"] == len(tex) * SAMPLES
    for k in ("rays", "nodesVisited", "trisTested", "shadedHits", "texFetches", "treeWidth", "nodeBytes", "traceLaunches", "numTriangles"):
        assert st[k] == plain[k], k                                  # the filter traces nothing
    assert st["kernelMs"] >= st["traceKernelMs"] > 0
    assert st["kernelMs"] >= plain["traceKernelMs"] > 0              # the whole filtered call against the unfiltered bake's gather time
