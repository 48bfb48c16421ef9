"""Lightmaps baked on the device (RaylibAMD_LightmapPoints, RaylibAMD_BakeLightmap, RaylibAMD_BakeLightmapDevice; include/raylib_amd.h): the raster stages
against the host oracle RaylibAMD_LightmapPointsHost bit for bit -- which tests/test_lightmap_host.py holds to the NumPy restatement --, the whole bake against
RaylibAMD_Gather on those points scattered and dilated by the restatement (tests/lightmap_cases.py), bit for bit on every texel and coverage byte, then the
cut into launches, the stream rule, the device entry and the stats.  Atlases of at most 128 x 128, 1 to 4 samples, maxPathLength 3."""
import ctypes as C
import os

import numpy as np
import pytest
import torch    # before the library is loaded: the device entry takes torch's tensors, and both must run on one HIP runtime

import helpers
from helpers import scenes
import lightmap_cases as lc

pytestmark = pytest.mark.gpu
F = np.float32
MAX_PATH = 3


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    monkeypatch.delenv("RAYLIB_GATHER_BATCH", raising=False)


@pytest.fixture(scope="module")
def cornells(gpu_lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "lightmap_gpu"); os.makedirs(d, exist_ok=True)
    out = {}
    for tess in (1, 12):
        ses = binding.SceneSession(gpu_lib, scenes.cornell(os.path.join(d, "cornell%d.obj" % tess), tess=tess)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
        out[tess] = (ses, lc.scene_triangles(gpu_lib, ses.scene))
    yield out
    for ses, _ in out.values():
        ses.close()


def _stats(lib):
    from raylib_amd import binding
    st = binding.Stats()
    lib.RaylibAMD_GetLastStats(C.byref(st))
    return st


def _device_is_host(lib, scene, w, h, uv, what, **kw):
    from raylib_amd import binding
    hp, ht, hn = binding.lightmap_points(lib, scene, w, h, uv, host=True, **kw)
    dp, dt, dn = binding.lightmap_points(lib, scene, w, h, uv, **kw)
    assert dn == hn, (what, dn, hn)
    assert np.array_equal(dt, ht), what
    assert lc.same_bits(dp, hp), what
    return hn


# ---- 1. the raster stages against the oracle ----
@pytest.mark.parametrize("atlas", lc.ATLASES, ids=lambda a: "%dx%d" % a)
@pytest.mark.parametrize("gen", ["grid", "own"])
@pytest.mark.parametrize("tess", [1, 12])
def test_points_are_the_oracles(gpu_lib, cornells, tess, gen, atlas):
    ses, tris = cornells[tess]
    uv = lc.grid_uv(len(tris)) if gen == "grid" else None
    _device_is_host(gpu_lib, ses.scene, atlas[0], atlas[1], uv, (tess, gen, atlas), time=0.25)


@pytest.mark.parametrize("name", sorted(lc.edge_inputs()))
def test_points_edge_inputs(gpu_lib, cornells, name):
    ses, tris = cornells[1]
    w, h, uv = lc.edge_inputs(len(tris))[name]
    _device_is_host(gpu_lib, ses.scene, w, h, uv, name)


def test_points_big_and_small(gpu_lib, cornells):
    """One triangle that fills 128 x 128 behind 5183 triangles smaller than a texel: the pairs of the last triangle are nearly all the pairs, and the binary
    search runs over thousands of triangles without pairs."""
    ses, tris = cornells[12]
    w, h, uv = lc.big_and_small(len(tris))
    assert _device_is_host(gpu_lib, ses.scene, w, h, uv, "big and small") == w * h


def test_points_sub_range_capacity_and_fallback(gpu_lib, cornells):
    from raylib_amd import binding
    ses, tris = cornells[12]
    uv = lc.grid_uv(len(tris))
    n = _device_is_host(gpu_lib, ses.scene, 61, 47, uv[100:300], "sub-range", tri_first=100, tri_count=200)
    _device_is_host(gpu_lib, ses.scene, 61, 47, uv[5000:], "to the end", tri_first=5000)
    assert n > 10
    hp, ht, hn = binding.lightmap_points(gpu_lib, ses.scene, 61, 47, uv[100:300], tri_first=100, tri_count=200, host=True, capacity=10)
    dp, dt, dn = binding.lightmap_points(gpu_lib, ses.scene, 61, 47, uv[100:300], tri_first=100, tri_count=200, capacity=10)
    assert dn == hn == n and len(dp) == 10 and lc.same_bits(dp, hp) and np.array_equal(dt, ht)
    flat = [[0, 0, 0], [1, 0, 0], [0, 0, -1]]
    zero, up = np.zeros((3, 3)), np.tile([[0.0, 1.0, 0.0]], (3, 1))
    scene, close = lc.triangle_scene(gpu_lib, [([[0, 0, 0], [1, 0, 0], [2, 0, 0]], zero, [0, 0, 1, 0, 0, 1]), (flat, zero, [0, 0, 2, 0, 0, 2]), (flat, up, [0, 0, 2, 0, 0, 2]),
                                             (flat, [[0, 1, 0], [0, -1, 0], [0, -1, 0]], [0.5, 1, 1, 0.5, 1, 1])])
    try:
        assert _device_is_host(gpu_lib, scene, 16, 16, None, "face fallback and empty texels") > 0
    finally:
        close()


# ---- 2. the whole bake ----
BAKE_W, BAKE_H, BAKE_SAMPLES = 61, 47, 2


@pytest.fixture(scope="module")
def reference(gpu_lib, cornells):
    """want(kind, tree, first, count) -> (points, texels, RaylibAMD_Gather's values on them, its stats), once per key; the caller has set RAYLIB_QUERY_TREE."""
    from raylib_amd import binding
    ses, tris = cornells[12]
    uv = lc.grid_uv(len(tris))
    cache = {}

    def want(kind, tree, first=0, count=-1):
        key = (kind, tree, first, count)
        if key not in cache:
            assert os.environ.get("RAYLIB_QUERY_TREE") == tree
            sub = uv[first:] if count < 0 else uv[first:first + count]
            pts, tex, n = binding.lightmap_points(gpu_lib, ses.scene, BAKE_W, BAKE_H, sub, tri_first=first, tri_count=count, host=True)
            assert 500 < n < BAKE_W * BAKE_H                       # there are gutters to fill
            vals = binding.gather(gpu_lib, ses.scene, pts, kind, max_path=MAX_PATH, sample_count=BAKE_SAMPLES)
            cache[key] = (pts, tex, vals, _stats(gpu_lib).as_dict(), sub)
        return cache[key]
    return want


@pytest.mark.parametrize("dilate", [0, 1, 3])
@pytest.mark.parametrize("tree", ["2", "4"])
@pytest.mark.parametrize("kind", [0, 1], ids=["irradiance", "sh9"])
def test_bake_is_gather_scattered_and_dilated(gpu_lib, cornells, reference, monkeypatch, kind, tree, dilate):
    from raylib_amd import binding
    monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
    ses, _ = cornells[12]
    pts, tex, vals, _, uv = reference(kind, tree)
    atlas, cov = lc.scatter(vals, tex, BAKE_W, BAKE_H)
    atlas, cov = lc.dilate(atlas, cov, dilate)
    got, got_cov = binding.bake_lightmap(gpu_lib, ses.scene, BAKE_W, BAKE_H, uv, kind, dilate=dilate, max_path=MAX_PATH, sample_count=BAKE_SAMPLES)
    assert got.shape == (BAKE_H, BAKE_W, 4 if kind == 0 else 27)
    assert np.array_equal(got_cov, cov)
    assert lc.same_bits(got, atlas), "%d texels differ" % (got.view(np.uint32) != atlas.view(np.uint32)).any(-1).sum()
    if dilate:
        assert (cov > 1).any() and cov.max() <= 1 + dilate
        if kind == 0:
            assert (got[cov > 0][:, 3] == 1).all()


@pytest.mark.parametrize("kind", [0, 1], ids=["irradiance", "sh9"])
def test_bake_of_a_sub_range(gpu_lib, cornells, reference, monkeypatch, kind):
    from raylib_amd import binding
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "4")
    ses, _ = cornells[12]
    pts, tex, vals, _, uv = reference(kind, "4", 1000, 3000)
    atlas, cov = lc.dilate(*lc.scatter(vals, tex, BAKE_W, BAKE_H), 2)
    got, got_cov = binding.bake_lightmap(gpu_lib, ses.scene, BAKE_W, BAKE_H, uv, kind, tri_first=1000, tri_count=3000, dilate=2, max_path=MAX_PATH, sample_count=BAKE_SAMPLES)
    assert np.array_equal(got_cov, cov) and lc.same_bits(got, atlas)


# ---- 3. the gather cut into several launches ----
@pytest.mark.parametrize("kind", [0, 1], ids=["irradiance", "sh9"])
def test_bake_cut_into_launches(gpu_lib, cornells, monkeypatch, kind):
    from raylib_amd import binding
    ses, tris = cornells[12]
    uv = lc.grid_uv(len(tris))
    args = dict(dilate=1, max_path=MAX_PATH, sample_count=4)
    whole, whole_cov = binding.bake_lightmap(gpu_lib, ses.scene, BAKE_W, BAKE_H, uv, kind, **args)
    n = int(_stats(gpu_lib).pixels)
    assert _stats(gpu_lib).traceLaunches == 1
    for slots in (n * 2 + 7, n // 3):                  # sample ranges; point ranges of one sample each
        monkeypatch.setenv("RAYLIB_GATHER_BATCH", str(slots))
        cut, cut_cov = binding.bake_lightmap(gpu_lib, ses.scene, BAKE_W, BAKE_H, uv, kind, **args)
        assert _stats(gpu_lib).traceLaunches > 1
        assert np.array_equal(cut_cov, whole_cov) and lc.same_bits(cut, whole), slots


# ---- 4. the stream rule ----
def test_a_texel_does_not_depend_on_other_charts(gpu_lib, cornells):
    from raylib_amd import binding
    ses, tris = cornells[1]
    full = lc.grid_uv(len(tris))
    alone = np.zeros_like(full); alone[0:2] = full[0:2]            # the floor's chart alone
    a, a_cov = binding.bake_lightmap(gpu_lib, ses.scene, 64, 64, alone, 0, max_path=MAX_PATH, sample_count=4)
    b, b_cov = binding.bake_lightmap(gpu_lib, ses.scene, 64, 64, full, 0, max_path=MAX_PATH, sample_count=4)
    own = a_cov == 1
    assert own.sum() > 20 and b_cov.sum() > 10 * own.sum()
    assert (b_cov[own] == 1).all() and lc.same_bits(a[own], b[own])
    assert (a[own][:, :3] > 0).any()


# ---- 5. the device entry ----
@pytest.mark.parametrize("kind", [0, 1], ids=["irradiance", "sh9"])
def test_device_entry(gpu_lib, cornells, kind):
    from raylib_amd import binding
    ses, tris = cornells[12]
    uv = lc.grid_uv(len(tris))
    args = dict(dilate=2, max_path=MAX_PATH, sample_count=2)
    want, want_cov = binding.bake_lightmap(gpu_lib, ses.scene, BAKE_W, BAKE_H, uv, kind, **args)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    # uv is made by a device operation on the caller's stream, behind a few milliseconds of other work there: the call's raster stages, which run on the
    # library's stream, must wait for it
    src = torch.from_numpy(uv).to(dev)
    busy = torch.full((2048, 2048), 1e-3, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(20):
            busy = (busy @ busy) * 1e-3
        uv_dev = src * 1.0
        got, got_cov = binding.bake_lightmap(gpu_lib, ses.scene, BAKE_W, BAKE_H, uv_dev, kind, **args)
        again, _ = binding.bake_lightmap(gpu_lib, ses.scene, BAKE_W, BAKE_H, torch.from_numpy(uv).to(dev), kind, **args)   # enqueued behind the first, on the same scratch
    stream.synchronize()
    assert lc.same_bits(got.cpu().numpy(), want) and np.array_equal(got_cov.cpu().numpy(), want_cov)
    assert lc.same_bits(again.cpu().numpy(), want)
    # the triangles' own UVs, the library's stream
    own, own_cov = binding.bake_lightmap(gpu_lib, ses.scene, 32, 32, None, kind, **args)
    got, got_cov = binding.bake_lightmap(gpu_lib, ses.scene, 32, 32, None, kind, device=dev, **args)
    torch.cuda.synchronize()
    assert lc.same_bits(got.cpu().numpy(), own) and np.array_equal(got_cov.cpu().numpy(), own_cov)
    # nothing covered: a success, zeros, coverage 0 -- on both entries
    off = np.full((len(tris), 6), 5.0, F); off[:, 2] = 6.0; off[:, 5] = 6.0
    e, e_cov = binding.bake_lightmap(gpu_lib, ses.scene, 16, 16, off, kind, **args)
    assert not e.view(np.uint32).any() and not e_cov.any() and _stats(gpu_lib).pixels == 0
    with torch.cuda.stream(stream):
        e, e_cov = binding.bake_lightmap(gpu_lib, ses.scene, 16, 16, torch.from_numpy(off).to(dev), kind, **args)
    stream.synchronize()
    assert not e.cpu().numpy().view(np.uint32).any() and not e_cov.cpu().numpy().any()
    # a pointer of the host's is refused by the device entry
    prm = binding.lightmap_params(16, 16, kind)
    out = np.zeros((16, 16, 27), F)
    assert gpu_lib.RaylibAMD_BakeLightmapDevice(ses.scene, C.byref(prm), None, out.ctypes.data_as(C.POINTER(C.c_float)), None, None) == 0


# ---- 6. the stats ----
def test_stats(gpu_lib, cornells, reference, monkeypatch):
    from raylib_amd import binding
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "4")
    ses, _ = cornells[12]
    pts, tex, vals, before, uv = reference(0, "4")
    binding.bake_lightmap(gpu_lib, ses.scene, BAKE_W, BAKE_H, uv, 0, dilate=1, max_path=MAX_PATH, sample_count=BAKE_SAMPLES)
    st = _stats(gpu_lib).as_dict()
    assert st["pixels"] == len(tex) and st["cameraSamples"] == len(tex) * BAKE_SAMPLES
    for k in ("rays", "nodesVisited", "trisTested", "shadedHits", "texFetches", "treeWidth", "nodeBytes", "traceLaunches", "numTriangles"):
        assert st[k] == before[k], k                   # what the gather of those points reports
    assert st["kernelMs"] >= st["traceKernelMs"] > 0
    again = binding.gather(gpu_lib, ses.scene, pts, 0, max_path=MAX_PATH, sample_count=BAKE_SAMPLES)
    after = _stats(gpu_lib).as_dict()
    assert lc.same_bits(again, vals)
    for k in before:
        if not k.endswith("Ms") and k not in ("waveTrips", "rankKernelMs", "rankTraceMs"):   # (times, and the trips of the waves through the job counter)
            assert after[k] == before[k], k            # a gather before and after a bake: the same numbers


# ---- 7. the pair budget ----
def test_pair_budget(gpu_lib, cornells):
    """5184 triangles whose boxes are a whole 16384 x 16384 atlas are 2^40 pairs: refused by the device calls as by the oracle, before anything of the
    atlas' size is allocated; 200 of them on 4096 x 4096 (under 2^32) are not."""
    from raylib_amd import binding
    ses, tris = cornells[12]
    uv = np.tile(np.array([[-0.5, -0.5, 2.5, -0.5, -0.5, 2.5]], F), (len(tris), 1))
    for host in (True, False):
        with pytest.raises(RuntimeError):
            binding.lightmap_points(gpu_lib, ses.scene, 16384, 16384, uv, host=host, capacity=0)
    prm = binding.lightmap_params(16384, 16384, max_path=MAX_PATH)
    out = np.full(4, 7.0, F)
    assert gpu_lib.RaylibAMD_BakeLightmap(ses.scene, C.byref(prm), uv.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)), None) == 0
    assert (out == 7.0).all()
    _, _, n = binding.lightmap_points(gpu_lib, ses.scene, 4096, 4096, uv[:200], tri_count=200, capacity=0)
    assert n == 4096 * 4096
