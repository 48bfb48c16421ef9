"""The lightmap atlas filter without a device (RaylibAMD_FilterLightmapHost, include/raylib_amd.h statement F): the host oracle against the NumPy restatement
(tests/lightmap_filter_cases.py) bit for bit, on atlases from 1 x 1 to 128 x 128, both kinds, K = 1 .. 8; checks that do not rest on the restatement (charts
apart in the world do not see each other, a flat chart's variance falls); in place; the record layout; every refusal."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from helpers import scenes
import lightmap_cases as lc
import lightmap_filter_cases as fc

F = np.float32
FILTER = (3, 0.8, 0.5, 0.05)          # (K, sigmaColor, sigmaNormal, sigmaPosition): the Cornell box is 2 units wide, a texel of a 61 x 47 grid atlas ~0.01


@pytest.fixture(scope="module")
def cornell(lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "lightmap_filter_host"); os.makedirs(d, exist_ok=True)
    ses = binding.SceneSession(lib, scenes.cornell(os.path.join(d, "cornell12.obj"), tess=12)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    tris = lc.scene_triangles(lib, ses.scene)
    yield ses, lc.grid_uv(len(tris))
    ses.close()


@pytest.fixture(scope="module")
def points_of(lib, cornell):
    from raylib_amd import binding
    ses, uv = cornell
    cache = {}

    def get(w, h):
        if (w, h) not in cache:
            pts, tex, n = binding.lightmap_points(lib, ses.scene, w, h, uv, host=True)
            assert n == len(tex) and (w * h < 1000 or 100 < n < w * h)   # the larger atlases have gutters between the charts
            cache[(w, h)] = (pts, tex)
        return cache[(w, h)]
    return get


# (atlas, kind, K): both kinds and K = 1 .. 8 across the sizes; at 7 x 5 every tap but the centre's lies outside the atlas from step 8 on
CASES = [((1, 1), 0, 1), ((1, 1), 1, 8), ((7, 5), 0, 2), ((7, 5), 1, 3), ((7, 5), 0, 8), ((61, 47), 0, 4), ((61, 47), 1, 5), ((61, 47), 1, 1), ((61, 47), 0, 7),
         ((128, 128), 0, 6), ((128, 128), 1, 2)]


@pytest.mark.parametrize("atlas,kind,k", CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_oracle_is_the_restatement(lib, points_of, atlas, kind, k):
    from raylib_amd import binding
    w, h = atlas
    pts, tex = points_of(w, h)
    if atlas != (1, 1):
        assert len(tex) > 0
    vals = fc.synthetic_values(len(tex), kind, seed=w * 131 + k)
    filt = (k,) + FILTER[1:]
    got = binding.filter_lightmap_host(lib, w, h, kind, filt, pts, tex, vals)
    want = fc.filter_values(vals, pts, tex, w, h, filt)
    assert got.shape == vals.shape
    assert lc.same_bits(got, want), "%d of %d points differ" % ((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum(), len(tex))
    if len(tex) > 100:
        assert not lc.same_bits(got, vals)                           # it filtered
    if kind == 0 and len(tex):
        assert (got[:, 3] == 1).all()


def test_non_finite_and_alpha_inputs(lib, points_of):
    """Channels that are not finite read as 0 (F3); channel 3 of an IRRADIANCE texel is ignored and written 1."""
    from raylib_amd import binding
    w, h = 61, 47
    pts, tex = points_of(w, h)
    for kind in (0, 1):
        vals = fc.synthetic_values(len(tex), kind, seed=5)
        vals[7, 0] = np.nan; vals[11, 2] = np.inf; vals[400, 1] = -np.inf
        if kind == 0:
            vals[:, 3] = 0.25
        got = binding.filter_lightmap_host(lib, w, h, kind, FILTER, pts, tex, vals)
        assert lc.same_bits(got, fc.filter_values(vals, pts, tex, w, h, FILTER))
        assert np.isfinite(got).all()
        zeroed = np.where(np.isfinite(vals), vals, F(0)).astype(F)
        assert lc.same_bits(got, binding.filter_lightmap_host(lib, w, h, kind, FILTER, pts, tex, zeroed))


# ---- checks that do not rest on the restatement ----
@pytest.fixture(scope="module")
def two_charts(lib):
    """Two unit quads 20 world units apart whose charts are the left and the right half of a 16 x 16 atlas: neighbours there, without a gutter between them."""
    from raylib_amd import binding
    up = np.tile([[0.0, 1.0, 0.0]], (3, 1))
    tris = []
    for x0, u0 in ((0.0, 0.0), (20.0, 0.5)):
        a, b, c, d = [x0, 0, 0], [x0 + 1, 0, 0], [x0 + 1, 0, -1], [x0, 0, -1]
        tris.append(([a, b, c], up, [u0, 0, u0 + 0.5, 0, u0 + 0.5, 1]))
        tris.append(([a, c, d], up, [u0, 0, u0 + 0.5, 1, u0, 1]))
    scene, close = lc.triangle_scene(lib, tris)
    pts, tex, n = binding.lightmap_points(lib, scene, 16, 16, None, host=True)
    assert n == 256
    in_a = pts[:, 0] < 10
    assert in_a.sum() == 128 and (np.abs(pts[in_a][:, None, 0] - pts[~in_a][None, :, 0]) >= 10).all()
    yield pts, tex, in_a
    close()


def test_charts_apart_in_the_world_are_independent(lib, two_charts):
    """sigmaPosition 0.01 and >= 10 units between the charts: dp * invP_i >= 100 / 0.32^2 ~ 977 for every i < 6, and expf of anything below -104 is +0, so a tap in
    the other chart weighs exactly nothing."""
    from raylib_amd import binding
    pts, tex, in_a = two_charts
    for kind in (0, 1):
        filt = (6, 10.0, 10.0, 0.01)
        vals = fc.synthetic_values(256, kind, seed=3)
        base = binding.filter_lightmap_host(lib, 16, 16, kind, filt, pts, tex, vals)
        big = vals.copy(); big[in_a] *= F(1000)
        got = binding.filter_lightmap_host(lib, 16, 16, kind, filt, pts, tex, big)
        assert lc.same_bits(got[~in_a], base[~in_a])
        assert not lc.same_bits(got[in_a], base[in_a])
        bad = vals.copy(); bad[np.nonzero(in_a)[0][37], 1] = np.nan; bad[np.nonzero(in_a)[0][90], 0] = np.inf
        got = binding.filter_lightmap_host(lib, 16, 16, kind, filt, pts, tex, bad)
        assert lc.same_bits(got[~in_a], base[~in_a])
        assert np.isfinite(got).all()


def test_a_flat_chart_is_smoothed(lib, two_charts):
    """One flat chart, one normal, value 1 plus noise, a colour tolerance far wider than the noise: the variance falls, the mean stays.  With equal range weights
    a step replaces a texel by the k x k average of independent noise, whose variance is sum(k^2)^2 / sum(k)^4 of the input's: 0.075 inside, 0.19 in a corner
    (three taps per axis) -- half the input's is a bound with room."""
    from raylib_amd import binding
    pts, tex, in_a = two_charts
    rng = np.random.default_rng(11)
    for kind in (0, 1):
        c = fc.CHANNELS[kind]
        vals = (1.0 + rng.normal(0.0, 0.1, (256, c))).astype(F)
        got = binding.filter_lightmap_host(lib, 16, 16, kind, (3, 1e3, 1.0, 1.0), pts, tex, vals)
        nf = 3 if kind == 0 else c
        for grp in (in_a, ~in_a):
            for ch in range(nf):
                assert got[grp, ch].astype(np.float64).var() < 0.5 * vals[grp, ch].astype(np.float64).var(), (kind, ch)
                assert abs(got[grp, ch].astype(np.float64).mean() - 1.0) < 0.05


def test_in_place(lib, points_of):
    from raylib_amd import binding
    w, h = 61, 47
    pts, tex = points_of(w, h)
    for kind in (0, 1):
        vals = fc.synthetic_values(len(tex), kind, seed=9)
        want = binding.filter_lightmap_host(lib, w, h, kind, FILTER, pts, tex, vals)
        work = vals.copy()
        got = binding.filter_lightmap_host(lib, w, h, kind, FILTER, pts, tex, work, in_place=True)
        assert got is work and lc.same_bits(work, want) and not lc.same_bits(work, vals)


def test_record_layout(lib):
    from raylib_amd import binding
    P = binding.LightmapFilterParams
    assert C.sizeof(P) == 16
    assert [getattr(P, f).offset for f in ("iterations", "sigmaColor", "sigmaNormal", "sigmaPosition")] == [0, 4, 8, 12]
    for name in ("RaylibAMD_BakeLightmapFiltered", "RaylibAMD_BakeLightmapFilteredDevice", "RaylibAMD_FilterLightmap", "RaylibAMD_FilterLightmapDevice",
                 "RaylibAMD_FilterLightmapHost"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


BAD_FILTERS = [(0, 1, 1, 1), (9, 1, 1, 1), (-1, 1, 1, 1), (2, float("nan"), 1, 1), (2, 1, float("inf"), 1), (2, 1, 1, float("nan")), (2, 5e-4, 1, 1), (2, 1, 2e3, 1),
               (2, 1, 1, 0.0), (2, 1, 1, -1.0), (2, -1.0, 1, 1), (2, 1, 1, 1.5e3)]


def test_host_refusals(lib, points_of):
    """Every refusal of RaylibAMD_FilterLightmapHost: 0, nothing written."""
    from raylib_amd import binding
    w, h = 61, 47
    pts, tex = points_of(w, h)
    n = 50
    pts, tex = np.ascontiguousarray(pts[:n]), np.ascontiguousarray(tex[:n])
    vals = fc.synthetic_values(n, 1, seed=1)
    out = np.full((n, 27), 7.0, F)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    pp = lambda a: a.ctypes.data_as(C.POINTER(binding.GatherPoint))
    tp = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    good = binding.LightmapFilterParams(2, 1.0, 1.0, 1.0)

    def call(width=w, height=h, kind=1, flt=good, points=pts, texel=tex, count=n, values=vals, dst=out):
        return lib.RaylibAMD_FilterLightmapHost(width, height, kind, C.byref(flt) if flt is not None else None, pp(points) if points is not None else None,
                                                tp(texel) if texel is not None else None, count, fp(values) if values is not None else None,
                                                fp(dst) if dst is not None else None)
    for kw in (dict(points=None), dict(texel=None), dict(values=None), dict(dst=None), dict(count=-1), dict(kind=2), dict(kind=-1), dict(flt=None),
               dict(width=0), dict(width=16385), dict(height=0), dict(height=16385), dict(height=-5)):
        assert call(**kw) == 0, kw
    for b in BAD_FILTERS:
        assert call(flt=binding.LightmapFilterParams(*b)) == 0, b
    for k, v in ((3, tex[2]), (3, tex[1]), (n - 1, w * h), (0, 0xffffffff)):   # equal, descending, outside, far outside
        t = tex.copy(); t[k] = v
        assert call(texel=t) == 0, (k, v)
    assert call(width=7, height=5) == 0                               # the texels do not fit that atlas
    assert (out == 7.0).all()
    # accepted: nothing to do without a point -- null arrays included --, and the good call
    assert call(count=0) == 1 and call(count=0, points=None, texel=None, values=None, dst=None) == 1
    assert (out == 7.0).all()
    assert call() == 1 and not (out == 7.0).any()


def test_device_entries_check_their_arguments_first(lib, cornell):
    """What the four device-side entries refuse of the filter and of `in`: 0 and nothing written, with or without a device."""
    from raylib_amd import binding
    ses, uv = cornell
    out = np.full((8, 8, 27), 7.0, F); cov = np.full((8, 8), 7, np.uint8); src = np.full((8, 8, 27), 3.0, F)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
    cp = cov.ctypes.data_as(C.POINTER(C.c_uint8))
    uvp = fp(uv)

    def calls(scene, prm, flt, src_=src, dst=out):
        p = C.byref(prm) if prm is not None else None
        f = C.byref(flt) if flt is not None else None
        return [lib.RaylibAMD_BakeLightmapFiltered(scene, p, f, uvp, fp(dst), cp), lib.RaylibAMD_BakeLightmapFilteredDevice(scene, p, f, uvp, fp(dst), cp, None),
                lib.RaylibAMD_FilterLightmap(scene, p, f, uvp, fp(src_), fp(dst), cp), lib.RaylibAMD_FilterLightmapDevice(scene, p, f, uvp, fp(src_), fp(dst), cp, None)]
    good = binding.LightmapFilterParams(2, 1.0, 1.0, 1.0)
    prm = binding.lightmap_params(8, 8, 1, max_path=3)
    for b in BAD_FILTERS:
        assert calls(ses.scene, prm, binding.LightmapFilterParams(*b)) == [0, 0, 0, 0], b
    assert calls(ses.scene, prm, None) == [0, 0, 0, 0]
    assert calls(ses.scene, None, good) == [0, 0, 0, 0] and calls(None, prm, good) == [0, 0, 0, 0]
    assert calls(ses.scene, prm, good, dst=None) == [0, 0, 0, 0]
    assert lib.RaylibAMD_FilterLightmap(ses.scene, C.byref(prm), C.byref(good), uvp, None, fp(out), cp) == 0                 # no `in`
    assert lib.RaylibAMD_FilterLightmapDevice(ses.scene, C.byref(prm), C.byref(good), uvp, None, fp(out), cp, None) == 0
    for kw in (dict(kind=2), dict(dilate=65), dict(tri_count=0), dict(skip_draws=63), dict(sample_count=0), dict(time=float("nan"))):   # as a bake checks them
        assert calls(ses.scene, binding.lightmap_params(8, 8, **dict(dict(kind=1, max_path=3), **kw)), good) == [0, 0, 0, 0], kw
    assert calls(ses.scene, binding.lightmap_params(0, 8, 1), good) == [0, 0, 0, 0]
    assert (out == 7.0).all() and (cov == 7).all() and (src == 3.0).all()
