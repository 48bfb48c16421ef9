"""The lightmap rasteriser without a device (RaylibAMD_LightmapPointsHost, include/raylib_amd.h): the host oracle against the NumPy restatement of the
header's statements 1 to 6 (tests/lightmap_cases.py) bit for bit, on two scenes, two UV generators, three atlases and constructed edge inputs; checks that do
not rest on the restatement (the point lies under its texel's centre, closed-form coverage counts); the record layout; every refusal."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from helpers import scenes
import lightmap_cases as lc

F = np.float32
ATLASES = lc.ATLASES
_triangle_scene = lc.triangle_scene


@pytest.fixture(scope="module")
def cornells(lib, workdir):
    """tess -> (session, triangles): the 36-triangle Cornell box and its 5184-triangle tessellation."""
    from raylib_amd import binding
    d = os.path.join(str(workdir), "lightmap_host"); os.makedirs(d, exist_ok=True)
    out = {}
    for tess in (1, 12):
        ses = binding.SceneSession(lib, scenes.cornell(os.path.join(d, "cornell%d.obj" % tess), tess=tess)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
        out[tess] = (ses, lc.scene_triangles(lib, ses.scene))
    assert len(out[1][1]) == 36 and len(out[12][1]) == 5184
    yield out
    for ses, _ in out.values():
        ses.close()


def _check(lib, ses, tris, w, h, uv, what, **kw):
    from raylib_amd import binding
    got_p, got_t, n = binding.lightmap_points(lib, ses.scene, w, h, uv, host=True, **kw)
    first, count = kw.get("tri_first", 0), kw.get("tri_count", -1)
    sub = tris[first:] if count < 0 else tris[first:first + count]
    want_p, want_t, owner = lc.points(sub, uv, w, h, kw.get("time", 0.0))
    assert n == len(want_t), (what, n, len(want_t))
    assert np.array_equal(got_t, want_t), what
    assert lc.same_bits(got_p, want_p), what
    assert np.array_equal(np.ascontiguousarray(got_p[:, 7]).view(np.uint32), got_t), what     # the stream is the texel's index
    return got_p, got_t, owner


@pytest.mark.parametrize("atlas", ATLASES, ids=lambda a: "%dx%d" % a)
@pytest.mark.parametrize("gen", ["grid", "own"])
@pytest.mark.parametrize("tess", [1, 12])
def test_oracle_is_the_restatement(lib, cornells, tess, gen, atlas):
    ses, tris = cornells[tess]
    uv = lc.grid_uv(len(tris)) if gen == "grid" else None
    pts, tex, owner = _check(lib, ses, tris, atlas[0], atlas[1], uv, (tess, gen, atlas), time=0.25)
    assert (pts[:, 3] == F(0.25)).all()
    if atlas != (1, 1):
        assert len(tex) > 0
    if gen == "own":
        # every quad's chart is the whole unit square: the 18 charts overlap, and the first quad's triangles, the lowest indices, win everywhere
        assert owner.max() < 2 * tess * tess and (owner >= 0).all()


@pytest.mark.parametrize("name", sorted(lc.edge_inputs()))
def test_edge_inputs(lib, cornells, name):
    ses, tris = cornells[1]
    w, h, uv = lc.edge_inputs(len(tris))[name]
    pts, tex, owner = _check(lib, ses, tris, w, h, uv, name)
    if name == "vertex_on_centre":
        assert owner[3, 2] == 3                                     # the vertex's own texel: edges and corners are inclusive
    if name.startswith("shared_edge"):
        lo = min(k for k in range(len(uv)) if uv[k].any())
        assert (owner[np.arange(8), np.arange(8)] == lo).all()       # the diagonal's texels: owned once, by the lower index
        assert len(np.unique(tex)) == len(tex) == (owner >= 0).sum() == 64
    if name == "overlap_lowest_wins":
        assert owner[1, 1] == 2 and owner[5, 5] == 5 and owner[14, 0] == 7
    if name == "zero_area":
        assert set(np.unique(owner)) == {-1, 2}
    if name == "nan_uv":
        assert set(np.unique(owner)) == {-1, 2}
    if name == "far_outside_skipped":
        assert set(np.unique(owner)) == {-1, 2}
    if name == "far_outside_clipped":
        assert (owner >= 0).all() and owner[0, 0] == 5 and owner[7, 7] == 0 and owner[3, 0] == 1
    if name == "box_is_whole_atlas":
        assert (owner == 6).all() and len(tex) == 13 * 7
    if name == "negative_area":
        assert (owner >= 0).sum() == 36                              # x + y <= 7 on 8 x 8: the winding does not matter


def test_big_and_small(lib, cornells):
    ses, tris = cornells[12]
    w, h, uv = lc.big_and_small(len(tris))
    pts, tex, owner = _check(lib, ses, tris, w, h, uv, "big and small")
    assert len(tex) == w * h and (owner == len(tris) - 1).sum() > 0 and (owner < len(tris) - 1).sum() > 100


def test_sub_range_and_capacity(lib, cornells):
    from raylib_amd import binding
    ses, tris = cornells[12]
    uv = lc.grid_uv(len(tris))
    full_p, full_t, _ = _check(lib, ses, tris, 61, 47, uv[100:300], "sub-range", tri_first=100, tri_count=200)
    _check(lib, ses, tris, 61, 47, uv[5000:], "to the end", tri_first=5000, tri_count=-1)
    # capacity below the count: the count is returned whole, the first `capacity` records are written and nothing behind them
    n = len(full_t)
    assert n > 10
    prm = binding.lightmap_params(61, 47, tri_first=100, tri_count=200)
    buf = np.full((n, 8), 7.0, F); tex = np.full(n, 7, np.uint32)
    sub = np.ascontiguousarray(uv[100:300])
    got = lib.RaylibAMD_LightmapPointsHost(ses.scene, C.byref(prm), sub.ctypes.data_as(C.POINTER(C.c_float)), buf.ctypes.data_as(C.POINTER(binding.GatherPoint)),
                                           tex.ctypes.data_as(C.POINTER(C.c_uint32)), 10)
    assert got == n
    assert lc.same_bits(buf[:10], full_p[:10]) and np.array_equal(tex[:10], full_t[:10]) and (buf[10:] == 7.0).all() and (tex[10:] == 7).all()
    assert lib.RaylibAMD_LightmapPointsHost(ses.scene, C.byref(prm), sub.ctypes.data_as(C.POINTER(C.c_float)), None, None, 0) == n      # a count alone
    got = lib.RaylibAMD_LightmapPointsHost(ses.scene, C.byref(prm), sub.ctypes.data_as(C.POINTER(C.c_float)), buf.ctypes.data_as(C.POINTER(binding.GatherPoint)), None, n)
    assert got == n and lc.same_bits(buf, full_p)                                                                                      # no texel indices wanted


def test_face_fallback_and_empty_texels(lib):
    """Zero vertex normals fall back to the face; a degenerate face or a position that is not finite leaves the texel empty, and an empty texel does not
    pass to the next triangle."""
    from raylib_amd import binding
    flat = [[0, 0, 0], [1, 0, 0], [0, 0, -1]]
    chart = [0, 0, 1, 0, 0, 1]
    zero, up = np.zeros((3, 3)), np.tile([[0.0, 1.0, 0.0]], (3, 1))
    cancel = [[0, 1, 0], [0, -1, 0], [0, -1, 0]]
    scene, close = _triangle_scene(lib, [
        ([[0, 0, 0], [1, 0, 0], [2, 0, 0]], zero, chart),           # 0: collinear in space, zero normals: every texel it owns is empty
        (flat, zero, [0, 0, 2, 0, 0, 2]),                           # 1: zero normals -> cross(e1, e2) = (0, 1, 0)
        (flat, up, [0, 0, 2, 0, 0, 2]),
        ([[-3e38, 0, 0], [3e38, 0, 0], [0, 0, -1]], up, [1, 1, 0.5, 1, 1, 0.5]),   # 3: an edge that overflows: positions that are not finite
        (flat, cancel, [0.5, 1, 1, 0.5, 1, 1]),                     # 4: normals that cancel along an edge
    ])
    try:
        class S:
            pass
        ses = S(); ses.scene = scene
        tris = lc.scene_triangles(lib, scene)
        assert len(tris) == 5
        pts, tex, owner = _check(lib, ses, tris, 16, 16, None, "fallback")
        by_owner = owner.ravel()[tex]
        assert (owner == 0).sum() > 0 and not (by_owner == 0).any()          # triangle 0 owns texels and none of them has a point
        assert (owner[tex // 16, tex % 16] == by_owner).all()
        one = pts[by_owner == 1]
        assert len(one) > 0 and (one[:, 4:7] == np.array([0, 1, 0], F)).all()            # (a zero may be -0: the cross product's)
        assert not (by_owner == 3).any() or np.isfinite(pts[by_owner == 3][:, :3]).all()
        assert np.isfinite(pts[:, :7]).all()
    finally:
        close()


@pytest.mark.parametrize("tess", [1, 12])
def test_point_lies_under_its_texel(lib, cornells, tess):
    """Without the restatement: the UV re-derived in double from a point's position, in its owner's plane, is the texel's centre to within the snap (1/256 texel:
    half a sub-texel step per corner, less than doubled by the interpolation) plus the float rounding of the position -- three roundings of about eps * |v|
    each against an edge of length |e|, a relative error in the barycentrics of under 16 eps |v|max / |e|min, times the chart's extent in texels."""
    from raylib_amd import binding
    ses, tris = cornells[tess]
    uv = lc.grid_uv(len(tris))
    w, h = 61, 47
    pts, tex, _ = binding.lightmap_points(lib, ses.scene, w, h, uv, host=True)
    owner = lc.owners(uv, w, h).ravel()[tex]
    assert len(tex) > 1000
    v = tris["v"][owner].astype(np.float64)
    e1, e2, p = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], pts[:, :3].astype(np.float64) - v[:, 0]
    a, b, c = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (p * e1).sum(1), (p * e2).sum(1)
    det = a * c - b * b
    b1, b2 = (r1 * c - r2 * b) / det, (r2 * a - r1 * b) / det
    t = uv[owner].astype(np.float64).reshape(-1, 3, 2) * [w, h]
    at = t[:, 0] + b1[:, None] * (t[:, 1] - t[:, 0]) + b2[:, None] * (t[:, 2] - t[:, 0])
    centre = np.stack([tex % w + 0.5, tex // w + 0.5], 1)
    extent = np.abs(t - t[:, :1]).max((1, 2))
    tol = 1.0 / 256 + 16 * np.finfo(F).eps * np.abs(v).max((1, 2)) / np.sqrt(np.minimum(a, c)) * extent
    err = np.abs(at - centre).max(1)
    assert (err <= tol).all(), (float(err.max()), float(tol.min()))


def test_closed_form_coverage(lib, cornells):
    from raylib_amd import binding
    ses, tris = cornells[1]
    uv = np.zeros((len(tris), 6), F)
    uv[0] = [0, 0, 1, 0, 0, 1]
    _, tex, n = binding.lightmap_points(lib, ses.scene, 64, 64, uv, host=True)
    assert n == 64 * 65 // 2                       # centres with (x + .5) + (y + .5) <= 64: the diagonal's 64 included
    assert ((tex % 64) + (tex // 64) <= 63).all() and (((tex % 64) + (tex // 64)) == 63).sum() == 64
    uv[0] = [0, 0, 1, 0, 1, 1]; uv[1] = [0, 0, 1, 1, 0, 1]  # a one-pair chart over the whole atlas covers every texel, the diagonal's once
    for w, h in ((64, 64), (61, 47), (1, 1)):
        _, tex, n = binding.lightmap_points(lib, ses.scene, w, h, uv, host=True)
        assert n == w * h and np.array_equal(tex, np.arange(w * h, dtype=np.uint32))


def test_record_layout(lib):
    from raylib_amd import binding
    P = binding.LightmapParams
    assert C.sizeof(P) == 56
    assert [getattr(P, f).offset for f in ("width", "height", "triFirst", "triCount", "dilate", "time", "gather")] == [0, 4, 8, 12, 16, 20, 24]
    for name in ("RaylibAMD_LightmapPoints", "RaylibAMD_LightmapPointsHost", "RaylibAMD_BakeLightmap", "RaylibAMD_BakeLightmapDevice"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


def test_refusals(lib, cornells):
    """Every refusal of the header: -1 from the two points calls, 0 from the two bakes, nothing written -- before a call looks for a device."""
    from raylib_amd import binding
    ses, tris = cornells[1]
    n_tris = len(tris)
    pts = np.full((64, 8), 7.0, F); tex = np.full(64, 7, np.uint32)
    out = np.full((8, 8, 27), 7.0, F); cov = np.full((8, 8), 7, np.uint8)
    pp, tp = pts.ctypes.data_as(C.POINTER(binding.GatherPoint)), tex.ctypes.data_as(C.POINTER(C.c_uint32))
    op, cp = out.ctypes.data_as(C.POINTER(C.c_float)), cov.ctypes.data_as(C.POINTER(C.c_uint8))
    good = dict(width=8, height=8, triFirst=0, triCount=-1, dilate=1, time=0.0)
    ggood = dict(kind=0, maxPathLength=3, rayTMin=1e-4, sampleFirst=0, sampleCount=1, skipDraws=0, timeMin=0.0, timeMax=0.0)

    def prm(**kw):
        g = binding.GatherParams(**dict(ggood, **{k: v for k, v in kw.items() if k in ggood}))
        return binding.LightmapParams(gather=g, **dict(good, **{k: v for k, v in kw.items() if k in good}))

    def calls(scene, p, points=pp, bake_out=op, capacity=64):
        pr = C.byref(p) if p is not None else None
        return [lib.RaylibAMD_LightmapPoints(scene, pr, None, points, tp, capacity), lib.RaylibAMD_LightmapPointsHost(scene, pr, None, points, tp, capacity),
                lib.RaylibAMD_BakeLightmap(scene, pr, None, bake_out, cp), lib.RaylibAMD_BakeLightmapDevice(scene, pr, None, bake_out, cp, None)]
    refused = [-1, -1, 0, 0]
    bad = [dict(width=0), dict(width=16385), dict(height=0), dict(height=-3), dict(height=16385), dict(dilate=-1), dict(dilate=65),
           dict(triFirst=-1), dict(triFirst=n_tris), dict(triCount=0), dict(triCount=-2), dict(triCount=n_tris + 1), dict(triFirst=30, triCount=7),
           dict(time=float("nan")), dict(time=float("inf")),
           dict(kind=2), dict(kind=-1), dict(skipDraws=63), dict(sampleCount=0), dict(rayTMin=-1e-4), dict(rayTMin=float("nan")), dict(maxPathLength=-1),
           dict(maxPathLength=32769)]
    for b in bad:
        assert calls(ses.scene, prm(**b)) == refused, b
    assert calls(None, prm()) == refused
    assert calls(ses.scene, None) == refused
    unfinished = lib.Raylib_CreateScene()
    assert calls(unfinished, prm()) == refused
    lib.Raylib_DestroyScene(unfinished)
    g = prm()
    for points, capacity in ((None, 64), (pp, -1)):                      # no room for the points: the two points calls alone (the parameters are a valid bake's)
        assert lib.RaylibAMD_LightmapPoints(ses.scene, C.byref(g), None, points, tp, capacity) == -1
        assert lib.RaylibAMD_LightmapPointsHost(ses.scene, C.byref(g), None, points, tp, capacity) == -1
    if lib.RaylibAMD_DeviceAvailable():                                  # ... which, with a device, bakes: into buffers of its own
        out2 = np.full((8, 8, 27), 7.0, F); cov2 = np.full((8, 8), 7, np.uint8)
        assert lib.RaylibAMD_BakeLightmap(ses.scene, C.byref(g), None, out2.ctypes.data_as(C.POINTER(C.c_float)), cov2.ctypes.data_as(C.POINTER(C.c_uint8))) == 1
        assert not (cov2 == 7).any()                                     # (every texel's coverage byte is written: 0, 1 or 2)
    assert lib.RaylibAMD_BakeLightmap(ses.scene, C.byref(g), None, None, cp) == 0 and lib.RaylibAMD_BakeLightmapDevice(ses.scene, C.byref(g), None, None, cp, None) == 0
    scene, close = _triangle_scene(lib, [])                              # a scene without triangles: every range is empty
    assert calls(scene, prm()) == refused
    close()
    assert (pts == 7.0).all() and (tex == 7).all() and (out == 7.0).all() and (cov == 7).all()


def test_no_covered_texel_is_a_success(lib, cornells):
    """Nothing covered: the oracle returns 0 points, with no device."""
    from raylib_amd import binding
    ses, tris = cornells[1]
    uv = np.full((len(tris), 6), 5.0, F)                                 # every chart outside the atlas
    uv[:, 2] = 6.0; uv[:, 5] = 6.0
    pts, tex, n = binding.lightmap_points(lib, ses.scene, 16, 16, uv, host=True)
    assert n == 0 and len(pts) == 0


def test_pair_budget(lib, cornells):
    """More than 2^36 (triangle, texel) pairs are refused: 5184 triangles whose boxes are a whole 16384 x 16384 atlas are 2^40.  At 2^36 exactly -- 256 such
    triangles -- the call is not refused by the budget (not run here: it would test 2^36 pairs); 2 of them on 1024 x 1024 are run."""
    from raylib_amd import binding
    ses, tris = cornells[12]
    uv = np.tile(np.array([[-0.5, -0.5, 2.5, -0.5, -0.5, 2.5]], F), (len(tris), 1))
    with pytest.raises(RuntimeError):
        binding.lightmap_points(lib, ses.scene, 16384, 16384, uv, host=True, capacity=0)
    with pytest.raises(RuntimeError):
        binding.lightmap_points(lib, ses.scene, 16384, 16384, uv[:257], tri_count=257, host=True, capacity=0)
    _, _, n = binding.lightmap_points(lib, ses.scene, 1024, 1024, uv[:2], tri_count=2, host=True, capacity=0)
    assert n == 1024 * 1024
