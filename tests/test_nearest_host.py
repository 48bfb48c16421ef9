"""Nearest-point queries (RaylibAMD_NearestPoints, include/raylib_amd.h statements N1 to N5) without a device: the host oracle RaylibAMD_NearestPointsHost
against a float32 NumPy restatement of the statements (tests/nearest_cases.py), bit for bit; the tie rule on a soup that holds every triangle twice; the
definition itself against a float64 brute force; the special values; the refusals; the planner (csrc/rl_plan.cc PlanNearest) under RAYLIB_QUERY_TREE.
tests/test_gpu_nearest.py holds the device to the oracle byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers  # noqa: F401
from helpers import scenes, ffi
import nearest_cases as nc

TREE_BVH2, TREE_GRID4 = 1, 3


@pytest.fixture(scope="module")
def S(lib, workdir):
    d = os.path.join(str(workdir), "nearest_host"); os.makedirs(d, exist_ok=True)
    out = {"soup": nc.session(lib, nc.write_soup(os.path.join(d, "soup.obj"), 2000)),
           "doubled": nc.session(lib, nc.write_soup(os.path.join(d, "doubled.obj"), 500, seed=5, doubled=True)),
           "soup0": nc.session(lib, nc.write_soup(os.path.join(d, "soup0.obj"), 600, seed=9)),
           "soup100": nc.session(lib, nc.write_soup(os.path.join(d, "soup100.obj"), 600, seed=9, offset=100.0)),
           "cornell": nc.session(lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
           "quad": nc.session(lib, nc.write_soup(os.path.join(d, "quad.obj"), 2, seed=1))}
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _host(lib, ses, pts, kind):
    from raylib_amd import binding
    return binding.nearest_points(lib, ses.scene, pts, kind, host=True)


def _same_records(got, want, what):
    for f in ("dist2", "prim", "b1", "b2"):
        bad = np.nonzero(got[f].view(np.uint32) != want[f].view(np.uint32))[0]
        assert bad.size == 0, "%s: %s differs at %d points, first %d: %r against %r" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])


def test_record_layouts_and_exports(lib):
    from raylib_amd import binding
    assert binding.NEAREST_QUERY_DTYPE.itemsize == 16 and binding.NEAREST_DTYPE.itemsize == 16
    assert [binding.NEAREST_DTYPE.fields[f][1] for f in ("dist2", "prim", "b1", "b2")] == [0, 4, 8, 12]
    assert (binding.NEAREST_WITHIN, binding.NEAREST_CLOSEST) == (0, 1)
    for name in ("RaylibAMD_NearestPoints", "RaylibAMD_NearestPointsDevice", "RaylibAMD_NearestPointsHost", "RaylibAMD_PlanNearest"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


def test_oracle_is_the_restatement_bit_for_bit(lib, S):
    """2000 triangles, 400 points -- random, on triangles, at vertices and on edges, 1e-4 off surfaces -- with maxDist +inf, a finite radius, and each point's own
    distance as the radius (D <= R2 at equality or an ulp beside it)."""
    tris, _ = S["soup"].export_flat()
    assert len(tris) == 2000
    pts = nc.point_set(np.random.RandomState(17), tris, 400)
    want, within, _ = nc.restate(pts, tris)
    assert (want["prim"] >= 0).all()
    _same_records(_host(lib, S["soup"], pts, nc.CLOSEST), want, "maxDist +inf")
    assert np.array_equal(_host(lib, S["soup"], pts, nc.WITHIN), within)
    own = np.sqrt(want["dist2"].astype(np.float64))
    for name, md in (("the median distance", np.full(len(pts), np.median(own))), ("its own distance", own), ("just below its own distance", own * (1 - 1e-6)),
                     ("just above its own distance", own * (1 + 1e-6)), ("zero", np.zeros(len(pts)))):
        q = nc.with_max_dist(pts, md.astype(np.float32))
        want_q, within_q, _ = nc.restate(q, tris)
        _same_records(_host(lib, S["soup"], q, nc.CLOSEST), want_q, name)
        assert np.array_equal(_host(lib, S["soup"], q, nc.WITHIN), within_q), name
        assert np.array_equal(within_q, (want_q["prim"] >= 0).astype(np.uint32))
    # the radii cut: the median radius finds about half the points a triangle, and a radius of zero only the points that lie on one up to rounding
    assert 100 < nc.restate(nc.with_max_dist(pts, np.float32(np.median(own))), tris)[1].sum() < 300


def test_doubled_soup_ties_go_to_the_lower_index(lib, S):
    tris, _ = S["doubled"].export_flat()
    assert len(tris) == 1000
    key = [t.tobytes() for t in np.stack([tris["v0"], tris["v1"], tris["v2"]], 1)]
    first = {}
    for k, b in enumerate(key):
        first.setdefault(b, k)
    assert len(first) == 500, "each triangle is present twice"
    pts = nc.point_set(np.random.RandomState(23), tris, 400)
    want, _, ties = nc.restate(pts, tris)
    assert (ties >= 2).sum() >= len(pts) // 2, "the input must tie: %d of %d points have their least D attained twice" % ((ties >= 2).sum(), len(pts))
    got = _host(lib, S["doubled"], pts, nc.CLOSEST)
    _same_records(got, want, "doubled soup")
    assert all(first[key[p]] == p for p in got["prim"]), "a winner is not the lower of its two indices"


def test_definition_against_float64_brute_force(lib, S):
    """|sqrt(dist2) - d64| <= 16 * 2^-23 * (the largest |coordinate| of the point and the scene): N3 and float32 move the distance at rounding level only.
    The bound's 16 has a margin of about 7 over the 2.2 units measured with the NumPy restatement on soups at offsets 0 and 100 when the call was specified;
    worst seen by this test: 0.95 units (offset 0) and 0.65 (offset 100).  The failure message carries the worst value."""
    worst = {}
    for name in ("soup0", "soup100"):
        tris, _ = S[name].export_flat()
        pts = nc.point_set(np.random.RandomState(31), tris, 300)
        got = _host(lib, S[name], pts, nc.CLOSEST)
        d64 = nc.brute64(pts, tris)
        scene_max = max(np.abs(tris[f]).max() for f in ("v0", "v1", "v2"))
        unit = 2.0 ** -23 * np.maximum(np.abs(pts[:, :3]).max(1), scene_max)
        err = np.abs(np.sqrt(got["dist2"].astype(np.float64)) - d64) / unit
        worst[name] = float(err.max())
    print("worst |sqrt(dist2) - d64| in units of 2^-23 * scale:", worst)
    assert max(worst.values()) <= 16.0, "worst error in units of 2^-23 * the largest coordinate: %r" % worst


def test_special_values(lib, S):
    tris, _ = S["soup"].export_flat()
    pts, what = nc.special_points(tris)
    want, within, _ = nc.restate(pts, tris)
    got = _host(lib, S["soup"], pts, nc.CLOSEST)
    _same_records(got, want, "special values")
    assert np.array_equal(_host(lib, S["soup"], pts, nc.WITHIN), within)
    row = {w: got[i] for i, w in enumerate(what)}
    miss = (0.0, -1, 0.0, 0.0)
    for w in ("NaN x", "NaN y", "+inf z", "-inf x", "maxDist NaN", "maxDist -1", "maxDist -0.0 off the surface", "1e25 away, maxDist 1e10"):
        assert row[w].tolist() == miss, (w, row[w])
    for w in ("maxDist -0.0 at a v0 vertex", "maxDist 0 at a v0 vertex"):
        assert row[w]["prim"] >= 0 and row[w]["dist2"] == 0.0, (w, row[w])
    for w in ("maxDist +inf", "maxDist 3e38"):
        assert row[w]["prim"] >= 0 and 0.0 < row[w]["dist2"] < 1.0, (w, row[w])
    assert row["maxDist +inf"].tobytes() == row["maxDist 3e38"].tobytes()
    # every distance is +inf: the least index among them
    for w in ("1e25 away, maxDist +inf", "1e25 away, maxDist 3e38"):
        assert row[w]["prim"] == 0 and row[w]["dist2"] == np.inf, (w, row[w])


def test_refusals(lib, S):
    from raylib_amd import binding
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    prims = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)],
                                      [dict(minBounds=(1, 0, 0), maxBounds=(1.5, 0.5, 0.5), timeStartMove=0.0, velocity=(0.0, 0.0, 0.0), material=0)])
    raw = lib.Raylib_CreateScene()
    pts = np.array([[0, 0, 0, np.inf]] * 3, np.float32)
    scene = S["soup"].scene
    try:
        for entry in ("RaylibAMD_NearestPointsHost", "RaylibAMD_NearestPoints"):
            f = getattr(lib, entry)
            for kind in (nc.WITHIN, nc.CLOSEST):
                out = np.full(3 * 4, 0x5a5a5a5a, np.uint32)
                cases = [("spheres and cubes", (prims.scene, kind, pts.ctypes.data, 3, out.ctypes.data)), ("unknown kind", (scene, 2, pts.ctypes.data, 3, out.ctypes.data)),
                         ("kind -1", (scene, -1, pts.ctypes.data, 3, out.ctypes.data)), ("n < 0", (scene, kind, pts.ctypes.data, -1, out.ctypes.data)),
                         ("not finalized", (raw, kind, pts.ctypes.data, 3, out.ctypes.data)), ("null points", (scene, kind, None, 3, out.ctypes.data)),
                         ("null scene", (None, kind, pts.ctypes.data, 3, out.ctypes.data))]
                for what, args in cases:
                    assert f(*args) == 0, (entry, what)
                    assert (out == 0x5a5a5a5a).all(), (entry, what)
                assert f(scene, kind, pts.ctypes.data, 3, None) == 0, (entry, "null out")
        for kind in (nc.WITHIN, nc.CLOSEST):
            assert lib.RaylibAMD_NearestPointsHost(scene, kind, None, 0, None) == 1, "n == 0 returns 1"
            out = np.full(4, 0x5a5a5a5a, np.uint32)
            assert lib.RaylibAMD_NearestPointsDevice(prims.scene, kind, pts.ctypes.data, 1, out.ctypes.data, None) == 0 and (out == 0x5a5a5a5a).all()
            p = binding.QueryPlan()
            assert lib.RaylibAMD_PlanNearest(prims.scene, kind, C.byref(p)) == 0 and lib.RaylibAMD_PlanNearest(raw, kind, C.byref(p)) == 0
            assert lib.RaylibAMD_PlanNearest(scene, kind, None) == 0
        assert lib.RaylibAMD_PlanNearest(scene, 2, C.byref(binding.QueryPlan())) == 0
    finally:
        lib.Raylib_DestroyScene(raw)
        prims.close()


@pytest.mark.parametrize("env,cornell_tree", [(None, TREE_GRID4), ("2", TREE_BVH2), ("4", TREE_GRID4), ("8", TREE_GRID4)])
def test_plan_nearest(lib, S, monkeypatch, env, cornell_tree):
    from raylib_amd import binding
    if env is not None:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", env)
    assert lib.RaylibAMD_SceneNumTriangles(S["quad"].scene) < 8
    for kind in (nc.WITHIN, nc.CLOSEST):
        rc, p = binding.plan_nearest(lib, S["cornell"].scene, kind)
        assert rc == 1
        want = (TREE_GRID4, 4, 64, 32) if cornell_tree == TREE_GRID4 else (TREE_BVH2, 2, 64, 32)
        assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"]) == want, p
        assert (p["prims"], p["early"]) == (0, int(kind == nc.WITHIN)), p
        rc, p = binding.plan_nearest(lib, S["quad"].scene, kind)   # fewer than 8 triangles: no wide tree, whatever is asked for
        assert rc == 1 and (p["tree"], p["treeWidth"], p["stack"], p["early"]) == (TREE_BVH2, 2, 32, int(kind == nc.WITHIN)), p
