"""The K nearest triangles and the count in range (RaylibAMD_NearestPointsAll, include/raylib_amd.h statements K1 to K5) without a device: the host oracle
RaylibAMD_NearestPointsAllHost against a float32 NumPy restatement (tests/nearest_all_cases.py), byte for byte, on point sets whose radii cut every row
every way; its first record against CLOSEST's and its count against WITHIN; the order inside exact-D ties; the special values; the refusals; the planner
(csrc/rl_plan.cc PlanNearestAll) under RAYLIB_QUERY_TREE.  tests/test_gpu_nearest_all.py holds the device to the oracle byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers  # noqa: F401
from helpers import ffi
import nearest_cases as nc
import nearest_all_cases as na
from raylib_amd import binding

TREE_BVH2, TREE_GRID4 = 1, 3
MAX_HITS = (1, 2, 5, 16)
POISON = 0x5a5a5a5a


@pytest.fixture(scope="module")
def S(lib, workdir):
    d = os.path.join(str(workdir), "nearest_all_host")
    out = na.make_sessions(lib, d)
    out["quad"] = nc.session(lib, nc.write_soup(os.path.join(d, "quad.obj"), 2, seed=1))
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def base(S):
    """per scene: 200 points with maxDist +inf and the oracle's rows of 16 for them (computed once)"""
    return {name: na.base_points(S[name], 17 + k, 200) for k, name in enumerate(na.SCENES)}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def test_record_layouts_and_exports(lib):
    assert binding.MAX_NEAREST == 16
    for name in ("RaylibAMD_NearestPointsAll", "RaylibAMD_NearestPointsAllDevice", "RaylibAMD_NearestPointsAllHost", "RaylibAMD_PlanNearestAll"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


@pytest.mark.parametrize("name", na.SCENES)
@pytest.mark.parametrize("max_hits", MAX_HITS)
def test_oracle_is_the_restatement_byte_for_byte(lib, S, base, name, max_hits):
    ses = S[name]
    tris, _ = ses.export_flat()
    pts = na.calibrated(base[name], max_hits)
    rows, counts = na.oracle(lib, ses, pts, max_hits)
    na.check_classes(counts, max_hits, na.TWINS[name])
    want_rows, want_counts = na.restate(pts, tris, max_hits)
    na.same_rows(rows, want_rows, "%s, maxHits %d" % (name, max_hits))
    assert np.array_equal(counts, want_counts)
    na.same_rows(na.oracle(lib, ses, pts, max_hits, count=False), rows, "without the count")
    # K2: the listed part of a row is min(maxHits, count) long and sorted by (D, k); K2 and N4: its first record is CLOSEST's; K1 and N4: count > 0 is WITHIN
    listed = (rows["prim"] >= 0).sum(1)
    assert np.array_equal(listed, np.minimum(counts, max_hits))
    assert ((rows["prim"] >= 0) == (np.arange(max_hits)[None, :] < listed[:, None])).all(), "the miss records stand behind the listed ones"
    d, k = rows["dist2"].astype(np.float64), rows["prim"].astype(np.int64)
    both = (k[:, 1:] >= 0)
    assert (((d[:, :-1] < d[:, 1:]) | ((d[:, :-1] == d[:, 1:]) & (k[:, :-1] < k[:, 1:]))) | ~both).all()
    assert rows[:, 0].tobytes() == binding.nearest_points(lib, ses.scene, pts, nc.CLOSEST, host=True).tobytes()
    assert np.array_equal(counts > 0, binding.nearest_points(lib, ses.scene, pts, nc.WITHIN, host=True) == 1)


def test_max_hits_1_is_closest(lib, S, base):
    for name in na.SCENES:
        pts = base[name][0]
        rows = na.oracle(lib, S[name], pts, 1, count=False)
        assert rows.shape == (len(pts), 1)
        assert rows.tobytes() == binding.nearest_points(lib, S[name].scene, pts, nc.CLOSEST, host=True).tobytes()


def test_doubled_soup_tied_pairs_come_lower_index_first(lib, S, base):
    ses = S["doubled"]
    tris, _ = ses.export_flat()
    key = [t.tobytes() for t in np.stack([tris["v0"], tris["v1"], tris["v2"]], 1)]
    assert len(set(key)) == len(tris) // 2 == 500, "each triangle is present twice"
    rows = base["doubled"][1]
    pairs = 0
    for row in rows:
        for j in range(0, na.MAX, 2):   # every count is even and a twin has its twin's D: the row is a sequence of pairs
            a, b = row[j], row[j + 1]
            assert key[a["prim"]] == key[b["prim"]] and a["dist2"].tobytes() == b["dist2"].tobytes(), (a, b)
            assert a["prim"] < b["prim"], "a tied pair's higher index first: %r %r" % (a, b)
            assert (a["b1"].tobytes(), a["b2"].tobytes()) == (b["b1"].tobytes(), b["b2"].tobytes())
            pairs += 1
    assert pairs == 8 * len(rows)
    # a row cut inside a pair keeps the lower index
    odd = na.oracle(lib, ses, base["doubled"][0], 5, count=False)
    na.same_rows(odd, rows[:, :5], "maxHits 5 is the first five of maxHits 16")


def test_special_values(lib, S):
    ses = S["soup"]
    tris, _ = ses.export_flat()
    pts, what = nc.special_points(tris)
    for max_hits in (1, 4, 16):
        rows, counts = na.oracle(lib, ses, pts, max_hits)
        want_rows, want_counts = na.restate(pts, tris, max_hits)
        na.same_rows(rows, want_rows, "special values, maxHits %d" % max_hits)
        assert np.array_equal(counts, want_counts)
    rows, counts = na.oracle(lib, ses, pts, 4)
    at = {w: i for i, w in enumerate(what)}
    miss = (0.0, -1, 0.0, 0.0)
    for w in ("NaN x", "NaN y", "+inf z", "-inf x", "maxDist NaN", "maxDist -1"):
        assert counts[at[w]] == 0 and all(r.tolist() == miss for r in rows[at[w]]), (w, rows[at[w]], counts[at[w]])
    for w in ("maxDist -0.0 at a v0 vertex", "maxDist 0 at a v0 vertex"):
        row, n = rows[at[w]], int(counts[at[w]])
        assert n >= 1 and (row["dist2"][:min(n, 4)] == 0.0).all() and (row["prim"][min(n, 4):] == -1).all(), (w, row, n)
        assert (np.diff(row["prim"][:min(n, 4)]) > 0).all(), "D = 0 entries are ordered by index"
    # ... and more than one of them where the vertex belongs to two triangles: the doubled soup
    dtris, _ = S["doubled"].export_flat()
    dpts, dwhat = nc.special_points(dtris)
    drows, dcounts = na.oracle(lib, S["doubled"], dpts, 4)
    for w in ("maxDist -0.0 at a v0 vertex", "maxDist 0 at a v0 vertex"):
        i = dwhat.index(w)
        assert dcounts[i] == 2 and (drows[i]["dist2"][:2] == 0.0).all() and drows[i]["prim"][0] < drows[i]["prim"][1] and (drows[i]["prim"][2:] == -1).all(), (w, drows[i])
    # every distance is +inf and so is R2: the whole scene is in range, the lowest indices are listed
    w = "1e25 away, maxDist +inf"
    assert rows[at[w]]["prim"].tolist() == [0, 1, 2, 3] and (rows[at[w]]["dist2"] == np.inf).all() and counts[at[w]] == len(tris), (rows[at[w]], counts[at[w]])


def test_refusals_leave_the_outputs_untouched(lib, S):
    """Statement K5 without a device: every entry, nothing written.  (A BVH deeper than 64 levels cannot be had from the builder, which stops at 61; the pointer
    and alignment refusals of the device entry need a device: tests/test_gpu_nearest_all.py.)"""
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    prims = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)],
                                      [dict(minBounds=(1, 0, 0), maxBounds=(1.5, 0.5, 0.5), timeStartMove=0.0, velocity=(0.0, 0.0, 0.0), material=0)])
    raw = lib.Raylib_CreateScene()
    pts = np.array([[0, 0, 0, np.inf]] * 3, np.float32)
    scene = S["soup"].scene
    p = pts.ctypes.data
    try:
        for entry in ("RaylibAMD_NearestPointsAllHost", "RaylibAMD_NearestPointsAll"):
            f = getattr(lib, entry)
            out = np.full(3 * 16 * 4, POISON, np.uint32)
            cnt = np.full(3, POISON, np.uint32)
            o, c = out.ctypes.data, cnt.ctypes.data
            cases = [("spheres and cubes", (prims.scene, p, 3, 4, o, c)), ("maxHits 0", (scene, p, 3, 0, o, c)), ("maxHits -1", (scene, p, 3, -1, o, c)),
                     ("maxHits 17", (scene, p, 3, binding.MAX_NEAREST + 1, o, c)), ("n < 0", (scene, p, -1, 4, o, c)),
                     ("n * maxHits above 2^31 - 1", (scene, p, 0x7fffffff, 2, o, c)), ("n * maxHits = 2^31", (scene, p, 1 << 27, 16, o, c)),
                     ("not finalized", (raw, p, 3, 4, o, c)), ("null points", (scene, None, 3, 4, o, c)), ("null scene", (None, p, 3, 4, o, c))]
            for what, args in cases:
                assert f(*args) == 0, (entry, what)
                assert (out == POISON).all() and (cnt == POISON).all(), (entry, what)
            assert f(scene, p, 3, 4, None, c) == 0 and (cnt == POISON).all(), (entry, "null outHits")
        assert lib.RaylibAMD_NearestPointsAllHost(scene, None, 0, 4, None, None) == 1, "n == 0 returns 1"
        out = np.full(16, POISON, np.uint32)
        assert lib.RaylibAMD_NearestPointsAllDevice(prims.scene, p, 1, 4, out.ctypes.data, None, None) == 0 and (out == POISON).all()
        assert lib.RaylibAMD_NearestPointsAllDevice(scene, p, 1, 0, out.ctypes.data, None, None) == 0 and (out == POISON).all()
        # the planner's return codes, as RaylibAMD_PlanRayQueryAll's
        q = binding.QueryPlan()
        for count in (0, 1):
            assert lib.RaylibAMD_PlanNearestAll(prims.scene, 4, count, C.byref(q)) == 0 and lib.RaylibAMD_PlanNearestAll(raw, 4, count, C.byref(q)) == 0
            assert lib.RaylibAMD_PlanNearestAll(scene, 4, count, None) == 0 and lib.RaylibAMD_PlanNearestAll(None, 4, count, C.byref(q)) == 0
            assert lib.RaylibAMD_PlanNearestAll(scene, 0, count, C.byref(q)) == 0 and lib.RaylibAMD_PlanNearestAll(scene, binding.MAX_NEAREST + 1, count, C.byref(q)) == 0
            assert lib.RaylibAMD_PlanNearestAll(scene, 1, count, C.byref(q)) == 1 and lib.RaylibAMD_PlanNearestAll(scene, binding.MAX_NEAREST, count, C.byref(q)) == 1
    finally:
        lib.Raylib_DestroyScene(raw)
        prims.close()


@pytest.mark.parametrize("env,cornell_tree", [(None, TREE_GRID4), ("2", TREE_BVH2), ("4", TREE_GRID4), ("8", TREE_GRID4)])
def test_plan_nearest_all(lib, S, monkeypatch, env, cornell_tree):
    if env is not None:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", env)
    assert lib.RaylibAMD_SceneNumTriangles(S["quad"].scene) < 8
    for max_hits in (1, 4, 16):
        for count in (False, True):
            rc, p = binding.plan_nearest_all(lib, S["cornell"].scene, max_hits, count)
            assert rc == 1
            want = (TREE_GRID4, 4, 64, 32) if cornell_tree == TREE_GRID4 else (TREE_BVH2, 2, 64, 32)
            assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"]) == want, p
            assert (p["prims"], p["early"]) == (0, 0), p
            rc1, closest = binding.plan_nearest(lib, S["cornell"].scene, nc.CLOSEST)
            assert rc1 == 1 and all(p[f] == closest[f] for f in ("tree", "treeWidth", "nodeBytes", "stack")), (p, closest)
            rc, p = binding.plan_nearest_all(lib, S["quad"].scene, max_hits, count)   # fewer than 8 triangles: no wide tree, whatever is asked for
            assert rc == 1 and (p["tree"], p["treeWidth"], p["stack"], p["early"]) == (TREE_BVH2, 2, 32, 0), p
