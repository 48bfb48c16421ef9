"""Triangle-overlap queries (RaylibAMD_OverlapTriangles, include/raylib_amd.h statements O1 to O6) without a device: the host oracle
RaylibAMD_OverlapTrianglesHost against a float32 NumPy restatement of the statements (tests/overlap_cases.py), byte for byte; against an independent
double-precision reference (an edge of one triangle pierces the other) on generic pairs; constructed cases on small-integer coordinates, where all arithmetic
is exact; the shape of LIST rows; the refusals; the planner (csrc/rl_plan.cc PlanOverlap) under RAYLIB_QUERY_TREE.  tests/test_gpu_overlap.py holds the device
to the oracle byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers  # noqa: F401
from helpers import scenes, ffi
import overlap_cases as oc
import stack_edges as se
from raylib_amd import binding

TREE_BVH2, TREE_GRID4 = 1, 3
CANARY = 0x5a5a5a5a


@pytest.fixture(scope="module")
def S(lib, workdir):
    d = os.path.join(str(workdir), "overlap_host"); os.makedirs(d, exist_ok=True)
    out = {"soup": oc.session(lib, oc.write_soup(os.path.join(d, "soup.obj"), 500)),
           "doubled": oc.session(lib, oc.write_soup(os.path.join(d, "doubled.obj"), 200, seed=5, doubled=True)),
           "cornell": oc.session(lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
           "quad": oc.session(lib, oc.write_soup(os.path.join(d, "quad.obj"), 2, seed=1))}
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _host(lib, ses, q, kind, flags=0, max_hits=16, count=True):
    return binding.overlap_triangles(lib, ses.scene, q, kind, flags, max_hits, host=True, count=count)


def _scene_of(lib, workdir, name, T):
    d = os.path.join(str(workdir), "overlap_host"); os.makedirs(d, exist_ok=True)
    ses = oc.session(lib, oc.write_triangles(os.path.join(d, name + ".obj"), T))
    assert np.array_equal(oc.tri_array(ses.export_flat()[0]), np.asarray(T, np.float32)), "the export order is the file's"
    return ses


def test_record_layout_and_exports(lib):
    assert binding.OVERLAP_QUERY_DTYPE.itemsize == 48
    assert [binding.OVERLAP_QUERY_DTYPE.fields[f][1] for f in ("v0", "reserved0", "v1", "reserved1", "v2", "reserved2")] == [0, 12, 16, 28, 32, 44]
    assert (binding.OVERLAP_ANY, binding.OVERLAP_LIST, binding.OVERLAP_SKIP_SHARED, binding.MAX_OVERLAPS) == (0, 1, 1, 16)
    for name in ("RaylibAMD_OverlapTriangles", "RaylibAMD_OverlapTrianglesDevice", "RaylibAMD_OverlapTrianglesHost", "RaylibAMD_PlanOverlap"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


def test_oracle_is_the_restatement_byte_for_byte(lib, S):
    """500 triangles x about 400 queries -- the soup's own triangles, those jittered, random triangles from 0.01 to 2 times the extent, the specials -- for both
    kinds and both flag values; the reserved words are not read."""
    tris, _ = S["soup"].export_flat()
    assert len(tris) == 500
    q = oc.query_set(np.random.RandomState(17), tris, 400)
    q["reserved0"], q["reserved1"], q["reserved2"] = 0xffffffff, 0x7fc00000, 12345
    for flags in (0, oc.SKIP_SHARED):
        assert _host(lib, S["soup"], q, oc.ANY, flags).tobytes() == oc.restate(q, tris, oc.ANY, flags).tobytes(), flags
        for k in (1, 16):
            rows, counts = _host(lib, S["soup"], q, oc.LIST, flags, k)
            want_rows, want_counts = oc.restate(q, tris, oc.LIST, flags, k)
            assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), (flags, k)
        assert 0.1 < (want_counts > 0).mean() < 0.9, "the set must cut"
    # the flag takes away a triangle's meeting with itself: the unmoved own triangles are the first quarter
    plain, shared = oc.restate(q, tris, oc.LIST, 0)[1], oc.restate(q, tris, oc.LIST, oc.SKIP_SHARED)[1]
    assert (plain[:100] >= 1).all() and (shared[:100] < plain[:100]).all()


def test_oracle_against_the_piercing_reference_on_generic_pairs(lib, workdir):
    """4096 generic pairs, each in a grid cell of its own (one scene of the T, one call with the Q; no other triangle is near): O4 in float32 against "an edge of
    one pierces the other" in float64.  A pair may disagree only when the float64 gap of O4's axes, normalised by the axis' length, is within 1e-5 of zero, and
    such pairs may be at most 1 % of the set.  (On these pairs no pair disagrees.)"""
    Q, T = oc.generic_pairs(np.random.RandomState(5), 4096)
    ses = _scene_of(lib, workdir, "pairs", T)
    try:
        rows, counts = _host(lib, ses, oc.as_queries(Q), oc.LIST)
    finally:
        ses.close()
    k = np.arange(len(Q))
    assert ((rows[:, 0] == k) | (rows[:, 0] == -1)).all() and (counts <= 1).all(), "a query meets its own partner or nothing"
    got, want = counts == 1, oc.pierce64(Q, T)
    assert 0.1 < want.mean() < 0.25, "about a sixth of the pairs meet: %.3f" % want.mean()
    differ = np.nonzero(got != want)[0]
    gaps = np.array([oc.pair_matrix(Q[i:i + 1], T[i:i + 1], dtype=np.float64, with_gap=True)[1][0, 0] for i in differ])
    print("pairs: %d, meeting %.3f, disagreeing %d, their gaps %r" % (len(Q), want.mean(), len(differ), gaps))
    assert (np.abs(gaps) <= 1e-5).all(), "a pair disagrees away from the boundary: %r" % [(int(i), float(g)) for i, g in zip(differ, gaps)]
    assert len(differ) <= len(Q) // 100


# Constructed cases on small-integer coordinates: every product, sum and difference is exact
A = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
CASES = [
    # (what, query, scene triangle, accepted, accepted with the flag)
    ("a triangle against itself", A, A, True, False),
    ("an edge neighbour", A, [(4, 0, 0), (0, 4, 0), (4, 4, 2)], True, False),
    ("a vertex neighbour", A, [(4, 0, 0), (8, 0, 0), (8, 4, 2)], True, False),
    ("a piercing pair", A, [(1, 1, -2), (1, 1, 2), (5, 5, 2)], True, True),
    ("touching at one vertex", A, [(1, 1, 0), (1, 1, 3), (3, 1, 3)], True, True),
    ("parallel planes one unit apart", [(4, 0, 0), (0, 4, 0), (0, 0, 4)], [(5, 0, 0), (0, 5, 0), (0, 0, 5)], False, False),   # (x + y + z = 4 and = 5)
    ("coplanar nested", A, [(1, 1, 0), (2, 1, 0), (1, 2, 0)], True, True),
    ("coplanar disjoint, boxes that meet", A, [(4, 4, 0), (4, 3, 0), (3, 4, 0)], False, False),
    ("boxes apart", A, [(9, 9, 9), (10, 9, 9), (9, 10, 9)], False, False),
]


@pytest.mark.parametrize("what,Q,T,accepted,with_flag", CASES, ids=[c[0] for c in CASES])
def test_constructed_cases(lib, workdir, what, Q, T, accepted, with_flag):
    far = [(100, 100, 100), (101, 100, 100), (100, 101, 100)]   # (a second triangle: the scene is never a single leaf's worth of nothing)
    ses = _scene_of(lib, workdir, "case_%d" % [c[0] for c in CASES].index(what), np.array([T, far], np.float32))
    try:
        q = oc.as_queries(np.array([Q], np.float32))
        lo, hi = np.min(Q, 0), np.max(Q, 0)
        if what != "boxes apart":
            assert (lo <= np.max(T, 0)).all() and (np.min(T, 0) <= hi).all(), "the case is decided behind O2"
        for flags, want in ((0, accepted), (oc.SKIP_SHARED, with_flag)):
            assert _host(lib, ses, q, oc.ANY, flags)[0] == int(want), (what, flags)
            rows, counts = _host(lib, ses, q, oc.LIST, flags, 4)
            assert rows[0].tolist() == ([0, -1, -1, -1] if want else [-1] * 4) and counts[0] == int(want), (what, flags)
            assert oc.restate(q, ses.export_flat()[0], oc.ANY, flags)[0] == int(want)
        if accepted and with_flag:
            assert oc.pierce64(np.array([Q], float), np.array([T], float))[0] or "coplanar" in what
    finally:
        ses.close()


def test_doubled_soup_lists_both_copies_lower_index_first(lib, S):
    tris, _ = S["doubled"].export_flat()
    assert len(tris) == 400
    T = oc.tri_array(tris)
    key = [t.tobytes() for t in T]
    twin = {}
    for k, b in enumerate(key):
        twin.setdefault(b, []).append(k)
    assert len(twin) == 200 and all(len(v) == 2 for v in twin.values()), "each triangle is present twice"
    q = oc.as_queries(T[::2])
    rows, counts = _host(lib, S["doubled"], q, oc.LIST)
    assert rows.tobytes() == oc.restate(q, tris, oc.LIST, 0)[0].tobytes()
    for i, row in enumerate(rows):
        listed = row[row >= 0].tolist()
        a, b = twin[key[2 * i]]
        assert a in listed and b in listed and listed.index(a) < listed.index(b), (i, listed)
        assert counts[i] % 2 == 0, "whatever meets one copy meets the other"
    assert (_host(lib, S["doubled"], q, oc.LIST, oc.SKIP_SHARED)[1] < counts).all()


def test_list_shape(lib, S):
    tris, _ = S["soup"].export_flat()
    q = oc.query_set(np.random.RandomState(29), tris, 400)
    full = oc.pair_matrix(oc.query_array(q), oc.tri_array(tris)) & np.isfinite(oc.query_array(q).reshape(len(q), 9)).all(1)[:, None]
    for k in (1, 16):
        rows, counts = _host(lib, S["soup"], q, oc.LIST, 0, k)
        assert rows.shape == (len(q), k)
        assert (counts > k).any(), "the set must hold queries with count > maxHits"
        assert (counts == 0).any() and ((counts > 0) & (counts < k + 1)).any()
        for row, c, acc in zip(rows, counts, full):
            listed = int((row >= 0).sum())
            assert (row[:listed] >= 0).all() and (row[listed:] == -1).all(), "-1 only behind the entries"
            assert (np.diff(row[:listed]) > 0).all(), "ascending"
            assert listed == min(k, c) and c >= listed
            assert row[:listed].tolist() == np.nonzero(acc)[0][:k].tolist()
        assert _host(lib, S["soup"], q, oc.LIST, 0, k, count=False).tobytes() == rows.tobytes(), "the rows do not depend on outCount"
        assert np.array_equal(_host(lib, S["soup"], q, oc.ANY), (counts > 0).astype(np.uint32))


def test_special_values(lib, S):
    for name in ("soup", "cornell"):
        tris, _ = S[name].export_flat()
        q, what = oc.specials(tris)
        rows, counts = _host(lib, S[name], q, oc.LIST)
        want_rows, want_counts = oc.restate(q, tris, oc.LIST, 0)
        assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes()
        hits = _host(lib, S[name], q, oc.ANY)
        got = dict(zip(what, counts))
        for w in ("a NaN vertex", "an inf vertex", "a -inf vertex", "a query far outside", "a point 1e30 away"):
            assert got[w] == 0 and hits[what.index(w)] == 0 and (rows[what.index(w)] == -1).all(), w
        for w in ("a point-sized query at a scene vertex", "a segment-sized query along a scene edge", "a scene triangle itself", "a 1e30 vertex"):
            assert got[w] >= 1 and hits[what.index(w)] == 1, w
        assert got["a query that contains the whole scene"] == len(tris) and hits[what.index("a query that contains the whole scene")] == 1
        assert 0 < got["a query whose box contains the scene"] < len(tris)
        flagged = _host(lib, S[name], q, oc.LIST, oc.SKIP_SHARED)[1]
        assert flagged[what.index("a point-sized query at a scene vertex")] < got["a point-sized query at a scene vertex"]


def test_refusals(lib, S):
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    prims = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)],
                                      [dict(minBounds=(1, 0, 0), maxBounds=(1.5, 0.5, 0.5), timeStartMove=0.0, velocity=(0.0, 0.0, 0.0), material=0)])
    raw = lib.Raylib_CreateScene()
    q = oc.as_queries(np.array([[(0, 0, 0), (1, 0, 0), (0, 1, 0)]] * 3, np.float32))
    scene = S["soup"].scene
    try:
        for entry in ("RaylibAMD_OverlapTrianglesHost", "RaylibAMD_OverlapTriangles", "RaylibAMD_OverlapTrianglesDevice"):
            f = getattr(lib, entry)
            tail = (None,) if entry.endswith("Device") else ()
            out, cnt = np.full(3 * 16, CANARY, np.uint32), np.full(3, CANARY, np.uint32)
            qp, op, cp = q.ctypes.data, out.ctypes.data, cnt.ctypes.data
            cases = [("spheres and cubes", (prims.scene, oc.LIST, 0, qp, 3, 4, op, cp)), ("spheres and cubes, ANY", (prims.scene, oc.ANY, 0, qp, 3, 4, op, None)),
                     ("unknown kind", (scene, 2, 0, qp, 3, 4, op, None)), ("kind -1", (scene, -1, 0, qp, 3, 4, op, None)),
                     ("n < 0", (scene, oc.LIST, 0, qp, -1, 4, op, cp)), ("n < 0, ANY", (scene, oc.ANY, 0, qp, -1, 4, op, None)),
                     ("flag bit 1", (scene, oc.LIST, 2, qp, 3, 4, op, cp)), ("flag bit 31", (scene, oc.ANY, 0x80000001, qp, 3, 4, op, None)),
                     ("maxHits 0", (scene, oc.LIST, 0, qp, 3, 0, op, cp)), ("maxHits 17", (scene, oc.LIST, 0, qp, 3, 17, op, cp)),
                     ("maxHits -1", (scene, oc.LIST, 1, qp, 3, -1, op, None)), ("n * maxHits above 2^31 - 1", (scene, oc.LIST, 0, qp, 0x7fffffff, 2, op, cp)),
                     ("ANY with outCount", (scene, oc.ANY, 0, qp, 3, 4, op, cp)),
                     ("not finalized", (raw, oc.LIST, 0, qp, 3, 4, op, cp)), ("null q", (scene, oc.LIST, 0, None, 3, 4, op, cp)),
                     ("null scene", (None, oc.LIST, 0, qp, 3, 4, op, cp))]
            for what, args in cases:
                assert f(*(args + tail)) == 0, (entry, what)
                assert (out == CANARY).all() and (cnt == CANARY).all(), (entry, what)
            assert f(*((scene, oc.LIST, 0, qp, 3, 4, None, cp) + tail)) == 0 and (cnt == CANARY).all(), (entry, "null out")
        # ANY does not read maxHits
        out = np.full(3, CANARY, np.uint32)
        for k in (0, -5, 17, 1 << 30):
            assert lib.RaylibAMD_OverlapTrianglesHost(scene, oc.ANY, 0, q.ctypes.data, 3, k, out.ctypes.data, None) == 1
        assert lib.RaylibAMD_OverlapTrianglesHost(scene, oc.LIST, 0, None, 0, 4, None, None) == 1, "n == 0 returns 1"
        for kind in (oc.ANY, oc.LIST):
            p = binding.QueryPlan()
            assert lib.RaylibAMD_PlanOverlap(prims.scene, kind, C.byref(p)) == 0 and lib.RaylibAMD_PlanOverlap(raw, kind, C.byref(p)) == 0
            assert lib.RaylibAMD_PlanOverlap(scene, kind, None) == 0 and lib.RaylibAMD_PlanOverlap(None, kind, C.byref(p)) == 0
        assert lib.RaylibAMD_PlanOverlap(scene, 2, C.byref(binding.QueryPlan())) == 0
    finally:
        lib.Raylib_DestroyScene(raw)
        prims.close()


@pytest.mark.parametrize("env,cornell_tree", [(None, TREE_GRID4), ("2", TREE_BVH2), ("4", TREE_GRID4), ("8", TREE_GRID4)])
def test_plan_overlap(lib, S, monkeypatch, env, cornell_tree):
    if env is not None:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", env)
    assert lib.RaylibAMD_SceneNumTriangles(S["quad"].scene) < 8
    for kind in (oc.ANY, oc.LIST):
        rc, p = binding.plan_overlap(lib, S["cornell"].scene, kind)
        assert rc == 1
        want = (TREE_GRID4, 4, 64, 32) if cornell_tree == TREE_GRID4 else (TREE_BVH2, 2, 64, 32)
        assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"]) == want, p
        assert (p["prims"], p["early"]) == (0, int(kind == oc.ANY)), p
        rc, p = binding.plan_overlap(lib, S["quad"].scene, kind)   # fewer than 8 triangles: no wide tree, whatever is asked for
        assert rc == 1 and (p["tree"], p["treeWidth"], p["stack"], p["early"]) == (TREE_BVH2, 2, 32, int(kind == oc.ANY)), p


# the default: the grid-4 tree while its walk is the 32-deep instance, else the binary tree (tests/stack_edges.py: depth 32 / need 32, depth 21 / need 33)
@pytest.mark.parametrize("name,env,width,stack", [("cone_d32", None, 4, 32), ("cone_n33", None, 2, 32), ("cone_n33", "4", 4, 64), ("cone_n33", "2", 2, 32), ("cone_d32", "2", 2, 32)])
def test_plan_overlap_by_the_grid_walks_stack(lib, workdir, monkeypatch, name, env, width, stack):
    spec = se.SCENES[name]
    ses, _ = se.make_session(lib, spec, os.path.join(str(workdir), "overlap_plan"), name)
    try:
        tn = se.tree_numbers(lib, ses.scene)
        assert (tn["depth"], tn["need4"]) == (spec["depth"], spec["need4"]), tn
        if env is not None:
            monkeypatch.setenv("RAYLIB_QUERY_TREE", env)
        for kind in (oc.ANY, oc.LIST):
            rc, p = binding.plan_overlap(lib, ses.scene, kind)
            assert rc == 1 and (p["treeWidth"], p["stack"]) == (width, stack), p
    finally:
        ses.close()
