"""Swept-sphere queries (RaylibAMD_SweepSpheres, include/raylib_amd.h statements W1 to W7) without a device: the host oracle RaylibAMD_SweepSpheresHost against a
float32 NumPy restatement of the statements (tests/sweep_cases.py), byte for byte; the tie rule on a soup that holds every triangle twice; ANY against
CLOSEST; a zero move against RaylibAMD_NearestPointsHost WITHIN; the special values; the refusals; the planner; and the statements' geometry against float64
point-triangle and segment-triangle distances that share nothing with W4.  tests/test_gpu_sweep.py holds the device to the oracle byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers  # noqa: F401
from helpers import scenes, ffi
import nearest_cases as nc
import sweep_cases as sc

TREE_BVH2, TREE_GRID4 = 1, 3
GEOMETRY_K = 1.0   # test_geometry_against_float64: 4 x the largest k measured, rounded up to a power of two


@pytest.fixture(scope="module")
def S(lib, workdir):
    d = os.path.join(str(workdir), "sweep_host"); os.makedirs(d, exist_ok=True)
    out = {"cornell": sc.session(lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
           "soup": sc.session(lib, sc.write_soup(os.path.join(d, "soup.obj"), 2000)),
           "doubled": sc.session(lib, sc.write_soup(os.path.join(d, "doubled.obj"), 500, seed=5, doubled=True)),
           "quad": sc.session(lib, sc.write_soup(os.path.join(d, "quad.obj"), 2, seed=1))}
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def R(lib, S):
    """Per scene: its triangles, 700 queries, the oracle's two answers and the restatement's -- computed once, shared, left unchanged."""
    out = {}
    for name in ("cornell", "soup", "doubled"):
        tris, _ = S[name].export_flat()
        q = sc.query_set(np.random.RandomState(17), tris, 700)
        want, any_want, ties = sc.restate(q, tris)
        out[name] = dict(tris=tris, q=q, closest=_host(lib, S[name], q, sc.CLOSEST), any=_host(lib, S[name], q, sc.ANY), want=want, any_want=any_want, ties=ties)
    return out


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _host(lib, ses, q, kind):
    from raylib_amd import binding
    return binding.sweep_spheres(lib, ses.scene, q, kind, host=True)


def _same_records(got, want, what):
    for f in ("t", "prim", "feature", "reserved0", "point", "reserved1"):
        a, b = got[f].view(np.uint32).reshape(len(got), -1), want[f].view(np.uint32).reshape(len(want), -1)
        bad = np.nonzero((a != b).any(1))[0]
        assert bad.size == 0, "%s: %s differs at %d queries, first %d: %r against %r" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])


def test_record_layouts_and_exports(lib):
    from raylib_amd import binding
    assert binding.SWEEP_QUERY_DTYPE.itemsize == 32 and binding.SWEEP_HIT_DTYPE.itemsize == 32
    assert [binding.SWEEP_QUERY_DTYPE.fields[f][1] for f in ("origin", "radius", "delta", "reserved")] == [0, 12, 16, 28]
    assert [binding.SWEEP_HIT_DTYPE.fields[f][1] for f in ("t", "prim", "feature", "reserved0", "point", "reserved1")] == [0, 4, 8, 12, 16, 28]
    assert (binding.SWEEP_ANY, binding.SWEEP_CLOSEST) == (0, 1)
    for name in ("RaylibAMD_SweepSpheres", "RaylibAMD_SweepSpheresDevice", "RaylibAMD_SweepSpheresHost", "RaylibAMD_PlanSweep"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


@pytest.mark.parametrize("name", ["cornell", "soup", "doubled"])
def test_oracle_is_the_restatement_byte_for_byte(R, name):
    r = R[name]
    _same_records(r["closest"], r["want"], name)
    assert r["closest"].tobytes() == r["want"].tobytes()
    assert np.array_equal(r["any"], r["any_want"])
    hit = r["closest"]["prim"] >= 0
    assert np.array_equal(r["any"] == 1, hit), "ANY is prim >= 0 of CLOSEST"
    assert 0.2 < hit.mean() < 0.9, "the moves must cut: %.2f hit" % hit.mean()
    miss = r["closest"][~hit]
    assert (miss.view(np.uint32).reshape(len(miss), 8)[:, [0, 2, 3, 4, 5, 6, 7]] == 0).all(), "a miss: prim = -1, every other word 0"
    t = r["closest"]["t"][hit]
    assert (t >= 0).all() and (t <= 1).all() and not np.signbit(t).any()
    seen = set(r["closest"]["feature"][hit].tolist())
    assert seen <= set(range(8)) and {0, 7} <= seen and len(seen) >= 6, seen


def test_doubled_soup_ties_go_to_the_lower_index(R):
    r = R["doubled"]
    tris = r["tris"]
    assert len(tris) == 1000
    key = [t.tobytes() for t in np.stack([tris["v0"], tris["v1"], tris["v2"]], 1)]
    first = {}
    for k, b in enumerate(key):
        first.setdefault(b, k)
    assert len(first) == 500, "each triangle is present twice"
    hit = r["closest"]["prim"] >= 0
    assert (r["ties"][hit] >= 2).all(), "every hit's least T is attained at least twice"
    assert all(first[key[p]] == p for p in r["closest"]["prim"][hit]), "a winner is not the lower of its two indices"


def test_a_zero_move_is_within(lib, S, R):
    """delta == 0 leaves W3 alone: ANY answers as RaylibAMD_NearestPointsHost WITHIN with maxDist = radius."""
    from raylib_amd import binding
    for name in ("cornell", "soup"):
        q = R[name]["q"].copy()
        q[:, 4:7] = 0
        q[::2, 4:7] = np.float32(-0.0)
        got = _host(lib, S[name], q, sc.ANY)
        pts = np.concatenate([q[:, 0:3], q[:, 3:4]], 1)
        want = binding.nearest_points(lib, S[name].scene, pts, nc.WITHIN, host=True)
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:5])
        assert 0.05 < got.mean() < 0.95, got.mean()
        rec = _host(lib, S[name], q, sc.CLOSEST)
        assert (rec["feature"][rec["prim"] >= 0] == 7).all() and (rec["t"] == 0).all()


def test_special_values(lib, S):
    from raylib_amd import binding
    for name in ("cornell", "soup"):
        tris, _ = S[name].export_flat()
        q, what = sc.special_queries(tris)
        want, any_want, _ = sc.restate(q, tris)
        got = _host(lib, S[name], q, sc.CLOSEST)
        _same_records(got, want, "special values")
        assert np.array_equal(_host(lib, S[name], q, sc.ANY), any_want)
        row = {w: got[i] for i, w in enumerate(what)}
        miss = np.zeros(1, binding.SWEEP_HIT_DTYPE); miss["prim"] = -1
        for w in ("NaN origin", "NaN delta", "NaN radius", "+inf origin", "-inf delta", "+inf radius", "negative radius", "1e30 away"):
            assert row[w].tobytes() == miss.tobytes(), (w, row[w])
        assert row["a denormal move"].tobytes() == row["a zero move"].tobytes(), "denormal components are read as 0"
        if name == "cornell":   # (there the space above the triangle is free)
            assert row["a zero move"].tobytes() == miss.tobytes()
            for w in ("towards the triangle", "along -x", "along +y"):
                assert row[w]["prim"] >= 0 and 0 < row[w]["t"] < 1 and row[w]["feature"] != 7, (w, row[w])
        assert row["the move's least component 1e-42"].tobytes() == row["the move's least component 0"].tobytes(), "a denormal component is read as 0"
        assert row["the move's least component 0"]["prim"] >= 0
        for w in ("radius -0.0 on a vertex, zero move", "radius 0 on a vertex, move -0.0", "origin exactly on a vertex", "origin exactly on a vertex, radius 0"):
            assert row[w]["prim"] >= 0 and row[w]["t"] == 0 and row[w]["feature"] == 7, (w, row[w])
        # a move that ends exactly at first contact is a hit: T <= 1 at equality
        cut = sc.ending_at_contact(lib, S[name], tris)
        assert len(cut) >= 1
        _same_records(_host(lib, S[name], cut, sc.CLOSEST), sc.restate(cut, tris)[0], "ending at contact")


def test_refusals(lib, S):
    from raylib_amd import binding
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    prims = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)],
                                      [dict(minBounds=(1, 0, 0), maxBounds=(1.5, 0.5, 0.5), timeStartMove=0.0, velocity=(0.0, 0.0, 0.0), material=0)])
    raw = lib.Raylib_CreateScene()
    q = np.array([[0, 0, 0, 0.1, 1, 0, 0, 0]] * 3, np.float32)
    scene = S["soup"].scene
    try:
        for entry in ("RaylibAMD_SweepSpheresHost", "RaylibAMD_SweepSpheres"):
            f = getattr(lib, entry)
            for kind in (sc.ANY, sc.CLOSEST):
                out = np.full(3 * 8, 0x5a5a5a5a, np.uint32)
                cases = [("spheres and cubes", (prims.scene, kind, q.ctypes.data, 3, out.ctypes.data)), ("unknown kind", (scene, 2, q.ctypes.data, 3, out.ctypes.data)),
                         ("kind -1", (scene, -1, q.ctypes.data, 3, out.ctypes.data)), ("n < 0", (scene, kind, q.ctypes.data, -1, out.ctypes.data)),
                         ("not finalized", (raw, kind, q.ctypes.data, 3, out.ctypes.data)), ("null queries", (scene, kind, None, 3, out.ctypes.data)),
                         ("null scene", (None, kind, q.ctypes.data, 3, out.ctypes.data))]
                for what, args in cases:
                    assert f(*args) == 0, (entry, what)
                    assert (out == 0x5a5a5a5a).all(), (entry, what)
                assert f(scene, kind, q.ctypes.data, 3, None) == 0, (entry, "null out")
        for kind in (sc.ANY, sc.CLOSEST):
            assert lib.RaylibAMD_SweepSpheresHost(scene, kind, None, 0, None) == 1, "n == 0 returns 1"
            out = np.full(8, 0x5a5a5a5a, np.uint32)
            assert lib.RaylibAMD_SweepSpheresDevice(prims.scene, kind, q.ctypes.data, 1, out.ctypes.data, None) == 0 and (out == 0x5a5a5a5a).all()
            p = binding.QueryPlan()
            assert lib.RaylibAMD_PlanSweep(prims.scene, kind, C.byref(p)) == 0 and lib.RaylibAMD_PlanSweep(raw, kind, C.byref(p)) == 0
            assert lib.RaylibAMD_PlanSweep(scene, kind, None) == 0
        assert lib.RaylibAMD_PlanSweep(scene, 2, C.byref(binding.QueryPlan())) == 0
    finally:
        lib.Raylib_DestroyScene(raw)
        prims.close()


@pytest.mark.parametrize("env,cornell_tree", [(None, TREE_GRID4), ("2", TREE_BVH2), ("4", TREE_GRID4), ("8", TREE_GRID4)])
def test_plan_sweep(lib, S, monkeypatch, env, cornell_tree):
    from raylib_amd import binding
    if env is not None:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", env)
    for kind in (sc.ANY, sc.CLOSEST):
        rc, p = binding.plan_sweep(lib, S["cornell"].scene, kind)
        assert rc == 1
        want = (TREE_GRID4, 4, 64, 32) if cornell_tree == TREE_GRID4 else (TREE_BVH2, 2, 64, 32)
        assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"]) == want, p
        assert (p["prims"], p["early"]) == (0, int(kind == sc.ANY)), p
        # PlanNearest's trees and stacks under RAYLIB_QUERY_TREE; without it PlanOverlap's default (the grid-4 tree only while the 32-deep instance fits)
        for name in ("cornell", "soup", "doubled"):
            ref = binding.plan_nearest(lib, S[name].scene, nc.CLOSEST)[1] if env is not None else binding.plan_overlap(lib, S[name].scene, 0)[1]
            assert binding.plan_sweep(lib, S[name].scene, kind)[1] == ref | {"early": int(kind == sc.ANY)}, (name, env)
        rc, p = binding.plan_sweep(lib, S["quad"].scene, kind)   # fewer than 8 triangles: no wide tree, whatever is asked for
        assert rc == 1 and (p["tree"], p["treeWidth"], p["stack"], p["early"]) == (TREE_BVH2, 2, 32, int(kind == sc.ANY)), p


def test_plan_sweep_default_leaves_a_64_deep_grid_tree(lib, workdir, monkeypatch):
    """A scene whose grid-4 walk needs the 64-deep instance (tests/stack_edges.py cone_d33): by default the binary tree, the grid nodes when asked for."""
    from raylib_amd import binding
    import stack_edges as se
    spec = se.SCENES["cone_d33"]
    ses, _ = se.make_session(lib, spec, os.path.join(str(workdir), "sweep_plan"), "cone_d33")
    try:
        rc, p = binding.plan_sweep(lib, ses.scene, sc.CLOSEST)
        assert rc == 1 and (p["treeWidth"], p["stack"]) == (2, 64), p
        monkeypatch.setenv("RAYLIB_QUERY_TREE", "4")
        rc, p = binding.plan_sweep(lib, ses.scene, sc.CLOSEST)
        assert rc == 1 and (p["treeWidth"], p["stack"]) == (4, 64), p
    finally:
        ses.close()


def test_geometry_against_float64(R):
    """The oracle against float64 point-triangle and segment-triangle distances, with tol = k * 2^-23 * (scene extent + |o| + |d| + r) and c(T) = o + T d:
      - every hit with feature != 7: |dist(c(T), triangle prim) - r| <= tol;
      - every hit: the distance from the segment [o, c(T)] to EVERY triangle is >= r - tol -- for a feature-7 hit the sphere touches at the start by
        definition and the path before the contact is empty, so what is checked there is that it does touch: dist(o, triangle prim) <= r + tol;
      - every miss: the distance from the whole move [o, o + d] to every triangle is >= r - tol.
    No query is left out; grazing moves are covered because the condition is on depth, not on time.  Largest k needed, measured on these inputs (cornell, the
    2000-triangle soup and the doubled soup, 700 queries each): 0.234 for the touching distance and for the clearance of a hit's path (the same query: its
    path ends where it touches), 0.058 for a start in contact, and no miss comes nearer than r at all -- far below the 64 at which the root form of W4
    would count as cancelling.  The test's k is 4 x 0.234 rounded up to a power of two: 1.  The failure message carries the measured values."""
    worst = {"touch": 0.0, "path": 0.0, "miss": 0.0, "start": 0.0}
    for name, r in R.items():
        tris, q, got = r["tris"], r["q"].astype(np.float64), r["closest"]
        _, _, ext = sc.extent_of(tris)
        V = [tris[f].astype(np.float64) for f in ("v0", "v1", "v2")]
        for i in range(len(q)):
            o, rad, d = q[i, 0:3], q[i, 3], q[i, 4:7]
            unit = 2.0 ** -23 * (ext + np.linalg.norm(o) + np.linalg.norm(d) + rad)
            if got["prim"][i] < 0:
                worst["miss"] = max(worst["miss"], float((rad - sc.segment_tri64(o, o + d, *V).min()) / unit))
                continue
            k, T = int(got["prim"][i]), float(got["t"][i])
            c = o + T * d
            touch = float(sc.point_tri64(c[None], V[0][k:k + 1], V[1][k:k + 1], V[2][k:k + 1])[0, 0])
            if got["feature"][i] == 7:
                worst["start"] = max(worst["start"], (touch - rad) / unit)
            else:
                worst["touch"] = max(worst["touch"], abs(touch - rad) / unit)
                worst["path"] = max(worst["path"], float((rad - sc.segment_tri64(o, c, *V).min()) / unit))
    print("largest k needed:", worst)
    assert max(worst.values()) <= GEOMETRY_K, "largest k needed, in units of 2^-23 * (extent + |o| + |d| + r): %r" % worst
