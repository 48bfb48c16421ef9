"""Oriented-box range queries (RaylibAMD_OverlapBoxes, include/raylib_amd.h statements B1 to B6) without a device: the host oracle RaylibAMD_OverlapBoxesHost
against a float32 NumPy restatement of the statements (tests/box_cases.py), byte for byte, for all three kinds; the special values; the refusals; the planner
(csrc/rl_plan.cc PlanOverlapBoxes) against PlanOverlap; and the float32 verdict against a 13-axis separating-axis test in float64 away from the boundary.
tests/test_gpu_boxes.py holds the device to the oracle byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers  # noqa: F401
from helpers import scenes, ffi
import box_cases as bc
from raylib_amd import binding

CANARY = 0x5a5a5a5a
MAX_HITS = (1, 4, 16)


@pytest.fixture(scope="module")
def S(lib, workdir):
    d = os.path.join(str(workdir), "box_host"); os.makedirs(d, exist_ok=True)
    out = {"soup": bc.session(lib, scenes.soup(os.path.join(d, "soup.obj"), 10000)[0]),
           "cornell": bc.session(lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0])}
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def restated(S):
    """Per scene: the triangles, the query set and the restatement's complete accepted sets, computed once."""
    out = {}
    for name, n in (("soup", 300), ("cornell", 600)):
        tris, _ = S[name].export_flat()
        q = bc.query_set(np.random.RandomState(17), tris, n)
        q["reserved"] = np.arange(len(q)) * 2654435761 % (1 << 32)    # the reserved word is not read
        out[name] = (tris, q, bc.accepted_sets(q, tris), n)
    return out


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _host(lib, ses, q, kind, k=16, count=True):
    return binding.overlap_boxes(lib, ses.scene, q, kind, k, count=count, host=True)


def test_record_layout_and_exports(lib):
    D = binding.BOX_QUERY_DTYPE
    assert D.itemsize == 64 and [D.fields[f][1] for f in ("center", "reserved", "axis")] == [0, 12, 16]
    A = D.fields["axis"][0]
    assert A.shape == (3,) and A.base.itemsize == 16 and [A.base.fields[f][1] for f in ("dir", "half")] == [0, 12]
    assert (binding.BOX_ANY, binding.BOX_LIST, binding.BOX_MARK) == (0, 1, 2)
    for name in ("RaylibAMD_OverlapBoxes", "RaylibAMD_OverlapBoxesDevice", "RaylibAMD_OverlapBoxesHost", "RaylibAMD_PlanOverlapBoxes"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_oracle_is_the_restatement_byte_for_byte(lib, S, restated, name):
    tris, q, acc, n = restated[name]
    assert len(tris) == 10000 or name == "cornell"
    assert _host(lib, S[name], q, bc.ANY).tobytes() == bc.restate(q, tris, bc.ANY, acc=acc).tobytes()
    for k in MAX_HITS:
        rows, counts = _host(lib, S[name], q, bc.LIST, k)
        want_rows, want_counts = bc.restate(q, tris, bc.LIST, k, acc=acc)
        bad = np.nonzero((rows != want_rows).any(1) | (counts != want_counts))[0]
        assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), (k, bad[:8], counts[bad[:8]], want_counts[bad[:8]])
        assert _host(lib, S[name], q, bc.LIST, k, count=False).tobytes() == want_rows.tobytes(), "the rows do not depend on outCount"
    mask = _host(lib, S[name], q, bc.MARK)
    assert mask.dtype == np.uint32 and len(mask) == (len(tris) + 31) // 32
    assert mask.tobytes() == bc.restate(q, tris, bc.MARK, acc=acc).tobytes()
    # MARK is the OR of the complete accepted sets; ANY == (count > 0)
    assert np.array_equal(np.unpackbits(mask.view(np.uint8), bitorder="little")[:len(tris)].astype(bool), acc.any(0))
    assert not np.unpackbits(mask.view(np.uint8), bitorder="little")[len(tris):].any(), "bits at and above numTriangles are 0"
    assert np.array_equal(_host(lib, S[name], q, bc.ANY), (want_counts > 0).astype(np.uint32))
    # the set cuts, also in front of the boxes that hold the whole scene
    core = bc.core_count(n)
    share = (want_counts[:core] > 0).mean()
    assert 0.2 < share < 0.95 and (want_counts[:core] > 16).any(), share
    part = _host(lib, S[name], np.ascontiguousarray(q[:bc.LEAD]), bc.MARK)   # (Cornell's 36 large triangles are all met by the whole set)
    assert part.any() and np.unpackbits(part.view(np.uint8)).sum() < len(tris), "a mask that is neither empty nor full"
    assert (want_counts[core:n] == len(tris)).all(), "the enclosing boxes hold every triangle"


def test_list_shape(lib, S, restated):
    tris, q, acc, _ = restated["cornell"]
    for k in MAX_HITS:
        rows, counts = _host(lib, S["cornell"], q, bc.LIST, k)
        assert rows.shape == (len(q), k) and (counts > k).any() and (counts == 0).any()
        for row, c, a in zip(rows, counts, acc):
            listed = int((row >= 0).sum())
            assert (row[listed:] == -1).all() and (np.diff(row[:listed]) > 0).all() and listed == min(k, c)
            assert row[:listed].tolist() == np.nonzero(a)[0][:k].tolist()


def test_special_values(lib, S):
    for name in ("soup", "cornell"):
        tris, _ = S[name].export_flat()
        q, what = bc.specials(tris)
        acc = bc.accepted_sets(q, tris)
        rows, counts = _host(lib, S[name], q, bc.LIST)
        want_rows, want_counts = bc.restate(q, tris, bc.LIST, acc=acc)
        assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), [(w, g, x) for w, g, x in zip(what, counts, want_counts) if g != x]
        hits = _host(lib, S[name], q, bc.ANY)
        assert np.array_equal(hits, (counts > 0).astype(np.uint32))
        got = dict(zip(what, counts))
        # B1: none of these takes part; alone in a call each leaves the mask empty
        out = [w for w in what if "NaN" in w or "inf" in w] + ["a negative half extent"]
        assert len(out) == 10
        for w in out:
            i = what.index(w)
            assert got[w] == 0 and hits[i] == 0 and (rows[i] == -1).all(), w
            assert not _host(lib, S[name], q[i:i + 1], bc.MARK).any(), w
        assert got["a box 1e30 away"] == 0
        assert got["a half extent of 1e30"] == len(tris), "B2's box is infinite, every projection is inside or a NaN: nothing separates"
        assert got["a -0.0 half extent"] >= 1, "-0.0 is 0: a rectangle through the triangle's centroid"
        assert got["a triangle strictly inside the box"] >= 1 and got["non-orthonormal axes"] >= 0
        # zeroed axes: every frame coordinate is +0, so B4 separates nothing and B2 decides alone -- the triangles whose own box holds the centre
        c = q["center"][what.index("zeroed axes")]
        T = bc.tri_array(tris)
        assert got["zeroed axes"] == int(((T.min(1) <= c) & (c <= T.max(1))).all(1).sum()) >= 1
        if name == "cornell":   # (axis-aligned walls of large triangles: the touch and the interior case are decided robustly)
            assert got["a face exactly on a triangle's plane"] >= 1 and got["a box strictly inside a large triangle"] >= 1
            face = q[what.index("a face exactly on a triangle's plane")]
            moved = face.copy(); moved["axis"]["half"] = face["axis"]["half"] * np.float32(0.5)
            assert _host(lib, S[name], np.array([moved]), bc.LIST)[1][0] < got["a face exactly on a triangle's plane"], "half the box ends before the plane"
        i = what.index("a corner exactly on a vertex")
        assert got["a corner exactly on a vertex"] == int(acc[i].sum())


def test_refusals(lib, S):
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    prims = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)],
                                      [dict(minBounds=(1, 0, 0), maxBounds=(1.5, 0.5, 0.5), timeStartMove=0.0, velocity=(0.0, 0.0, 0.0), material=0)])
    raw = lib.Raylib_CreateScene()
    q = binding.box_queries(np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32))
    scene = S["cornell"].scene
    words = (lib.RaylibAMD_SceneNumTriangles(scene) + 31) // 32
    try:
        for entry in ("RaylibAMD_OverlapBoxesHost", "RaylibAMD_OverlapBoxes", "RaylibAMD_OverlapBoxesDevice"):
            f = getattr(lib, entry)
            tail = (None,) if entry.endswith("Device") else ()
            out, cnt = np.full(max(3 * 16, words), CANARY, np.uint32), np.full(3, CANARY, np.uint32)
            qp, op, cp = q.ctypes.data, out.ctypes.data, cnt.ctypes.data
            cases = [("spheres and cubes", (prims.scene, bc.LIST, qp, 3, 4, op, cp)), ("spheres and cubes, MARK", (prims.scene, bc.MARK, qp, 3, 4, op, None)),
                     ("unknown kind", (scene, 3, qp, 3, 4, op, None)), ("kind -1", (scene, -1, qp, 3, 4, op, None)),
                     ("n < 0", (scene, bc.LIST, qp, -1, 4, op, cp)), ("n < 0, MARK", (scene, bc.MARK, qp, -1, 4, op, None)),
                     ("maxHits 0", (scene, bc.LIST, qp, 3, 0, op, cp)), ("maxHits 17", (scene, bc.LIST, qp, 3, 17, op, cp)),
                     ("maxHits -1", (scene, bc.LIST, qp, 3, -1, op, None)), ("n * maxHits above 2^31 - 1", (scene, bc.LIST, qp, 0x7fffffff, 2, op, cp)),
                     ("ANY with outCount", (scene, bc.ANY, qp, 3, 4, op, cp)), ("MARK with outCount", (scene, bc.MARK, qp, 3, 4, op, cp)),
                     ("MARK with outCount, n == 0", (scene, bc.MARK, qp, 0, 4, op, cp)),
                     ("not finalized", (raw, bc.LIST, qp, 3, 4, op, cp)), ("not finalized, MARK", (raw, bc.MARK, qp, 3, 4, op, None)),
                     ("null q", (scene, bc.MARK, None, 3, 4, op, None)), ("null scene", (None, bc.MARK, qp, 3, 4, op, None))]
            for what, args in cases:
                assert f(*(args + tail)) == 0, (entry, what)
                assert (out == CANARY).all() and (cnt == CANARY).all(), (entry, what)
            assert f(*((scene, bc.LIST, qp, 3, 4, None, cp) + tail)) == 0 and (cnt == CANARY).all(), (entry, "null out")
            assert f(*((scene, bc.MARK, qp, 3, 4, None, None) + tail)) == 0, (entry, "null mask")
        # ANY and MARK do not read maxHits; n == 0 returns 1, and MARK's mask is then all zero
        out = np.full(max(3, words) + 1, CANARY, np.uint32)
        for k in (0, -5, 17, 1 << 30):
            assert lib.RaylibAMD_OverlapBoxesHost(scene, bc.ANY, q.ctypes.data, 3, k, out.ctypes.data, None) == 1
            assert lib.RaylibAMD_OverlapBoxesHost(scene, bc.MARK, q.ctypes.data, 3, k, out.ctypes.data, None) == 1
        assert out[-1] == CANARY or words < 3
        assert lib.RaylibAMD_OverlapBoxesHost(scene, bc.LIST, None, 0, 4, None, None) == 1, "n == 0 returns 1"
        assert lib.RaylibAMD_OverlapBoxesHost(scene, bc.MARK, None, 0, 0, None, None) == 1
        mask = np.full(words + 1, CANARY, np.uint32)
        assert lib.RaylibAMD_OverlapBoxesHost(scene, bc.MARK, None, 0, 0, mask.ctypes.data, None) == 1
        assert not mask[:words].any() and mask[words] == CANARY
        for kind in (bc.ANY, bc.LIST, bc.MARK):
            p = binding.QueryPlan()
            assert lib.RaylibAMD_PlanOverlapBoxes(prims.scene, kind, C.byref(p)) == 0 and lib.RaylibAMD_PlanOverlapBoxes(raw, kind, C.byref(p)) == 0
            assert lib.RaylibAMD_PlanOverlapBoxes(scene, kind, None) == 0 and lib.RaylibAMD_PlanOverlapBoxes(None, kind, C.byref(p)) == 0
        assert lib.RaylibAMD_PlanOverlapBoxes(scene, 3, C.byref(binding.QueryPlan())) == 0
    finally:
        lib.Raylib_DestroyScene(raw)
        prims.close()


@pytest.mark.parametrize("env", [None, "2", "4", "8"])
def test_plan_is_plan_overlaps(lib, S, monkeypatch, env):
    if env is not None:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", env)
    for name in ("cornell", "soup"):
        for kind, like in ((bc.ANY, 0), (bc.LIST, 1), (bc.MARK, 1)):
            rc, p = binding.plan_overlap_boxes(lib, S[name].scene, kind)
            rc2, p2 = binding.plan_overlap(lib, S[name].scene, like)
            assert rc == rc2 == 1 and p == p2, (name, kind, p, p2)
            assert p["early"] == int(kind == bc.ANY)


def test_float32_verdict_is_the_float64_verdict_away_from_the_boundary(lib, workdir):
    """4096 pairs of a rotated box and a triangle, each pair in a grid cell of its own (overlap_cases.generic_pairs' layout: one scene of the triangles, one call
    with the boxes), half extents 0.02 to 0.3: every pair whose float64 |margin| exceeds 2^-18 * (scene extent + |center|_max + half_max) has the float64
    verdict; the pairs inside that band are at most 1 % of the pairs whose B2 boxes meet."""
    import overlap_cases as oc
    rng = np.random.RandomState(5)
    n = 4096
    _, T = oc.generic_pairs(rng, n)
    centre = T.mean(1, dtype=np.float64) + rng.normal(size=(n, 3)) * 0.25
    half = np.exp(rng.uniform(np.log(0.02), np.log(0.3), (n, 3)))
    q = binding.box_queries(centre.astype(np.float32), half.astype(np.float32), bc.rotations(rng, n))
    ses = bc.session(lib, oc.write_triangles(os.path.join(str(workdir), "box_pairs.obj"), T))
    try:
        tris, _ = ses.export_flat()
        assert np.array_equal(bc.tri_array(tris), T), "the export order is the file's"
        rows, counts = _host(lib, ses, q, bc.LIST)
        extent = float(np.ptp(T.reshape(-1, 3).astype(np.float64), axis=0).max())
    finally:
        ses.close()
    k = np.arange(n)
    got = (rows == k[:, None]).any(1)
    assert (counts <= 16).all()
    margin = bc.margin64(q, T)
    band = 2.0 ** -18 * (extent + np.abs(q["center"].astype(np.float64)).max(1) + q["axis"]["half"].astype(np.float64).max(1))
    decisive = np.abs(margin) > band
    meet = bc.boxes_meet(q, T)[k, k]
    print("pairs %d, accepted %.3f, in the band %d, B2 boxes meet %d, disagreeing outside the band %d" % (
        n, got.mean(), int((~decisive).sum()), int(meet.sum()), int((got != (margin < 0))[decisive].sum())))
    assert 0.1 < got.mean() < 0.6, "the set must cut"
    bad = np.nonzero(decisive & (got != (margin < 0)))[0]
    assert len(bad) == 0, [(int(i), float(margin[i]), float(band[i]), bool(got[i])) for i in bad[:8]]
    assert (~decisive & meet).sum() <= 0.01 * meet.sum()
