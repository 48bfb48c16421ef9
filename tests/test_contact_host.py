"""Contact segments of the overlapping pairs (RaylibAMD_OverlapContacts, include/raylib_amd.h statements C1 to C6) without a device: the host oracle
RaylibAMD_OverlapContactsHost against a float32 NumPy restatement of the statements (tests/contact_cases.py), byte for byte, with LIST's rows and counts; every
endpoint bitwise the piercing point of the edge its feature names; exact cases on small-integer coordinates; every kind reached on the edge-touching set; the
accuracy against an independent double-precision reference; the refusals; the planner.  tests/test_gpu_contact.py holds the device to the oracle byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers  # noqa: F401
from helpers import scenes, ffi
import contact_cases as cc
import overlap_cases as oc
from raylib_amd import binding

CANARY = 0x5a5a5a5a


@pytest.fixture(scope="module")
def S(lib, workdir):
    d = os.path.join(str(workdir), "contact_host"); os.makedirs(d, exist_ok=True)
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


def _host(lib, ses, q, flags=0, max_hits=16, count=True):
    return binding.overlap_contacts(lib, ses.scene, q, flags, max_hits, host=True, count=count)


def _scene_of(lib, workdir, name, T):
    d = os.path.join(str(workdir), "contact_host"); os.makedirs(d, exist_ok=True)
    ses = oc.session(lib, oc.write_triangles(os.path.join(d, name + ".obj"), T))
    assert np.array_equal(oc.tri_array(ses.export_flat()[0]), np.asarray(T, np.float32)), "the export order is the file's"
    return ses


def _pairs_through_the_oracle(lib, workdir, name, Q, T, slice_=None):
    """Each pair (Q[k], T[k]) alone: (accepted (n,), records (n,)).  slice_ None: pair k sits in a cell of its own -- one scene of the T, one call with the Q, a
    query meets its own partner or nothing.  slice_ = 16: the pairs overlap one another (all about the origin), so 16 pairs at a time make a scene and a call
    with maxHits 16: no row is cut, and query i's partner, if accepted, is the entry that names it."""
    n = len(Q)
    if slice_ is None:
        ses = _scene_of(lib, workdir, name, T)
        try:
            rows, recs, counts = _host(lib, ses, oc.as_queries(Q), 0, 1)
        finally:
            ses.close()
        k = np.arange(n)
        assert ((rows[:, 0] == k) | (rows[:, 0] == -1)).all() and (counts <= 1).all(), "a query meets its own partner or nothing"
        return counts == 1, recs[:, 0]
    assert slice_ <= binding.MAX_OVERLAPS
    accepted, out = np.zeros(n, bool), np.zeros(n, cc.DTYPE)
    for a in range(0, n, slice_):
        ses = _scene_of(lib, workdir, name, T[a:a + slice_])
        try:
            rows, recs, counts = _host(lib, ses, oc.as_queries(Q[a:a + slice_]), 0, slice_)
        finally:
            ses.close()
        own = rows == np.arange(len(rows))[:, None]
        accepted[a:a + slice_] = own.any(1)
        i, e = np.nonzero(own)
        out[a + i] = recs[i, e]
    return accepted, out


def test_record_layout_and_exports(lib):
    assert cc.DTYPE.itemsize == 32
    assert [cc.DTYPE.fields[f][1] for f in ("p0", "kind", "p1", "features")] == [0, 12, 16, 28]
    assert (binding.CONTACT_NONE, binding.CONTACT_SEGMENT, binding.CONTACT_GAP, binding.CONTACT_NO_CROSSING) == (0, 1, 2, 3)
    for name in ("RaylibAMD_OverlapContacts", "RaylibAMD_OverlapContactsDevice", "RaylibAMD_OverlapContactsHost", "RaylibAMD_PlanOverlapContacts"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


@pytest.mark.parametrize("name,n", [("soup", 400), ("doubled", 200), ("cornell", 200), ("quad", 50)])
def test_oracle_is_the_restatement_byte_for_byte(lib, S, name, n):
    """The scenes of tests/test_overlap_host.py, both flag values, maxHits 1, 3 and 16: rows and counts are RaylibAMD_OverlapTrianglesHost LIST's, the records the
    restatement's; the reserved words are not read."""
    tris, _ = S[name].export_flat()
    q = oc.query_set(np.random.RandomState(17), tris, n)
    q["reserved0"], q["reserved1"], q["reserved2"] = 0xffffffff, 0x7fc00000, 12345
    kinds = set()
    for flags in (0, oc.SKIP_SHARED):
        for k in (1, 3, 16):
            rows, recs, counts = _host(lib, S[name], q, flags, k)
            list_rows, list_counts = binding.overlap_triangles(lib, S[name].scene, q, oc.LIST, flags, k, host=True)
            assert rows.tobytes() == list_rows.tobytes() and counts.tobytes() == list_counts.tobytes(), (name, flags, k)
            want_rows, want, want_counts = cc.restate(q, tris, flags, k)
            assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes()
            bad = np.argwhere(recs != want)
            assert recs.tobytes() == want.tobytes(), "%s, flags %d, maxHits %d: %d records differ, first %r got %r want %r" % (
                name, flags, k, len(bad), bad[0], recs[tuple(bad[0])], want[tuple(bad[0])])
            assert cc.rows_are_pairs(rows, recs)
            assert _host(lib, S[name], q, flags, k, count=False)[1].tobytes() == recs.tobytes(), "the records do not depend on outCount"
            kinds |= set(np.unique(recs["kind"]).tolist())
    if name != "quad":
        assert {cc.NONE, cc.SEGMENT, cc.NO_CROSSING} <= kinds, kinds


def test_endpoints_lie_on_their_edges(lib, S):
    """Tolerance-free: for every SEGMENT and GAP record each endpoint is bitwise the restated piercing point of the edge its feature names, whose weight is in
    [0, 1]; NONE and NO_CROSSING records have the bytes the statement gives."""
    seen = 0
    for name in ("soup", "cornell", "doubled"):
        tris, _ = S[name].export_flat()
        q = oc.query_set(np.random.RandomState(23), tris, 300)
        rows, recs, _ = _host(lib, S[name], q)
        Q, T = oc.query_array(q), oc.tri_array(tris)
        i, e = np.nonzero((recs["kind"] == cc.SEGMENT) | (recs["kind"] == cc.GAP))
        r = recs[i, e]
        for end, shift in (("p0", 0), ("p1", 8)):
            f = (r["features"] >> shift) & 0xff
            assert (f <= 5).all()
            p, w = cc.edge_point(Q[i], T[rows[i, e]], f)
            assert r[end].tobytes() == p.astype(np.float32).tobytes(), (name, end)
            assert ((w >= 0) & (w <= 1)).all(), (name, end, w.min(), w.max())
        assert (r["features"] >> 16 == 0).all()
        seen += len(r)
        rest = recs[(recs["kind"] == cc.NONE)]
        assert not rest.tobytes().strip(b"\0")
        nc = recs[recs["kind"] == cc.NO_CROSSING]
        want = np.zeros(len(nc), cc.DTYPE); want["kind"] = cc.NO_CROSSING
        assert nc.tobytes() == want.tobytes(), "NO_CROSSING: points +0, features 0"
        assert set(np.unique(recs["kind"]).tolist()) <= {0, 1, 2, 3}
    assert seen > 1000


def test_exact_cases(lib, workdir):
    T, Q = cc.exact_scene_and_queries()
    ses = _scene_of(lib, workdir, "exact", T)
    try:
        rows, recs, counts = _host(lib, ses, oc.as_queries(Q), 0, 2)
        assert recs.tobytes() == cc.restate(oc.as_queries(Q), ses.export_flat()[0], 0, 2)[1].tobytes()
    finally:
        ses.close()
    for k, (what, _, _, accepted, kind, ends, features) in enumerate(cc.EXACT):
        off = np.array((100.0 * k, 0, 0))
        assert counts[k] == int(accepted) and rows[k].tolist() == [k, -1], what
        r = recs[k, 0]
        assert r["kind"] == kind, (what, r)
        assert recs[k, 1].tobytes() == bytes(32), what
        if ends is None:
            assert r["p0"].tobytes() == bytes(12) and r["p1"].tobytes() == bytes(12) and r["features"] == 0, (what, r)
        else:
            got = {tuple((r["p0"] - off).tolist()), tuple((r["p1"] - off).tolist())}
            assert got == {tuple(float(x) for x in p) for p in ends}, (what, r)
            if len(ends) == 2:
                assert r["p0"].tolist() != r["p1"].tolist(), what
        if features is not None:
            assert {int(r["features"]) & 0xff, int(r["features"]) >> 8} == features, (what, r)


def test_every_kind_is_reached_on_the_edge_touching_set(lib, workdir):
    """2000 pairs whose Q has an edge through a point of T's edge, rounded to float32: whether the two intervals on the common line still meet is decided by the
    rounding.  At least 100 SEGMENT and 100 GAP records -- a condition on the inputs -- and the oracle is the restatement."""
    Q, T = cc.edge_touching_pairs(np.random.RandomState(11), 2000)
    accepted, recs = _pairs_through_the_oracle(lib, workdir, "touching", Q, T, slice_=16)
    assert np.array_equal(accepted, np.concatenate([oc.pair_matrix(Q[a:a + 50], T[a:a + 50]).diagonal() for a in range(0, len(Q), 50)]))
    want = cc.contact_of_pairs(Q[accepted], T[accepted])
    assert recs[accepted].tobytes() == want.tobytes()
    n_seg, n_gap = int((want["kind"] == cc.SEGMENT).sum()), int((want["kind"] == cc.GAP).sum())
    print("edge-touching pairs: %d accepted of %d, %d SEGMENT, %d GAP" % (accepted.sum(), len(Q), n_seg, n_gap))
    assert n_seg >= 100 and n_gap >= 100
    assert (recs[~accepted]["kind"] == cc.NONE).all()
    # a GAP still names the two facing ends, each on its edge
    g = accepted & (recs["kind"] == cc.GAP)
    for end, shift in (("p0", 0), ("p1", 8)):
        p, w = cc.edge_point(Q[g], T[g], (recs[g]["features"] >> shift) & 0xff)
        assert recs[g][end].tobytes() == p.astype(np.float32).tobytes() and ((w >= 0) & (w <= 1)).all()


@pytest.mark.parametrize("spacing", [8.0, 0.0])
@pytest.mark.parametrize("seed", cc.ACCURACY_SEEDS)
def test_accuracy_against_the_piercing_reference(lib, workdir, seed, spacing):
    """20000 generic pairs (oc.generic_pairs; at spacing 0 all about the origin, asked in slices of 16) against the float64 reference: no pair the reference
    says meets is left out, each has exactly two piercing points and kind SEGMENT, and the endpoints are within cc.ACCURACY_BOUND_ULPS of the reference's as an
    unordered pair.  At spacing 0, seed 1, O4 accepts exactly the pairs the reference says meet.
    Measured (the restatement, which the library equals bitwise): at most 0.531 ulp at spacing 8; 29.1, 329.2 and 38.9 ulp at spacing 0 (seeds 1, 2, 3)."""
    Q, T = oc.generic_pairs(np.random.RandomState(seed), cc.ACCURACY_PAIRS, spacing)
    meets = oc.pierce64(Q, T)
    count, pts = cc.pierce_points64(Q, T)
    assert (count[meets] == 2).all(), "general position: a meeting pair has exactly two piercing points"
    assert (count[~meets] == 0).all()
    accepted, recs = _pairs_through_the_oracle(lib, workdir, "generic_%d_%d" % (seed, int(spacing)), Q, T, slice_=None if spacing else 16)
    assert accepted[meets].all(), "no meeting pair is left out"
    if spacing == 0.0 and seed == 1:
        assert np.array_equal(accepted, meets), "O4 accepts exactly the pairs the reference says meet"
    r = recs[meets]
    assert (r["kind"] == cc.SEGMENT).all(), np.unique(r["kind"], return_counts=True)
    assert r.tobytes() == cc.contact_of_pairs(Q[meets], T[meets]).tobytes(), "the library meets the bound through being the restatement"
    err = cc.segment_error_ulps(r, Q[meets], T[meets], pts[meets])
    print("seed %d spacing %g: %d meeting pairs, error max %.3f ulp, 99.9th percentile %.3f" % (seed, spacing, meets.sum(), err.max(), np.percentile(err, 99.9)))
    assert err.max() <= cc.ACCURACY_BOUND_ULPS[spacing]


def test_refusals(lib, S):
    """Every refusal of LIST, the null outContact, the unknown kinds RaylibAMD_OverlapTriangles keeps refusing; nothing is written."""
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    prims = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)],
                                      [dict(minBounds=(1, 0, 0), maxBounds=(1.5, 0.5, 0.5), timeStartMove=0.0, velocity=(0.0, 0.0, 0.0), material=0)])
    raw = lib.Raylib_CreateScene()
    q = oc.as_queries(np.array([[(0, 0, 0), (1, 0, 0), (0, 1, 0)]] * 3, np.float32))
    scene = S["soup"].scene
    try:
        for entry in ("RaylibAMD_OverlapContactsHost", "RaylibAMD_OverlapContacts", "RaylibAMD_OverlapContactsDevice"):
            f = getattr(lib, entry)
            tail = (None,) if entry.endswith("Device") else ()
            out, rec, cnt = np.full(3 * 16, CANARY, np.uint32), np.full(3 * 16 * 8, CANARY, np.uint32), np.full(3, CANARY, np.uint32)
            qp, op, rp, cp = q.ctypes.data, out.ctypes.data, rec.ctypes.data, cnt.ctypes.data
            cases = [("spheres and cubes", (prims.scene, 0, qp, 3, 4, op, rp, cp)), ("n < 0", (scene, 0, qp, -1, 4, op, rp, cp)),
                     ("flag bit 1", (scene, 2, qp, 3, 4, op, rp, cp)), ("flag bit 31", (scene, 0x80000001, qp, 3, 4, op, rp, None)),
                     ("maxHits 0", (scene, 0, qp, 3, 0, op, rp, cp)), ("maxHits 17", (scene, 0, qp, 3, 17, op, rp, cp)),
                     ("maxHits -1", (scene, 1, qp, 3, -1, op, rp, None)), ("n * maxHits above 2^31 - 1", (scene, 0, qp, 0x7fffffff, 2, op, rp, cp)),
                     ("not finalized", (raw, 0, qp, 3, 4, op, rp, cp)), ("null q", (scene, 0, None, 3, 4, op, rp, cp)),
                     ("null outIndex", (scene, 0, qp, 3, 4, None, rp, cp)), ("null outContact", (scene, 0, qp, 3, 4, op, None, cp)),
                     ("null scene", (None, 0, qp, 3, 4, op, rp, cp))]
            for what, args in cases:
                assert f(*(args + tail)) == 0, (entry, what)
                assert (out == CANARY).all() and (rec == CANARY).all() and (cnt == CANARY).all(), (entry, what)
        assert lib.RaylibAMD_OverlapContactsHost(scene, 0, None, 0, 4, None, None, None) == 1, "n == 0 returns 1"
        # RaylibAMD_OverlapTriangles has no third kind
        out = np.full(3 * 16, CANARY, np.uint32)
        for kind in (2, 3):
            assert lib.RaylibAMD_OverlapTrianglesHost(scene, kind, 0, q.ctypes.data, 3, 4, out.ctypes.data, None) == 0 and (out == CANARY).all()
        p = binding.QueryPlan()
        assert lib.RaylibAMD_PlanOverlapContacts(prims.scene, C.byref(p)) == 0 and lib.RaylibAMD_PlanOverlapContacts(raw, C.byref(p)) == 0
        assert lib.RaylibAMD_PlanOverlapContacts(scene, None) == 0 and lib.RaylibAMD_PlanOverlapContacts(None, C.byref(p)) == 0
    finally:
        lib.Raylib_DestroyScene(raw)
        prims.close()


@pytest.mark.parametrize("env", [None, "2", "4", "8"])
def test_plan_overlap_contacts_is_plan_overlap_for_list(lib, S, monkeypatch, env):
    if env is not None:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", env)
    for name in ("cornell", "quad", "soup"):
        rc, p = binding.plan_overlap_contacts(lib, S[name].scene)
        assert (rc, p) == binding.plan_overlap(lib, S[name].scene, oc.LIST), (name, env)
        assert rc == 1 and p["early"] == 0 and p["prims"] == 0
