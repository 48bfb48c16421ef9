"""What tests/test_nearest_all_host.py (no device) and tests/test_gpu_nearest_all.py share: statements K1 to K3 of include/raylib_amd.h (the K nearest
triangles and the count in range) restated in NumPy on nearest_cases.pair_distances, the scenes, and point sets whose radii are taken from the host oracle's
own rows so that every relation between a point's count and maxHits occurs."""
import os

import numpy as np

import helpers  # noqa: F401  (puts the package on sys.path)
from helpers import scenes
import nearest_cases as nc
from raylib_amd import binding

INF = np.float32(np.inf)
MAX = binding.MAX_NEAREST


def restate(points, tris, max_hits, chunk=256):
    """K1 to K3 for (n, 4) float32 points on triangles as export_flat gives them: ((n, max_hits) records, uint32 counts).  The set is sorted by a stable sort
    on D over the triangles in export order, which is the order (D, k)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    rows = np.zeros((len(pts), max_hits), binding.NEAREST_DTYPE); rows["prim"] = -1
    counts = np.zeros(len(pts), np.uint32)
    for a in range(0, len(pts), chunk):
        P, md = pts[a:a + chunk, :3], pts[a:a + chunk, 3]
        D, b1, b2 = nc.pair_distances(P, tris["v0"], tris["v1"], tris["v2"])
        with np.errstate(all="ignore"):
            takes = np.isfinite(P).all(1) & (md >= 0)
            R2 = md * md
            member = (D <= R2[:, None]) & takes[:, None]
        cnt = member.sum(1)
        # members first, by (D, k): a stable sort on "not a member", then D, over ascending k
        order = np.lexsort((D, ~member), axis=1)[:, :max_hits]
        if order.shape[1] < max_hits:   # fewer triangles than records
            order = np.concatenate([order, np.zeros((len(P), max_hits - order.shape[1]), order.dtype)], 1)
        r = np.arange(len(P))[:, None]
        held = np.arange(max_hits)[None, :] < cnt[:, None]
        rec = rows[a:a + chunk]
        rec["dist2"] = np.where(held, D[r, order], 0); rec["prim"] = np.where(held, order, -1)
        rec["b1"] = np.where(held, b1[r, order], 0); rec["b2"] = np.where(held, b2[r, order], 0)
        counts[a:a + chunk] = cnt
    return rows, counts


# ---- scenes ----
SCENES = ("cornell", "soup", "doubled")
TWINS = {"cornell": 1, "soup": 1, "doubled": 2}   # how many times a scene holds each of its triangles: every count there is a multiple of it


def make_sessions(lib, d):
    """Cornell, the soup of 2000 triangles, and the soup of 500 with every triangle twice (exact-D ties between different export indices)."""
    os.makedirs(d, exist_ok=True)
    return {"cornell": nc.session(lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
            "soup": nc.session(lib, nc.write_soup(os.path.join(d, "soup.obj"), 2000)),
            "doubled": nc.session(lib, nc.write_soup(os.path.join(d, "doubled.obj"), 500, seed=5, doubled=True))}


def oracle(lib, ses, pts, max_hits, count=True):
    return binding.nearest_points_all(lib, ses.scene, pts, max_hits, count=count, host=True)


# ---- points ----
def base_points(ses, seed, n):
    """nearest_cases.point_set with maxDist +inf, and the host oracle's own rows for them at maxHits = 16: the distances the radii are taken from."""
    tris, _ = ses.export_flat()
    assert len(tris) > MAX, "the scene must hold more triangles than a row"
    pts = nc.point_set(np.random.RandomState(seed), tris, n)
    rows = oracle(ses.lib, ses, pts, MAX, count=False)
    assert (rows["prim"] >= 0).all()
    return pts, rows


def calibrated(base, max_hits):
    """`base` = base_points(...) with each point's radius one of ten, in turn: sqrt(D_j) * (1 - 1e-6) and sqrt(D_j) * (1 + 1e-6) for j among entries 0,
    maxHits - 1, maxHits and 15 of the point's own row (maxHits = 16: entry 15 again), radius 0, and +inf.  1e-6 is 17 units of float32 rounding on the radius,
    so the radius squared lies strictly on its side of D_j unless D_j is 0."""
    pts, rows = base
    K = int(max_hits)
    d = np.sqrt(rows["dist2"].astype(np.float64))
    js = (0, K - 1, min(K, MAX - 1), MAX - 1)
    choices = [d[:, j] * f for j in js for f in (1 - 1e-6, 1 + 1e-6)] + [np.zeros(len(pts)), np.full(len(pts), np.inf)]
    which = np.arange(len(pts)) % len(choices)
    md = np.select([which == k for k in range(len(choices))], choices)
    return nc.with_max_dist(pts, md.astype(np.float32))


def check_classes(counts, max_hits, twins=1):
    """The condition on a calibrated point set, asserted on the oracle's counts before any comparison: the points with count 0, with 0 < count < maxHits, with
    count == maxHits and with count > maxHits are each at least a tenth of the set.  A class that no count can fall in is left out, and only then: a scene
    that holds every triangle `twins` times has counts that are multiples of `twins`, so "0 < count < maxHits" needs a multiple of `twins` strictly between
    0 and maxHits (none for maxHits 1, or for maxHits 2 with twins 2) and "count == maxHits" needs maxHits to be one."""
    counts = np.asarray(counts).astype(np.int64)
    K, tenth = int(max_hits), len(counts) / 10.0
    assert (counts % twins == 0).all()
    classes = {"count 0": counts == 0, "count > maxHits": counts > K}
    if twins < K:
        classes["0 < count < maxHits"] = (counts > 0) & (counts < K)
    if K % twins == 0:
        classes["count == maxHits"] = counts == K
    for what, m in classes.items():
        assert m.sum() >= tenth, "%s: %d of %d points at maxHits %d" % (what, m.sum(), len(counts), K)


def same_rows(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint32).reshape(len(got), -1) != want.view(np.uint32).reshape(len(want), -1)).any(1))[0]
        raise AssertionError("%s: %d points differ, first %d: got %r want %r" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]]))
