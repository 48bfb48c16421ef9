"""What tests/test_contact_host.py (no device) and tests/test_gpu_contact.py share: statements C1 to C6 of include/raylib_amd.h (the contact segment of an
overlapping triangle pair) restated in NumPy, an independent double-precision reference, the exact cases and the edge-touching set.

The restatement is elementwise float32 NumPy over matched pairs (Q[k], T[k]): NumPy does not fuse operations, so each + - * / rounds once, as the library's
-ffp-contract=off build does; every selection is np.where on the header's comparisons.  The reference uses none of C1 to C5: the segment's ends are the points
where an edge of one triangle pierces the other (tests/overlap_cases.py _pierces, a Moeller-Trumbore segment test in float64, extended to return the point)."""
import numpy as np

import helpers  # noqa: F401  (puts the package on sys.path)
import overlap_cases as oc
from raylib_amd import binding

NONE, SEGMENT, GAP, NO_CROSSING = 0, 1, 2, 3
DTYPE = binding.CONTACT_DTYPE


# ---- the restatement ----
def _crosses(ai, aj):
    return ((ai <= 0) & (0 < aj)) | ((aj <= 0) & (0 < ai))


def piercing_points(P, a):
    """C2 and C3 for one triangle per pair: P (n, 3, 3) vertices, a three (n,) plane values.  Returns (ok, pts) -- ok: exactly two edges cross; pts[i]: (n, 3), edge
    i's piercing point, computed for every edge whether it crosses or not (elementwise, so a crossing edge's point is the statement's) -- and the crossing flags."""
    c = [_crosses(a[i], a[(i + 1) % 3]) for i in range(3)]
    ok = (c[0].astype(int) + c[1].astype(int) + c[2].astype(int)) == 2
    pts = []
    for i in range(3):
        j = (i + 1) % 3
        w = a[i] / (a[i] - a[j])
        pts.append(P[:, i] + w[:, None] * (P[:, j] - P[:, i]))
    return ok, pts, c


def planes(Q, T):
    """C1: (a0, a1, a2), (b0, b1, b2), nQ, nT for matched pairs."""
    q0, q1, q2 = Q[:, 0], Q[:, 1], Q[:, 2]
    v0, v1, v2 = T[:, 0], T[:, 1], T[:, 2]
    nQ, nT = oc._cross(q1 - q0, q2 - q1), oc._cross(v1 - v0, v2 - v1)
    a = [oc._dot(nT, q - v0) for q in (q0, q1, q2)]
    b = [oc._dot(nQ, v - q0) for v in (v0, v1, v2)]
    return a, b, nQ, nT


def contact_of_pairs(Q, T, dtype=np.float32):
    """C1 to C6 for matched pairs that O1 to O4 accepted: CONTACT_DTYPE records (n,).  Q, T: (n, 3, 3)."""
    Q, T = np.asarray(Q, dtype), np.asarray(T, dtype)
    n = len(Q)
    out = np.zeros(n, DTYPE)
    with np.errstate(all="ignore"):
        a, b, nQ, nT = planes(Q, T)
        okQ, pQ, cQ = piercing_points(Q, a)
        okT, pT, cT = piercing_points(T, b)
        sel = lambda c, x, y: np.where(c[:, None] if x.ndim == 2 else c, x, y)
        # the lower crossing edge is 0 or 1, the higher 1 or 2
        PQ0, PQ1, fQ0, fQ1 = sel(cQ[0], pQ[0], pQ[1]), sel(cQ[2], pQ[2], pQ[1]), np.where(cQ[0], 0, 1), np.where(cQ[2], 2, 1)
        PT0, PT1, fT0, fT1 = sel(cT[0], pT[0], pT[1]), sel(cT[2], pT[2], pT[1]), np.where(cT[0], 3, 4), np.where(cT[2], 5, 4)
        d = np.abs(oc._cross(nQ, nT))
        m = np.where((d[:, 0] >= d[:, 1]) & (d[:, 0] >= d[:, 2]), 0, np.where(d[:, 1] >= d[:, 2], 1, 2))
        par = lambda P: np.take_along_axis(P, m[:, None], 1)[:, 0]
        swQ, swT = par(PQ1) < par(PQ0), par(PT1) < par(PT0)
        loQ, hiQ, fLoQ, fHiQ = sel(swQ, PQ1, PQ0), sel(swQ, PQ0, PQ1), np.where(swQ, fQ1, fQ0), np.where(swQ, fQ0, fQ1)
        loT, hiT, fLoT, fHiT = sel(swT, PT1, PT0), sel(swT, PT0, PT1), np.where(swT, fT1, fT0), np.where(swT, fT0, fT1)
        sT, eT = par(loT) > par(loQ), par(hiT) < par(hiQ)
        p0, p1 = sel(sT, loT, loQ), sel(eT, hiT, hiQ)
        kind = np.where(par(p0) <= par(p1), SEGMENT, GAP)
        feat = np.where(sT, fLoT, fLoQ) | (np.where(eT, fHiT, fHiQ) << 8)
    ok = okQ & okT
    out["p0"][ok], out["p1"][ok] = p0[ok], p1[ok]
    out["kind"] = np.where(ok, kind, NO_CROSSING)
    out["features"] = np.where(ok, feat, 0)
    return out


def edge_point(Q, T, feature):
    """The restated piercing point (float32) of the edge a feature names, per pair: 0..2 Q's edge, 3..5 T's edge; and its weight w."""
    Q, T = np.asarray(Q, np.float32), np.asarray(T, np.float32)
    with np.errstate(all="ignore"):
        a, b, _, _ = planes(Q, T)
        pts, ws = [], []
        for P, s in ((Q, a), (T, b)):
            for i in range(3):
                j = (i + 1) % 3
                w = s[i] / (s[i] - s[j])
                pts.append(P[:, i] + w[:, None] * (P[:, j] - P[:, i])); ws.append(w)
    pts, ws = np.stack(pts, 1), np.stack(ws, 1)    # (n, 6, 3), (n, 6)
    k = np.arange(len(Q))
    return pts[k, feature], ws[k, feature]


def restate(queries, tris, flags, max_hits=16):
    """RaylibAMD_OverlapContacts on OVERLAP_QUERY_DTYPE records: (rows, records, counts)."""
    rows, counts = oc.restate(queries, tris, oc.LIST, flags, max_hits)
    Q, T = oc.query_array(queries), oc.tri_array(tris)
    recs = np.zeros(rows.shape, DTYPE)
    i, e = np.nonzero(rows >= 0)
    recs[i, e] = contact_of_pairs(Q[i], T[rows[i, e]])
    return rows, recs, counts


def rows_are_pairs(rows, recs):
    """kind is NONE exactly behind the count, where all 32 bytes are zero."""
    none = recs["kind"] == NONE
    return np.array_equal(none, rows < 0) and not recs[none].tobytes().strip(b"\0")


# ---- the independent reference ----
def pierce_points64(Q, T):
    """Per pair: (count, points) -- how many of the six edges (Q's against T, then T's against Q) pierce the other triangle, float64, and those points, (n, 6, 3)
    with NaN where an edge does not pierce."""
    Q, T = np.asarray(Q, np.float64), np.asarray(T, np.float64)
    pts = np.full((len(Q), 6, 3), np.nan)
    hit = np.zeros((len(Q), 6), bool)
    for s, (A, B) in enumerate(((Q, T), (T, Q))):
        for i in range(3):
            a, b = A[:, i], A[:, (i + 1) % 3]
            h = oc._pierces(a, b, B[:, 0], B[:, 1], B[:, 2])
            # the point: where the segment meets B's plane
            n = np.cross(B[:, 1] - B[:, 0], B[:, 2] - B[:, 0])
            with np.errstate(all="ignore"):
                t = ((B[:, 0] - a) * n).sum(-1) / ((b - a) * n).sum(-1)
            pts[:, 3 * s + i] = np.where(h[:, None], a + t[:, None] * (b - a), np.nan)
            hit[:, 3 * s + i] = h
    return hit.sum(1), pts


def segment_error_ulps(recs, Q, T, pts):
    """For pairs with exactly two reference points: the larger component difference between the record's endpoints and the reference's, as an unordered pair, in
    ulps (float32) of the largest coordinate magnitude among the pair's six vertices."""
    order = np.argsort(np.isnan(pts[:, :, 0]), 1, kind="stable")[:, :2]
    k = np.arange(len(pts))
    r0, r1 = pts[k, order[:, 0]], pts[k, order[:, 1]]
    p0, p1 = recs["p0"].astype(np.float64), recs["p1"].astype(np.float64)
    straight = np.maximum(np.abs(p0 - r0).max(1), np.abs(p1 - r1).max(1))
    swapped = np.maximum(np.abs(p0 - r1).max(1), np.abs(p1 - r0).max(1))
    mag = np.maximum(np.abs(np.asarray(Q, np.float32)).reshape(len(Q), 9).max(1), np.abs(np.asarray(T, np.float32)).reshape(len(T), 9).max(1))
    return np.minimum(straight, swapped) / np.spacing(mag).astype(np.float64)


# The accuracy test's bound per spacing of oc.generic_pairs, in ulps: 8 times the largest error of the NumPy restatement against the float64 reference on the
# test's own inputs (np.random.RandomState seeds 1, 2, 3, 20000 pairs each; measured by tools/contact_accuracy.py into profiles/contact_accuracy.json), rounded
# up to a power of two.  At spacing 8 output rounding dominates: 0.531, 0.514, 0.505 ulp, so 8 x 0.531 = 4.2 -> 8.  At spacing 0 the tail is set by conditioning:
# 29.1, 329.2, 38.9 ulp with the 99.9th percentile between 10 and 19, so 8 x 329.2 = 2634 -> 4096.
ACCURACY_SEEDS, ACCURACY_PAIRS = (1, 2, 3), 20000
ACCURACY_BOUND_ULPS = {8.0: 8.0, 0.0: 4096.0}


# ---- exact cases: small-integer coordinates, every operation exact, the segment known by hand ----
A = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
EXACT = [
    # (what, Q, T, accepted, kind, the segment's two ends as a set (or None), the features' set)
    ("a plain crossing", A, [(1, 1, -2), (1, 1, 2), (3, 1, 2)], True, SEGMENT, {(1, 1, 0), (2, 1, 0)}, None),
    ("a crossing that ends at a vertex on the other plane", A, [(1, 1, 0), (1, 1, 4), (3, 1, -4)], True, SEGMENT, {(1, 1, 0), (2, 1, 0)}, None),
    ("coplanar overlapping", A, [(1, 1, 0), (6, 1, 0), (1, 6, 0)], True, NO_CROSSING, None, None),
    ("a vertex touching a face from the non-positive side", A, [(1, 1, 0), (1, 1, -3), (3, 1, -3)], True, NO_CROSSING, None, None),
    ("a vertex touching a face from the positive side", A, [(1, 1, 0), (1, 1, 3), (3, 1, 3)], True, SEGMENT, {(1, 1, 0)}, None),   # (a segment of one point)
    ("a zero-area T", A, [(1, 1, -1), (1, 1, 1), (1, 1, 1)], True, NO_CROSSING, None, None),
    ("a zero-area Q", [(1, 1, 0), (2, 2, 0), (2, 2, 0)], A, True, NO_CROSSING, None, None),
]


def exact_scene_and_queries():
    """One scene of the cases' T, 100 apart along x so that each query meets its own T alone; (T (m, 3, 3), Q (m, 3, 3))."""
    T = np.array([np.array(c[2], np.float32) + (100.0 * k, 0, 0) for k, c in enumerate(EXACT)], np.float32)
    Q = np.array([np.array(c[1], np.float32) + (100.0 * k, 0, 0) for k, c in enumerate(EXACT)], np.float32)
    return T, Q


# ---- the edge-touching set ----
def edge_touching_pairs(rng, n, spacing=0.0):
    """Pairs whose Q has an edge through a point of T's edge: T in float32; a point on T's edge v0-v1, a Q edge q0-q1 through it, Q's third vertex pushed away from
    T's third vertex, all in float64; then Q rounded to float32, once.  Whether Q's edge then passes T's edge on the inside (SEGMENT), misses it by less than
    O4 can tell (GAP) or by more (not accepted) is decided by the rounding.  spacing 0: every pair about the origin, where the rounding of the inputs is as fine as
    the arithmetic's, so GAP is common; the pairs then overlap one another and are asked in slices.  spacing > 0 (a power of two): pair k in its own cell, as
    oc.generic_pairs places its pairs; the inputs' rounding is coarser there and GAP rarer."""
    side = int(np.ceil(n ** (1 / 3)))
    cell = (np.stack(np.unravel_index(np.arange(n), (side, side, side)), 1) * spacing)[:, None, :]
    T = (cell + rng.uniform(-1, 1, (n, 3, 3))).astype(np.float32)
    T64 = T.astype(np.float64)
    u = rng.uniform(0.1, 0.9, n)
    p = T64[:, 0] + u[:, None] * (T64[:, 1] - T64[:, 0])
    direction = rng.normal(size=(n, 3)); direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    s, t = rng.uniform(0.2, 1.0, n), rng.uniform(0.2, 1.0, n)
    q0, q1 = p - s[:, None] * direction, p + t[:, None] * direction
    away = p - T64[:, 2]; away /= np.linalg.norm(away, axis=1, keepdims=True)
    q2 = p + away * rng.uniform(0.3, 1.0, n)[:, None] + 0.2 * rng.normal(size=(n, 3))
    return np.stack([q0, q1, q2], 1).astype(np.float32), T
