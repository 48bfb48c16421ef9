"""What tests/test_overlap_host.py (no device) and tests/test_gpu_overlap.py share: statements O1 to O5 of include/raylib_amd.h (triangle-overlap queries)
restated in NumPy, an independent double-precision reference, the scenes and the query sets.

The restatement is elementwise float32 NumPy over every (query, triangle) pair: NumPy does not fuse operations, so each + - * rounds once, as the library's
-ffp-contract=off build does; least and greatest are np.where on the header's comparisons, in the header's order.  With dtype=float64 the same function gives
the gap the agreement test excuses pairs by.  The reference uses none of O4's axes: two triangles meet when an edge of one pierces the other (a
Moeller-Trumbore segment test with closed bounds, tried both ways), float64 throughout."""
import numpy as np

import helpers  # noqa: F401  (puts the package on sys.path)
import nearest_cases as nc
from raylib_amd import binding

ANY, LIST, SKIP_SHARED = 0, 1, 1
write_soup, session = nc.write_soup, nc.session


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _min3(a, b, c):
    m = np.where(b < a, b, a)
    return np.where(c < m, c, m)


def _max3(a, b, c):
    m = np.where(a < b, b, a)
    return np.where(m < c, c, m)


def axes_of(q0, q1, q2, v0, v1, v2):
    """O4's 17 axes in the header's order, from broadcastable (..., 3) vertices."""
    eQ = (q1 - q0, q2 - q1, q0 - q2)
    eT = (v1 - v0, v2 - v1, v0 - v2)
    nQ, nT = _cross(eQ[0], eQ[1]), _cross(eT[0], eT[1])
    return [nQ, nT] + [_cross(eQ[i], eT[j]) for i in range(3) for j in range(3)] + [_cross(nQ, e) for e in eQ] + [_cross(nT, e) for e in eT]


def pair_matrix(Q, T, skip_shared=False, dtype=np.float32, with_gap=False):
    """accepted[i, k]: O2 to O4 for query i (Q: (n, 3, 3)) and triangle k (T: (m, 3, 3)), every pair.  with_gap: also, per pair, the largest over the axes of
    (the distance by which the axis separates, negative when the projections overlap) / |axis|, over the axes of non-zero length."""
    Q, T = np.asarray(Q, dtype), np.asarray(T, dtype)
    with np.errstate(all="ignore"):
        q0, q1, q2 = (Q[:, None, k, :] for k in range(3))
        v0, v1, v2 = (T[None, :, k, :] for k in range(3))
        loQ, hiQ, loT, hiT = _min3(q0, q1, q2), _max3(q0, q1, q2), _min3(v0, v1, v2), _max3(v0, v1, v2)
        ok = ((loQ <= hiT) & (loT <= hiQ)).all(-1)
        if skip_shared:
            shared = np.zeros(ok.shape, bool)
            for a in (q0, q1, q2):
                for b in (v0, v1, v2):
                    shared |= (a == b).all(-1)
            ok &= ~shared
        d1, d2, t0, t1, t2 = q1 - q0, q2 - q0, v0 - q0, v1 - q0, v2 - q0
        zero = np.zeros((), dtype)
        gap = np.full(ok.shape, -np.inf)
        for a in axes_of(q0, q1, q2, v0, v1, v2):
            p1, p2 = _dot(a, d1), _dot(a, d2)
            s0, s1, s2 = _dot(a, t0), _dot(a, t1), _dot(a, t2)
            minQ, maxQ, minT, maxT = _min3(zero, p1, p2), _max3(zero, p1, p2), _min3(s0, s1, s2), _max3(s0, s1, s2)
            ok &= ~((maxQ < minT) | (maxT < minQ))
            if with_gap:
                length = np.sqrt(_dot(a, a).astype(np.float64))
                g = np.maximum(minT - maxQ, minQ - maxT) / length
                gap = np.where((length > 0) & (g > gap), g, gap)
    return (ok, gap) if with_gap else ok


def tri_array(tris):
    """(m, 3, 3) vertices of triangles as export_flat gives them."""
    return np.stack([tris["v0"], tris["v1"], tris["v2"]], 1).astype(np.float32)


def query_array(q):
    """(n, 3, 3) vertices of OVERLAP_QUERY_DTYPE records."""
    return np.stack([q["v0"], q["v1"], q["v2"]], 1)


def restate(queries, tris, kind, flags, max_hits=16, chunk=64):
    """O1 to O5 on OVERLAP_QUERY_DTYPE records: the ANY words, or (LIST rows, counts)."""
    Q, T = query_array(queries), tri_array(tris)
    n = len(Q)
    takes = np.isfinite(Q.reshape(n, 9)).all(1)
    rows, counts = np.full((n, max_hits), -1, np.int32), np.zeros(n, np.uint32)
    for a in range(0, n, chunk):
        acc = pair_matrix(Q[a:a + chunk], T, bool(flags & SKIP_SHARED)) & takes[a:a + chunk, None]
        counts[a:a + chunk] = acc.sum(1)
        for i, r in enumerate(acc):
            k = np.nonzero(r)[0][:max_hits]    # ascending
            rows[a + i, :len(k)] = k
    return (counts > 0).astype(np.uint32) if kind == ANY else (rows, counts)


# ---- the independent reference ----
def _pierces(a, b, v0, v1, v2):
    """Segment a-b against triangle v0 v1 v2, float64, (..., 3) each: Moeller-Trumbore with closed bounds; a segment parallel to the plane pierces nothing."""
    d, e1, e2 = b - a, v1 - v0, v2 - v0
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    with np.errstate(all="ignore"):
        s = a - v0
        u = (s * p).sum(-1) / det
        q = np.cross(s, e1)
        v = (d * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
        return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)


def pierce64(Q, T):
    """Per pair k: an edge of Q[k] pierces T[k] or an edge of T[k] pierces Q[k].  Q, T: (n, 3, 3)."""
    Q, T = np.asarray(Q, np.float64), np.asarray(T, np.float64)
    hit = np.zeros(len(Q), bool)
    for A, B in ((Q, T), (T, Q)):
        for i in range(3):
            hit |= _pierces(A[:, i], A[:, (i + 1) % 3], B[:, 0], B[:, 1], B[:, 2])
    return hit


def generic_pairs(rng, n, spacing=8.0):
    """n generic pairs (Q, T), (n, 3, 3) float32 each: vertices uniform in a unit-sized cube about the centre, the two centres a third of that apart in a random
    direction (about a sixth of such pairs meet); pair k sits in its own cell of a grid `spacing` apart, far from every other pair, so that one scene of the T and one call with the Q ask about
    each pair alone.  The cell offsets are multiples of `spacing` (a power of two): the float32 vertices are what every side of the comparison reads."""
    side = int(np.ceil(n ** (1 / 3)))
    cell = np.stack(np.unravel_index(np.arange(n), (side, side, side)), 1) * spacing
    direction = rng.normal(size=(n, 3)); direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    Q = cell[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 3))
    T = cell[:, None, :] + direction[:, None, :] * 0.33 + rng.uniform(-0.5, 0.5, (n, 3, 3))
    return Q.astype(np.float32), T.astype(np.float32)


def write_triangles(path, T):
    """An OBJ of the (m, 3, 3) triangles, three vertices of their own each, in this order."""
    lines = ["o tris\n"]
    for k, p in enumerate(np.asarray(T, np.float32)):
        for q in p:
            lines.append("v %.9g %.9g %.9g\n" % tuple(q))
        lines.append("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))
    with open(path, "w") as f:
        f.write("".join(lines))
    return path


# ---- query sets ----
def as_queries(Q):
    Q = np.asarray(Q, np.float32)
    return binding.overlap_queries(Q[:, 0], Q[:, 1], Q[:, 2])


def bounds(tris):
    T = tri_array(tris).reshape(-1, 3).astype(np.float64)
    return T.min(0), T.max(0)


def own_triangles(rng, tris, n, jitter=0.0):
    """n of the scene's own triangles; jitter: every vertex moved by up to that fraction of the triangle's size."""
    T = tri_array(tris)[rng.randint(0, len(tris), n)].astype(np.float64)
    if jitter:
        size = (T.max(1) - T.min(1)).max(1)
        T = T + rng.uniform(-1, 1, T.shape) * (jitter * size)[:, None, None]
    return T.astype(np.float32)


def random_triangles(rng, tris, n, lo=0.01, hi=2.0):
    """n random triangles about points of the scene's bounds, sized log-uniformly from lo to hi times the scene's extent."""
    mn, mx = bounds(tris)
    extent = float((mx - mn).max())
    size = extent * np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    centre = rng.uniform(mn, mx, (n, 3))
    return (centre[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 3)) * size[:, None, None]).astype(np.float32)


def specials(tris):
    """The special values of the contract on a scene's triangles: (records, what each is)."""
    T = tri_array(tris)
    mn, mx = bounds(tris)
    mid, ext = (mn + mx) / 2, float((mx - mn).max())
    t = T[len(T) // 2].copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rows = []
    for name, val in (("a NaN vertex", nan), ("an inf vertex", inf), ("a -inf vertex", -inf)):
        q = t.copy(); q[1, 2] = val
        rows.append((q, name))
    q = t.copy(); q[2] = (1e30, 0, 0)
    rows.append((q, "a 1e30 vertex"))
    q = t.copy(); q[0] = q[1] = q[2] = (1e30, -1e30, 1e30)
    rows.append((q, "a point 1e30 away"))
    rows.append((np.stack([t[0], t[0], t[0]]), "a point-sized query at a scene vertex"))
    rows.append((np.stack([t[0], t[1], t[1]]), "a segment-sized query along a scene edge"))
    # so large that, to its float arithmetic, the whole scene is one point -- the origin, which lies in its interior: v - q0 rounds to -q0 for every scene
    # vertex, no axis separates that point from the triangle around it, and the axes that overflow are NaN and separate nothing (O4)
    rows.append((np.array([(-1e30, -1e30, -1e30), (1e30, 1e30, -1e30), (0.0, 0.0, 2e30)]), "a query that contains the whole scene"))
    big = 4.0 * ext
    rows.append((np.array([mid + (-big, -big, -big), mid + (big, big, -big), mid + (0.0, 0.0, 2 * big)]), "a query whose box contains the scene"))
    rows.append((t + np.float32(1e6), "a query far outside"))
    rows.append((t, "a scene triangle itself"))
    return as_queries(np.stack([np.asarray(r, np.float32) for r, _ in rows])), [w for _, w in rows]


def query_set(rng, tris, n):
    """About n queries: a quarter the scene's own triangles, a quarter those jittered by up to 0.3 of their size, the rest random triangles from 0.01 to 2 times
    the scene's extent; then the specials."""
    q = n // 4
    sp, _ = specials(tris)
    Q = np.concatenate([own_triangles(rng, tris, q), own_triangles(rng, tris, q, jitter=0.3), random_triangles(rng, tris, n - 2 * q)])
    return np.concatenate([as_queries(Q), sp])
