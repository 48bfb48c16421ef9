"""What tests/test_box_host.py (no device) and tests/test_gpu_boxes.py share: statements B1 to B5 of include/raylib_amd.h (oriented-box range queries)
restated in NumPy, a double-precision 13-axis reference with its margin, the scenes and the query sets.

The restatement is elementwise float32 NumPy over every (query, triangle) pair: NumPy does not fuse operations, so each + - * rounds once, as the library's
-ffp-contract=off build does; least and greatest are np.where on the header's comparisons, in the header's order (overlap_cases._min3 / _max3)."""
import numpy as np

import helpers  # noqa: F401  (puts the package on sys.path)
import overlap_cases as oc
from raylib_amd import binding

ANY, LIST, MARK = 0, 1, 2
write_soup, session, tri_array, bounds = oc.write_soup, oc.session, oc.tri_array, oc.bounds
_dot, _cross, _min3, _max3 = oc._dot, oc._cross, oc._min3, oc._max3
EDGE_UW = ((1, 2), (2, 0), (0, 1))


def fields(q):
    """(center (n, 3), axes (n, 3, 3), half (n, 3)) of BOX_QUERY_DTYPE records."""
    return q["center"], q["axis"]["dir"], q["axis"]["half"]


def takes_part(q):
    """B1."""
    c, A, h = fields(q)
    n = len(q)
    with np.errstate(all="ignore"):
        return np.isfinite(c).all(1) & np.isfinite(A.reshape(n, 9)).all(1) & np.isfinite(h).all(1) & (h >= 0).all(1)


def enclosing(q, dtype=np.float32):
    """B2: (loQ, hiQ), (n, 3) each."""
    c, A, h = (np.asarray(x, dtype) for x in fields(q))
    with np.errstate(all="ignore"):
        e = (np.abs(A[:, 0, :]) * h[:, 0, None] + np.abs(A[:, 1, :]) * h[:, 1, None]) + np.abs(A[:, 2, :]) * h[:, 2, None]
        return c - e, c + e


def boxes_meet(q, T):
    """meets[i, k]: B2's box of query i against the own box of triangle k (T: (m, 3, 3)), float32."""
    T = np.asarray(T, np.float32)
    lo, hi = enclosing(q)
    v0, v1, v2 = (T[None, :, k, :] for k in range(3))
    loT, hiT = _min3(v0, v1, v2), _max3(v0, v1, v2)
    with np.errstate(all="ignore"):
        return ((lo[:, None, :] <= hiT) & (loT <= hi[:, None, :])).all(-1)


def pair_matrix(q, T):
    """accepted[i, k]: B2 to B4 for query i and triangle k (T: (m, 3, 3)), every pair, float32, operation for operation."""
    T = np.asarray(T, np.float32)
    c, A, h = (np.asarray(x, np.float32) for x in fields(q))
    ok = boxes_meet(q, T)
    with np.errstate(all="ignore"):
        p = []
        for k in range(3):
            d = T[None, :, k, :] - c[:, None, :]                                            # B3
            p.append(np.stack([_dot(A[:, None, i, :], d) for i in range(3)], -1))
        p0, p1, p2 = p
        H = h[:, None, :]
        for i in range(3):                                                                   # B4, the faces
            ok &= ~((_min3(p0[..., i], p1[..., i], p2[..., i]) > H[..., i]) | (_max3(p0[..., i], p1[..., i], p2[..., i]) < -H[..., i]))
        e = (p1 - p0, p2 - p1, p0 - p2)
        n = _cross(e[0], e[1])                                                               # the plane
        r = (H[..., 0] * np.abs(n[..., 0]) + H[..., 1] * np.abs(n[..., 1])) + H[..., 2] * np.abs(n[..., 2])
        s = _dot(n, p0)
        ok &= ~((s > r) | (s < -r))
        for i in range(3):                                                                   # the nine edge axes, the box axis outer
            u, w = EDGE_UW[i]
            for j in range(3):
                eu, ew = e[j][..., u], e[j][..., w]
                s0, s1, s2 = (x[..., w] * eu - x[..., u] * ew for x in (p0, p1, p2))
                r = H[..., u] * np.abs(ew) + H[..., w] * np.abs(eu)
                ok &= ~((_min3(s0, s1, s2) > r) | (_max3(s0, s1, s2) < -r))
    return ok


def accepted_sets(q, tris, chunk=64):
    """The complete accepted sets of B1 to B4: a bool matrix (n, m)."""
    T = tri_array(tris)
    takes = takes_part(q)
    return np.concatenate([pair_matrix(q[a:a + chunk], T) & takes[a:a + chunk, None] for a in range(0, len(q), chunk)]) if len(q) else np.zeros((0, len(T)), bool)


def mask_of(acc):
    """B5's MARK words of a bool matrix (n, m): bit k % 32 of word k / 32."""
    m = acc.shape[1]
    bits = np.zeros((m + 31) // 32 * 32, bool)
    bits[:m] = acc.any(0)
    return (bits.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def restate(q, tris, kind, max_hits=16, acc=None):
    """B1 to B5 on BOX_QUERY_DTYPE records: the ANY words, (LIST rows, counts), or the MARK mask."""
    acc = accepted_sets(q, tris) if acc is None else acc
    counts = acc.sum(1).astype(np.uint32)
    if kind == ANY:
        return (counts > 0).astype(np.uint32)
    if kind == MARK:
        return mask_of(acc)
    rows = np.full((len(q), max_hits), -1, np.int32)
    for i, r in enumerate(acc):
        k = np.nonzero(r)[0][:max_hits]    # ascending
        rows[i, :len(k)] = k
    return rows, counts


# ---- the double-precision reference ----
def margin64(q, T):
    """Per pair k (q[k] against T[k], (n, 3, 3)): the 13-axis separating-axis test in float64 on the box's axes normalised.  The margin is the greatest over
    the axes of (the gap by which the axis separates) / |axis|: positive means separated, negative is the least penetration.  Axes of zero length are left out."""
    c, A, h = (np.asarray(x, np.float64) for x in fields(q))
    A = A / np.linalg.norm(A, axis=2, keepdims=True)
    T = np.asarray(T, np.float64)
    p = [np.einsum("nij,nj->ni", A, T[:, k, :] - c) for k in range(3)]
    e = (p[1] - p[0], p[2] - p[1], p[0] - p[2])
    unit = np.eye(3)
    axes = [np.broadcast_to(unit[i], c.shape) for i in range(3)] + [np.cross(e[0], e[1])] + [np.cross(np.broadcast_to(unit[i], c.shape), e[j]) for i in range(3) for j in range(3)]
    margin = np.full(len(c), -np.inf)
    for L in axes:
        length = np.linalg.norm(L, axis=1)
        s = np.stack([(L * x).sum(1) for x in p], 1)
        r = (np.abs(L) * h).sum(1)
        with np.errstate(all="ignore"):
            g = np.maximum(s.min(1) - r, -r - s.max(1)) / length
        margin = np.where((length > 0) & (g > margin), g, margin)
    return margin


# ---- query sets ----
def rotations(rng, n):
    """n random rotations (n, 3, 3) float32: row k is axis k."""
    R = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    R[:, :, 0] *= np.sign(np.linalg.det(R))[:, None]
    return R.astype(np.float32)


def _extent(tris):
    mn, mx = bounds(tris)
    return mn, mx, float((mx - mn).max())


def own_boxes(rng, tris, n, jitter=0.0):
    """Axis-aligned boxes about n of the scene's own triangles: tight (their own boxes), or with centre and half extents jittered by up to that fraction."""
    T = tri_array(tris)[rng.randint(0, len(tris), n)].astype(np.float64)
    lo, hi = T.min(1), T.max(1)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    if jitter:
        size = h.max(1)[:, None]
        c = c + rng.uniform(-1, 1, c.shape) * jitter * size
        h = np.maximum(h + rng.uniform(-1, 1, h.shape) * jitter * size, 0)
    return binding.box_queries(c.astype(np.float32), h.astype(np.float32))


def random_boxes(rng, tris, n, lo=0.005, hi=0.5, rotated=True, zero=0):
    """n boxes about points of the scene's bounds, half extents log-uniform from lo to hi times the scene's extent per axis; zero: that many of the three half
    extents (chosen per box) are 0 -- 1: a flat box, 2: a needle, 3: a point."""
    mn, mx, ext = _extent(tris)
    h = ext * np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 3)))
    for k in range(n):
        h[k, rng.permutation(3)[:zero]] = 0.0
    return binding.box_queries(rng.uniform(mn, mx, (n, 3)).astype(np.float32), h.astype(np.float32), rotations(rng, n) if rotated else None)


def enclosing_boxes(rng, tris, n):
    """n boxes, rotated, that hold the whole scene."""
    mn, mx, ext = _extent(tris)
    h = ext * rng.uniform(2.0, 4.0, (n, 3))
    return binding.box_queries(np.tile(((mn + mx) / 2).astype(np.float32), (n, 1)), h.astype(np.float32), rotations(rng, n))


def _exact_offset(v, h):
    """c near v + h such that c - v is exact in float32 (the touch of an identity-axes box is then exact): (c, c - v)."""
    for step in range(64):
        c = np.float32(np.float64(v) + h * (1 + step / 64.0))
        d = np.float64(c) - np.float64(v)
        if np.float64(np.float32(d)) == d:
            return c, np.float32(d)
    raise AssertionError("no exactly representable offset")


def specials(tris):
    """The special values of the contract on a scene's triangles: (records, what each is)."""
    T = tri_array(tris)
    mn, mx, ext = _extent(tris)
    mid = ((mn + mx) / 2).astype(np.float32)
    rng = np.random.RandomState(len(T))
    R = rotations(rng, 4)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    base = binding.box_queries(mid[None], np.full((1, 3), 0.25 * ext, np.float32), R[:1])
    rows, what = [], []

    def add(q, name):
        rows.append(q.copy()); what.append(name)
    for name, val in (("NaN", nan), ("+inf", inf), ("-inf", -inf)):
        q = base.copy(); q["center"][0, 1] = val; add(q, "a %s centre" % name)
        q = base.copy(); q["axis"]["dir"][0, 2, 0] = val; add(q, "a %s axis" % name)
        q = base.copy(); q["axis"]["half"][0, 1] = val; add(q, "a %s half extent" % name)
    q = base.copy(); q["axis"]["half"][0, 2] = -1e-3; add(q, "a negative half extent")
    t = T[len(T) // 2]
    q = binding.box_queries(t.mean(0, dtype=np.float64).astype(np.float32)[None], np.array([[1.0, -0.0, 1.0]], np.float32) * ext); add(q, "a -0.0 half extent")
    q = base.copy(); q["center"][0] = (1e30, -1e30, 1e30); add(q, "a box 1e30 away")
    q = base.copy(); q["axis"]["half"][0] = 1e30; add(q, "a half extent of 1e30")
    # identity axes: a face exactly on a triangle's plane (a triangle that lies in a coordinate plane when the scene has one, else the plane through its
    # greatest-x vertex), and a corner exactly on a vertex
    planar = [(k, a) for k, tr in enumerate(T) for a in range(3) if tr[0, a] == tr[1, a] == tr[2, a]]
    k, a = planar[0] if planar else (len(T) // 3, 0)
    tr = T[k]
    v = tr[np.argmax(tr[:, a])]
    c = tr.mean(0, dtype=np.float64).astype(np.float32); h = np.full(3, 2.0 * ext, np.float32)
    c[a], h[a] = _exact_offset(v[a], 0.125 * ext)
    add(binding.box_queries(c[None], h[None]), "a face exactly on a triangle's plane")
    v = T[len(T) // 5][1]
    ch = [_exact_offset(v[b], 0.0625 * ext) for b in range(3)]
    add(binding.box_queries(np.array([[x[0] for x in ch]], np.float32), np.array([[x[1] for x in ch]], np.float32)), "a corner exactly on a vertex")
    # the largest triangle: a small rotated box about its centroid (no vertex or edge of the triangle is inside it: the plane axis or the edge axes decide)
    E = T.astype(np.float64)
    area = np.linalg.norm(np.cross(E[:, 1] - E[:, 0], E[:, 2] - E[:, 0]), axis=1)
    big = E[np.argmax(area)]
    edge = min(np.linalg.norm(big[i] - big[(i + 1) % 3]) for i in range(3))
    add(binding.box_queries(big.mean(0).astype(np.float32)[None], np.full((1, 3), 0.01 * edge, np.float32), R[1:2]), "a box strictly inside a large triangle")
    size = float((t.max(0) - t.min(0)).max())
    add(binding.box_queries(t.mean(0, dtype=np.float64).astype(np.float32)[None], np.full((1, 3), 2.0 * size, np.float32), R[2:3]), "a triangle strictly inside the box")
    add(binding.box_queries(t[0][None], np.full((1, 3), 0.25 * ext, np.float32), np.zeros((1, 3, 3), np.float32)), "zeroed axes")
    shear = np.array([[[2.0, 0.5, 0.0], [0.0, 0.5, 0.25], [1.0, 0.0, 3.0]]], np.float32)
    add(binding.box_queries(mid[None], np.full((1, 3), 0.05 * ext, np.float32), shear), "non-orthonormal axes")
    return np.concatenate(rows), what


LEAD = 4    # query_set's first records, tight boxes about four triangles: their MARK mask is neither empty nor full on every scene of the tests


def core_count(n):
    """How many of query_set(rs, tris, n)'s leading records are neither enclosing boxes nor specials."""
    return n - max(2, n // 100)


def query_set(rs, tris, n):
    """About n boxes, then the specials.  A fifth axis-aligned boxes about the scene's own triangles, half of them tight and half jittered by up to 0.5 of their
    size; a fifth random axis-aligned boxes; two fifths random rotated boxes with half extents from 0.005 to 0.5 of the scene's extent; the rest flat boxes,
    needles and points under random rotations; the last max(2, n / 100) of the n enclose the whole scene (core_count(n): the records in front of them)."""
    core = core_count(n)
    a = core // 5
    z = (core - 4 * a) // 3
    parts = [own_boxes(rs, tris, a // 2), own_boxes(rs, tris, a - a // 2, jitter=0.5), random_boxes(rs, tris, a, rotated=False), random_boxes(rs, tris, 2 * a),
             random_boxes(rs, tris, z, hi=0.2, zero=1), random_boxes(rs, tris, z, hi=0.2, zero=2), random_boxes(rs, tris, core - 4 * a - 2 * z, zero=3),
             enclosing_boxes(rs, tris, n - core), specials(tris)[0]]
    return np.concatenate(parts)
