"""What tests/test_sweep_host.py (no device), tests/test_gpu_sweep.py and tests/sweep_rank_child.py share: statements W1 to W7 of include/raylib_amd.h
(swept-sphere queries, csrc/rl_sweep.h) restated in NumPy, the float64 geometry the statements are judged by, the scenes' sessions and the query sets.

The restatement is elementwise float32 NumPy over every (query, triangle) pair: NumPy does not fuse operations, so each + - * / and sqrt rounds once, as the
library's -ffp-contract=off build does.  W3 is tests/nearest_cases.py's restatement of N1 to N3.  The float64 check shares nothing with W4: it is point-triangle
and segment-triangle distance."""
import numpy as np

import helpers  # noqa: F401  (puts the package on sys.path)
import nearest_cases as nc
from raylib_amd import binding

ANY, CLOSEST = 0, 1
F = np.float32
INF = F(np.inf)
BIG = F(3.40282347e+38)

write_soup = nc.write_soup
session = nc.session


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def as_rows(queries):
    """(n, 8) float32 rows of queries given as rows or as SWEEP_QUERY_DTYPE records."""
    q = np.ascontiguousarray(queries)
    if q.dtype == binding.SWEEP_QUERY_DTYPE:
        q = q.view(F)
    return np.ascontiguousarray(q, F).reshape(-1, 8)


# ---- W1 to W7, float32 ----
def takes_part(q):
    """W1 for (n, 8) rows: (takes, o, d, inv, r) with d and inv as the statements read them."""
    o, r, delta = q[:, 0:3], q[:, 3], q[:, 4:7]
    with np.errstate(all="ignore"):
        ok = (r >= 0) & (r <= BIG) & ((o >= -BIG) & (o <= BIG) & (delta >= -BIG) & (delta <= BIG)).all(1)
        inv = F(1) / delta
        fin = (inv >= -BIG) & (inv <= BIG)
    return ok, o, np.where(fin, delta, F(0)).astype(F), np.where(fin, inv, F(0)).astype(F), r


def box_time(o, d, inv, r, lo, hi):
    """W2: o, d, inv (.., 3) and r (..) against boxes lo, hi (.., 3), broadcast."""
    shape = np.broadcast(o[..., 0], lo[..., 0]).shape
    entry, exit_, ok = np.zeros(shape, F), np.full(shape, INF, F), np.ones(shape, bool)
    for a in range(3):
        l, h = lo[..., a] - r, hi[..., a] + r
        tl, th = (l - o[..., a]) * inv[..., a], (h - o[..., a]) * inv[..., a]
        moving = np.broadcast_to(d[..., a] != 0, shape)
        near, far = np.where(d[..., a] > 0, tl, th), np.where(d[..., a] > 0, th, tl)
        entry = np.where(moving & (near > entry), near, entry)
        exit_ = np.where(moving & (far < exit_), far, exit_)
        ok = ok & (moving | ((l <= o[..., a]) & (o[..., a] <= h)))
    return np.where(ok & (entry <= exit_), entry, INF).astype(F)


def _root(m, v, r):
    """W4's root of |m + t v| = r: (accepted, t)."""
    a, b = _dot(v, v), _dot(m, v)
    f = b / a
    h = m - f[..., None] * v
    disc = a * (r * r - _dot(h, h))
    t = ((F(0) - b) - np.sqrt(disc)) / a
    return (a > 0) & (disc >= 0) & (t >= 0) & (t <= 1), t


def pair_times(q, V0, V1, V2):
    """(candidate, T, feature, point) of every (query, triangle) pair, shapes (n, m) and (n, m, 3): W1 to W5."""
    takes, o_, d_, inv_, r_ = takes_part(q)
    V0, V1, V2 = (np.asarray(a, F) for a in (V0, V1, V2))
    with np.errstate(all="ignore"):
        o, d, inv, r = o_[:, None, :], d_[:, None, :], inv_[:, None, :], r_[:, None]
        V = [V0[None], V1[None], V2[None]]
        ab, ac = V[1] - V[0], V[2] - V[0]
        shape = (len(q), len(V0))
        t = np.full(shape, INF, F); feature = np.full(shape, -1, np.int32); point = np.zeros(shape + (3,), F)
        # the face
        n = _cross(ab, ac)
        ln, s, nd = np.sqrt(_dot(n, n)), _dot(n, o - V[0]), _dot(n, d)
        rl, as_ = r * ln, np.abs(s)
        closing = np.where(s > 0, F(0) - nd, nd)
        tf = (as_ - rl) / closing
        c, off = o + tf[..., None] * d, (r[..., None] * n) / ln[..., None]
        P = np.where((s > 0)[..., None], c - off, c + off)
        ok = (as_ > rl) & (closing > 0) & (tf <= 1)
        for j in range(3):
            A, B = V[j], V[(j + 1) % 3]
            ok = ok & (_dot(_cross(B - A, P - A), n) >= 0)
        t = np.where(ok, tf, t); feature = np.where(ok, 0, feature); point = np.where(ok[..., None], P, point)
        # the edges
        for j in range(3):
            A, B = V[j], V[(j + 1) % 3]
            e, m = B - A, o - A
            ie = F(1) / _dot(e, e)
            fd, fm = _dot(d, e) * ie, _dot(m, e) * ie
            ok, te = _root(m - fm[..., None] * e, d - fd[..., None] * e, r)
            u = fm + te * fd
            ok = ok & (u >= 0) & (u <= 1) & (te < t)
            t = np.where(ok, te, t); feature = np.where(ok, 1 + j, feature); point = np.where(ok[..., None], A + u[..., None] * e, point)
        # the vertices
        for j in range(3):
            ok, tv = _root(o - V[j], np.broadcast_to(d, shape + (3,)), r)
            ok = ok & (tv < t)
            t = np.where(ok, tv, t); feature = np.where(ok, 4 + j, feature); point = np.where(ok[..., None], np.broadcast_to(V[j], shape + (3,)), point)
        # W3 comes first
        D, b1, b2 = nc.pair_distances(o_, V0, V1, V2)
        start = D <= r * r
        qn = (V[0] + b1[..., None] * ab) + b2[..., None] * ac
        t = np.where(start, F(0), t); feature = np.where(start, 7, feature); point = np.where(start[..., None], qn, point)
        # W5
        lo = np.where(V[1] < V[0], V[1], V[0]); lo = np.where(V[2] < lo, V[2], lo)
        hi = np.where(V[0] < V[1], V[1], V[0]); hi = np.where(hi < V[2], V[2], hi)
        Bt = box_time(o, d, inv, r, lo, hi)
        T = np.where(t >= Bt, t, Bt)
        cand = (feature >= 0) & (T <= 1) & takes[:, None]
    return cand, T.astype(F), feature.astype(np.int32), point.astype(F)


def restate(queries, tris, chunk=64):
    """W1 to W6 for the queries on triangles as export_flat gives them: (CLOSEST records, ANY words, per query how many triangles attain the least T)."""
    q = as_rows(queries)
    out = np.zeros(len(q), binding.SWEEP_HIT_DTYPE); out["prim"] = -1
    ties = np.zeros(len(q), np.int64)
    for a in range(0, len(q), chunk):
        cand, T, feature, point = pair_times(q[a:a + chunk], tris["v0"], tris["v1"], tris["v2"])
        least = np.where(cand, T, INF).min(1)
        at = cand & (T == least[:, None])
        k = at.argmax(1)                      # the first, i.e. lowest, index that attains it
        hit = cand.any(1)
        rows = np.arange(len(k))
        rec = out[a:a + chunk]
        rec["t"] = np.where(hit, T[rows, k], 0); rec["prim"] = np.where(hit, k, -1); rec["feature"] = np.where(hit, feature[rows, k], 0)
        rec["point"] = np.where(hit[:, None], point[rows, k], 0)
        ties[a:a + chunk] = np.where(hit, at.sum(1), 0)
    return out, (out["prim"] >= 0).astype(np.uint32), ties


def ties_near(queries, tris):
    """Per query how many triangles attain the least T, by the restatement on the triangles whose box meets the move's box grown by the radius and a little --
    every candidate is among them.  For judging an input (does it tie?), not a result."""
    q = as_rows(queries)
    lo = np.minimum(np.minimum(tris["v0"], tris["v1"]), tris["v2"]).astype(np.float64)
    hi = np.maximum(np.maximum(tris["v0"], tris["v1"]), tris["v2"]).astype(np.float64)
    out = np.zeros(len(q), np.int64)
    for i, row in enumerate(q.astype(np.float64)):
        a, b = np.minimum(row[0:3], row[0:3] + row[4:7]), np.maximum(row[0:3], row[0:3] + row[4:7])
        pad = row[3] + 1e-3 * (1 + np.abs(row[0:3]).max() + np.abs(row[4:7]).max())
        near = np.nonzero(((lo <= b + pad) & (hi >= a - pad)).all(1))[0]
        if len(near):
            out[i] = restate(q[i:i + 1], tris[near])[2][0]
    return out


# ---- float64 geometry that shares nothing with W4 ----
def _clamp01(x):
    return np.minimum(np.maximum(x, 0.0), 1.0)


def _seg_seg(p1, q1, p2, q2):
    """Least distance between segments [p1, q1] and [p2, q2], (.., 3) float64, broadcast (Ericson's clamped closest points)."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f = (d1 * d1).sum(-1), (d2 * d2).sum(-1), (d2 * r).sum(-1)
    b, c = (d1 * d2).sum(-1), (d1 * r).sum(-1)
    tiny = 1e-300
    den = a * e - b * b
    with np.errstate(all="ignore"):
        s = np.where(den > tiny, _clamp01((b * f - c * e) / np.where(den > tiny, den, 1.0)), 0.0)
        s = np.where(a > tiny, s, 0.0)
        t = np.where(e > tiny, (b * s + f) / np.where(e > tiny, e, 1.0), 0.0)
        s = np.where(t < 0, np.where(a > tiny, _clamp01(-c / np.where(a > tiny, a, 1.0)), 0.0), np.where(t > 1, np.where(a > tiny, _clamp01((b - c) / np.where(a > tiny, a, 1.0)), 0.0), s))
        t = _clamp01(t)
    w = (p1 + s[..., None] * d1) - (p2 + t[..., None] * d2)
    return np.sqrt((w * w).sum(-1))


def point_tri64(P, V0, V1, V2):
    """Least distance from points (n, 3) to triangles (m, 3 each): (n, m), float64."""
    return np.sqrt(nc.pair_distances(np.asarray(P, np.float64), V0, V1, V2, dtype=np.float64, own_box=False)[0])


def segment_tri64(p, q, V0, V1, V2):
    """Least distance from the segment [p, q] (3,) to each of m triangles, float64: the segment meets the triangle (0), or the least of the end points'
    distances to the triangle and the segment's distances to the three edges."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    V0, V1, V2 = (np.asarray(a, np.float64) for a in (V0, V1, V2))
    ends = point_tri64(np.stack([p, q]), V0, V1, V2).min(0)
    edges = np.minimum(np.minimum(_seg_seg(p, q, V0, V1), _seg_seg(p, q, V1, V2)), _seg_seg(p, q, V2, V0))
    # the crossing: the end points on opposite sides of the plane and the crossing point inside the three edge planes
    n = np.cross(V1 - V0, V2 - V0)
    sp, sq = ((p - V0) * n).sum(-1), ((q - V0) * n).sum(-1)
    with np.errstate(all="ignore"):
        u = sp / (sp - sq)
        x = p + u[..., None] * (q - p)
        inside = np.ones(len(V0), bool)
        for A, B in ((V0, V1), (V1, V2), (V2, V0)):
            inside &= (np.cross(B - A, x - A) * n).sum(-1) >= 0
        cross = (sp * sq <= 0) & (sp != sq) & inside
    return np.where(cross, 0.0, np.minimum(ends, edges))


def extent_of(tris):
    lo = np.minimum(np.minimum(tris["v0"].min(0), tris["v1"].min(0)), tris["v2"].min(0)).astype(np.float64)
    hi = np.maximum(np.maximum(tris["v0"].max(0), tris["v1"].max(0)), tris["v2"].max(0)).astype(np.float64)
    return lo, hi, float((hi - lo).max())


# ---- queries ----
def query_set(rng, tris, n, rmax=0.2):
    """n queries as (n, 8) float32 rows on a scene's exported triangles.  Radii run from 0 to rmax extents (a fifth of them 0 to a hundredth of that, one in 16
    exactly 0).  Origins lie on and near triangles, 0 to 3 radii off along the normal -- but for a tenth that start outside the scene's box and leave it.  The
    moves, in equal parts: along the normal towards the triangle; against it; grazing along an edge at about a radius from it; aimed at a vertex and aimed at
    an edge's midpoint, both from outside the triangle near its plane; random, of 0.01 to 2 extents; zero."""
    lo, hi, ext = extent_of(tris)
    k = rng.randint(0, len(tris), n)
    v = [tris[f][k].astype(np.float64) for f in ("v0", "v1", "v2")]
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    on = v[0] + a[:, None] * (v[1] - v[0]) + b[:, None] * (v[2] - v[0])          # a point of triangle k
    nrm = np.cross(v[1] - v[0], v[2] - v[0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    u = rng.uniform(0, 1, n)
    r = rmax * ext * np.where(rng.uniform(0, 1, n) < 0.2, 0.01 * u, u ** 3)
    r[rng.uniform(0, 1, n) < 1 / 16] = 0.0
    side = rng.choice([-1.0, 1.0], n)
    off = rng.uniform(0, 3, n)
    off[rng.uniform(0, 1, n) < 0.15] = 0.0                                       # on the triangle
    rr = np.maximum(r, 1e-3 * ext)                                               # (a radius of 0 still starts off the surface)
    org = on + (side * off * rr)[:, None] * nrm
    kind = np.arange(n) % 7
    j = rng.randint(0, 3, n)
    A, B = np.stack([v[x][i] for i, x in enumerate(j)]), np.stack([v[(x + 1) % 3][i] for i, x in enumerate(j)])
    e = B - A
    el = np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-30)
    rnd = rng.normal(size=(n, 3)); rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    reach = rng.uniform(0.5, 1.5, n)[:, None]
    delta = np.zeros((n, 3))
    m = kind == 0; delta[m] = (-side * (off + 1) * rr * rng.uniform(0.3, 2.0, n))[m, None] * nrm[m]
    m = kind == 1; delta[m] = (side * rr * rng.uniform(0.1, 4.0, n))[m, None] * nrm[m]
    m = kind == 2                                                                 # beside the edge, about a radius from it, moving along it
    across = np.cross(e / el, nrm)
    org[m] = (A - 0.5 * e + (rr * rng.uniform(0.8, 1.2, n))[:, None] * (across * np.cos(off)[:, None] + nrm * np.sin(off)[:, None]))[m]
    delta[m] = (2.0 * e * reach)[m]
    centre = (v[0] + v[1] + v[2]) / 3
    for which, X in ((3, A), (4, A + 0.5 * e)):                                   # from outside the triangle, near its plane, aimed at a vertex / an edge's midpoint
        m = kind == which
        outward = X - centre
        outward /= np.maximum(np.linalg.norm(outward, axis=1, keepdims=True), 1e-30)
        org[m] = (X + ((1 + off) * rr)[:, None] * outward + (rr * rng.uniform(-0.5, 0.5, n))[:, None] * nrm)[m]
        delta[m] = ((X - org) * reach)[m]
    m = kind == 5; delta[m] = (rnd * (ext * 10 ** rng.uniform(-2, np.log10(2), n))[:, None])[m]
    out = rng.uniform(0, 1, n) < 0.1                                             # from outside the box, leaving
    face = rng.randint(0, 3, n)
    away = np.zeros((n, 3)); away[np.arange(n), face] = side
    org[out] = ((lo + hi) / 2 + away * ((hi - lo) / 2 + r[:, None] + ext * rng.uniform(0.05, 0.5, n)[:, None]) + rnd * 0.2 * ext)[out]
    delta[out] = (away * ext * rng.uniform(0, 1, n)[:, None] + rnd * 0.02 * ext)[out]
    q = np.zeros((n, 8), F)
    q[:, 0:3] = org; q[:, 3] = r; q[:, 4:7] = delta
    return q


def special_queries(tris):
    """The special values of the contract on a scene's triangles: (rows, what each row is)."""
    lo, hi, ext = extent_of(tris)
    k = len(tris) // 2
    v0, v1, v2 = (tris[f][k].astype(F) for f in ("v0", "v1", "v2"))
    n = np.cross((v1 - v0).astype(np.float64), (v2 - v0).astype(np.float64)); n /= max(np.linalg.norm(n), 1e-30)
    c = ((v0.astype(np.float64) + v1 + v2) / 3)
    r = F(0.02 * ext)
    above = (c + 3 * float(r) * n).astype(F)
    down = (-4 * float(r) * n).astype(F)
    weak = int(np.abs(down).argmin())
    nan, inf = F(np.nan), F(np.inf)
    z = np.zeros(3, F)
    rows = [(above, r, down, "towards the triangle"),
            ((nan, 0, 0), r, down, "NaN origin"), (above, r, (0, nan, 0), "NaN delta"), (above, nan, down, "NaN radius"),
            ((inf, 0, 0), r, down, "+inf origin"), (above, r, (0, 0, -inf), "-inf delta"), (above, inf, down, "+inf radius"),
            (above, F(-1.0), down, "negative radius"), (v0, F(-0.0), z, "radius -0.0 on a vertex, zero move"), (v0, F(0.0), (F(-0.0), F(-0.0), F(-0.0)), "radius 0 on a vertex, move -0.0"),
            (above, r, np.where(np.arange(3) == weak, F(1e-42), down), "the move's least component 1e-42"), (above, r, np.where(np.arange(3) == weak, F(0), down), "the move's least component 0"),
            (above, r, (F(1e-42), F(-1e-42), F(1e-45)), "a denormal move"), (above, r, z, "a zero move"),
            ((1e30, 0, 0), r, down, "1e30 away"), ((1e30, 1e30, -1e30), F(1e29), (-1e30, -1e30, 1e30), "1e30 away, moving back"),
            (v0, r, down, "origin exactly on a vertex"), (v0, F(0.0), down, "origin exactly on a vertex, radius 0"),
            ((c + 0.5 * (v1 - v0)).astype(F) - (v1 - v0) * F(2), r, ((v1 - v0) * F(4)).astype(F), "a move in the triangle's plane"),
            ((c + 0.5 * (v1 - v0)).astype(F) - (v1 - v0) * F(2), F(0.0), ((v1 - v0) * F(4)).astype(F), "a move in the triangle's plane, radius 0"),
            (c.astype(F) + np.array([ext, 0, 0], F), r, (F(-2 * ext), 0, 0), "along -x"), (c.astype(F) - np.array([0, ext, 0], F), r, (0, F(2 * ext), 0), "along +y"),
            (c.astype(F) + np.array([0, 0, ext], F), F(0.0), (0, 0, F(-2 * ext)), "along -z, radius 0")]
    q = np.zeros((len(rows), 8), F)
    for i, (o, rad, d, _) in enumerate(rows):
        q[i, 0:3] = o; q[i, 3] = rad; q[i, 4:7] = d
    q[:, 7] = nan                                                                 # the reserved word is not read
    return q, [w for _, _, _, w in rows]


def ending_at_contact(lib, ses, tris):
    """Queries whose move ends exactly at first contact: axis-parallel moves towards the scene, cut to delta * T with the oracle's own T, kept where the
    float32 product reproduces T == 1."""
    lo, hi, ext = extent_of(tris)
    rng = np.random.RandomState(5)
    q = np.zeros((64, 8), F)
    q[:, 0:3] = rng.uniform(lo, hi, (64, 3)); q[:, 3] = 0.01 * ext
    axis = np.arange(64) % 3
    q[np.arange(64), axis] = (lo - 0.5 * ext)[axis]
    q[np.arange(64), 4 + axis] = 2.0 * ext
    first = binding.sweep_spheres(lib, ses.scene, q, CLOSEST, host=True)
    hit = first["prim"] >= 0
    cut = q[hit].copy()
    cut[:, 4:7] = cut[:, 4:7] * first["t"][hit][:, None]
    again = binding.sweep_spheres(lib, ses.scene, cut, CLOSEST, host=True)
    return cut[(again["prim"] >= 0) & (again["t"] == 1.0)]
