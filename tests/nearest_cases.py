"""What tests/test_nearest_host.py (no device) and tests/test_gpu_nearest.py share: statements N1 to N4 of include/raylib_amd.h (nearest-point queries) restated
in NumPy, the scenes and the point sets.

The restatement is elementwise float32 NumPy over every (point, triangle) pair: NumPy does not fuse operations, so each + - * / rounds once, as the library's
-ffp-contract=off build does.  With dtype=float64 and own_box=False the same function is the brute force the definition's accuracy is judged by."""
import os

import numpy as np

import helpers  # noqa: F401  (puts the package on sys.path)
from raylib_amd import binding

WITHIN, CLOSEST = 0, 1
INF = np.float32(np.inf)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pair_distances(P, V0, V1, V2, dtype=np.float32, own_box=True):
    """(D, b1, b2), each (points, triangles): N1 to N3 (own_box False: E of N1 alone)."""
    P, V0, V1, V2 = (np.asarray(a, dtype) for a in (P, V0, V1, V2))
    one, zero = dtype(1), dtype(0)
    with np.errstate(all="ignore"):
        p, v0, v1, v2 = P[:, None, :], V0[None], V1[None], V2[None]
        ab, ac, ap, bp, cp = v1 - v0, v2 - v0, p - v0, p - v1, p - v2
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        den = one / ((va + vb) + vc)
        b1, b2 = vb * den, vc * den                                    # the interior
        w = e / (e + g)
        c = (va <= 0) & (e >= 0) & (g >= 0); b1 = np.where(c, one - w, b1); b2 = np.where(c, w, b2)
        c = (vb <= 0) & (d2 >= 0) & (d6 <= 0); b1 = np.where(c, zero, b1); b2 = np.where(c, d2 / (d2 - d6), b2)
        c = (d6 >= 0) & (d5 <= d6); b1 = np.where(c, zero, b1); b2 = np.where(c, one, b2)
        c = (vc <= 0) & (d1 >= 0) & (d3 <= 0); b1 = np.where(c, d1 / (d1 - d3), b1); b2 = np.where(c, zero, b2)
        c = (d3 >= 0) & (d4 <= d3); b1 = np.where(c, one, b1); b2 = np.where(c, zero, b2)
        c = (d1 <= 0) & (d2 <= 0); b1 = np.where(c, zero, b1); b2 = np.where(c, zero, b2)   # the first condition that holds decides
        b1, b2 = b1.astype(dtype), b2.astype(dtype)
        q = (v0 + b1[..., None] * ab) + b2[..., None] * ac
        r = p - q
        E = _dot(r, r)
        if not own_box:
            return E, b1, b2
        lo = np.where(v1 < v0, v1, v0); lo = np.where(v2 < lo, v2, lo)
        hi = np.where(v0 < v1, v1, v0); hi = np.where(hi < v2, v2, hi)
        t, u = lo - p, p - hi
        d = np.where(t > 0, t, np.where(u > 0, u, zero)).astype(dtype)
        B = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        D = np.where(E >= B, E, B)
    return D.astype(dtype), b1, b2


def restate(points, tris, chunk=256):
    """N1 to N4 for (n, 4) float32 points on triangles as export_flat gives them: (CLOSEST records, WITHIN words, per point how many triangles attain the least D)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    out = np.zeros(len(pts), binding.NEAREST_DTYPE); out["prim"] = -1
    ties = np.zeros(len(pts), np.int64)
    for a in range(0, len(pts), chunk):
        P, md = pts[a:a + chunk, :3], pts[a:a + chunk, 3]
        D, b1, b2 = pair_distances(P, tris["v0"], tris["v1"], tris["v2"])
        with np.errstate(all="ignore"):
            takes = np.isfinite(P).all(1) & (md >= 0)
            R2 = md * md
            cand = (D <= R2[:, None]) & takes[:, None]
        least = np.where(cand, D, INF).min(1)
        at = cand & (D == least[:, None])
        k = at.argmax(1)                      # the first, i.e. lowest, index that attains it
        hit = cand.any(1)
        rows = np.arange(len(P))
        rec = out[a:a + chunk]
        rec["dist2"] = np.where(hit, D[rows, k], 0); rec["prim"] = np.where(hit, k, -1)
        rec["b1"] = np.where(hit, b1[rows, k], 0); rec["b2"] = np.where(hit, b2[rows, k], 0)
        ties[a:a + chunk] = np.where(hit, at.sum(1), 0)
    return out, (out["prim"] >= 0).astype(np.uint32), ties


def brute64(points, tris):
    """The least distance (not squared) from each point to the triangles, float64 throughout."""
    E, _, _ = pair_distances(np.asarray(points, np.float64)[:, :3], tris["v0"], tris["v1"], tris["v2"], dtype=np.float64, own_box=False)
    return np.sqrt(E.min(1))


# ---- scenes ----
def write_soup(path, n_tris, seed=3, extent=4.0, size=0.35, offset=0.0, doubled=False):
    """scenes.soup's triangles, moved by `offset` on every axis; doubled: each triangle twice, the 2 n faces in a shuffled order."""
    rng = np.random.RandomState(seed)
    tris = np.array([(rng.uniform(-extent, extent, 3) + rng.uniform(-size, size, (3, 3)) + offset) for _ in range(n_tris)]).astype(np.float32)
    if doubled:
        tris = np.concatenate([tris, tris])[rng.permutation(2 * n_tris)]
    lines = ["o soup\n"]
    for k, p in enumerate(tris):
        for q in p:
            lines.append("v %.9g %.9g %.9g\n" % tuple(q))
        lines.append("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))
    with open(path, "w") as f:
        f.write("".join(lines))
    return path


def session(lib, obj):
    return binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0)


# ---- points ----
def surface_points(rng, tris, n):
    """Points on n random triangles (barycentric, rounded to float32: on the surface up to rounding) and which triangle each lies on."""
    k = rng.randint(0, len(tris), n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    v0, v1, v2 = (tris[f][k].astype(np.float64) for f in ("v0", "v1", "v2"))
    return (v0 + a[:, None] * (v1 - v0) + b[:, None] * (v2 - v0)).astype(np.float32), k


def point_set(rng, tris, n, spread=1.5):
    """n points as (n, 4) rows: a quarter each random in `spread` x the bounds, on triangles, at vertices and on edges, a little (1e-4) off surfaces; maxDist +inf."""
    lo = np.minimum(np.minimum(tris["v0"].min(0), tris["v1"].min(0)), tris["v2"].min(0)).astype(np.float64)
    hi = np.maximum(np.maximum(tris["v0"].max(0), tris["v1"].max(0)), tris["v2"].max(0)).astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * spread
    q = n // 4
    rand = rng.uniform(mid - half, mid + half, (n - 3 * q, 3))
    on, _ = surface_points(rng, tris, q)
    k = rng.randint(0, len(tris), q)
    corner = np.stack([tris[("v0", "v1", "v2")[j % 3]][i] for j, i in enumerate(k)])
    edge = ((tris["v0"][k].astype(np.float64) + tris["v1"][k]) / 2)
    at = np.where((np.arange(q) % 2 == 0)[:, None], corner, edge)
    off, k2 = surface_points(rng, tris, q)
    nrm = np.cross(tris["v1"][k2].astype(np.float64) - tris["v0"][k2], tris["v2"][k2].astype(np.float64) - tris["v0"][k2])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    off = off + 1e-4 * nrm
    pts = np.concatenate([rand, on, at, off]).astype(np.float32)
    return np.concatenate([pts, np.full((len(pts), 1), np.inf, np.float32)], 1)


def special_points(tris):
    """The special values of the contract on a scene's triangles, (rows, what each row is): positions that are not finite, maxDist NaN / -1 / -0.0 / +inf / 3e38,
    a point 1e25 away."""
    v = tris["v0"][len(tris) // 2]
    away = v + np.float32(0.25)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rows = [((nan, 0, 0), inf, "NaN x"), ((0, nan, 0), 1.0, "NaN y"), ((0, 0, inf), inf, "+inf z"), ((-inf, 0, 0), inf, "-inf x"),
            (v, nan, "maxDist NaN"), (v, -1.0, "maxDist -1"), (v, -0.0, "maxDist -0.0 at a v0 vertex"), (away, -0.0, "maxDist -0.0 off the surface"),
            (v, 0.0, "maxDist 0 at a v0 vertex"), (away, inf, "maxDist +inf"), (away, 3e38, "maxDist 3e38"), ((1e25, 0, 0), inf, "1e25 away, maxDist +inf"),
            ((1e25, -1e25, 1e25), 3e38, "1e25 away, maxDist 3e38"), ((1e25, 0, 0), 1e10, "1e25 away, maxDist 1e10")]
    pts = np.array([list(p) + [m] for p, m, _ in rows], np.float32)
    return pts, [w for _, _, w in rows]


def with_max_dist(points, max_dist):
    out = np.array(points, np.float32)
    out[:, 3] = max_dist
    return out
