"""What tests/test_ray_query_all_host.py, tests/test_gpu_ray_query_all.py and tests/ray_query_all_rank_child.py share: the scenes, the truth and the one check
of the ordered multi-hit queries (include/raylib_amd.h statements M1 to M5).

The truth is oracle/ alone: a ray is peeled through oracle.interval_hits, layer j being the brute force over [nextup(t_(j-1)), tMax].  Layer j gives t_j, how
many primitives lie at exactly t_j (count_j) and up to 8 of them; the ray's sequence is the concatenation of its tie groups, its crossing count the sum of
count_j once a layer comes back empty.  Peeling moves tMin, and the candidate rule's "own box ends before tMin" depends on tMin: a ray is EXCUSED when any
peel call after its first reports nearerRejected > 0 -- there the oracle itself cannot tell.  That is a condition on the rays, computed from the oracle before
any result under test is looked at, and capped per scene (EXCUSED_CAP)."""
import os

import numpy as np

import helpers
from helpers import bits, nextup, with_interval

MAX_HITS = (1, 2, 3, 4, 8, 16)
LAYERS = 20
ORACLE_THREADS = 16
# the share of a scene's rays that may be excused: none, but on the Cornell box's vertex and edge rays, where profiles/r09_ray_query_intervals.log bounds it by
# 304 of 3696 (8.2 %)
EXCUSED_CAP = {"soup": 0.0, "room": 0.0, "cutout8": 0.0, "stack": 0.0, "cornell": 0.10}
N_RAYS = {"soup": 300, "room": 300, "cutout8": 600, "cornell": 3800}


class Peel:
    """T (LAYERS, n): t_j, +inf from the layer at which the ray runs out; count (LAYERS, n); prims (LAYERS, n, 8); excused (n); done (n): the peel ran out
    within LAYERS layers, so total = count.sum(0) is the ray's crossing count."""

    def __init__(self, oracle, osc, rays, layers=LAYERS):
        n = len(rays)
        self.T = np.full((layers, n), np.inf, np.float32)
        self.count = np.zeros((layers, n), np.int64)
        self.prims = np.full((layers, n, 8), -1, np.int64)
        self.excused = np.zeros(n, bool)
        lo = np.array(rays[:, 3], np.float32)
        alive = np.ones(n, bool)
        for k in range(layers):
            idx = np.nonzero(alive)[0]
            if not len(idx):
                break
            got = oracle.interval_hits(osc, with_interval(rays[idx], lo[idx], None), 0.0, ORACLE_THREADS)
            hit = np.isfinite(got["t"])
            self.T[k, idx] = got["t"]
            self.count[k, idx] = np.where(hit, got["count"], 0)
            self.prims[k, idx] = got["prims"]
            if k > 0:
                self.excused[idx] |= got["nearerRejected"] > 0
            alive[idx] = hit
            lo[idx] = nextup(got["t"])
        self.done = ~alive
        self.total = self.count.sum(0)
        self.cum = np.cumsum(self.count, 0)


def assert_excused_cap(name, P):
    """before any result under test is looked at"""
    share = P.excused.mean() if len(P.excused) else 0.0
    print("%-8s rays %5d  excused %4d (%.1f %%)  peeled out %5d  layers up to %d  largest tie %d" % (
        name, len(P.excused), P.excused.sum(), 100 * share, P.done.sum(), np.isfinite(P.T).sum(0).max(), P.count.max()))
    assert share <= EXCUSED_CAP[name], "%s: %d of %d rays excused" % (name, P.excused.sum(), len(P.excused))


def check(label, rays, tris, P, max_hits, hits, counts, problems):
    """hits (n, max_hits) HITT records and counts (n uint32, or None) against the peel P of the same rays; differences go to `problems`."""
    n = len(rays)
    assert hits.shape == (n, max_hits), (hits.shape, n, max_hits)
    ok = ~P.excused

    def report(what, bad):
        bad = bad & ok
        if bad.any():
            i = int(np.argmax(bad))
            problems.append("%s / maxHits %d: %s on %d of %d rays; first ray %d %s: records %s, count %s, oracle t %s counts %s" % (
                label, max_hits, what, bad.sum(), n, i, [hex(b) for b in bits(rays[i])], hits[i].tolist(), None if counts is None else int(counts[i]),
                P.T[:, i][np.isfinite(P.T[:, i])].tolist(), P.count[:, i][:8].tolist()))

    got = hits["prim"] >= 0
    nhit = got.sum(1)
    # the hits come first, the miss records behind them, and a miss record is (0, -1, 0, 0)
    report("a hit behind a miss record", (got[:, 1:] & ~got[:, :-1]).any(1) if max_hits > 1 else np.zeros(n, bool))
    miss = ~got
    report("a miss record is not (0, -1, 0, 0)", (miss & ((bits(hits["t"]) != 0) | (hits["prim"] != -1) | (bits(hits["b1"]) != 0) | (bits(hits["b2"]) != 0))).any(1))
    known = np.minimum(P.total, max_hits)
    report("fewer records than the oracle's layers hold", nhit < known)
    report("more records than the ray has crossings", P.done & (nhit > known))
    o64, d64 = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    for k in range(max_hits):
        layer = (P.cum <= k).sum(0)                       # the tie group record k belongs to
        inside = layer < P.T.shape[0]
        lay = np.minimum(layer, P.T.shape[0] - 1)
        ar = np.arange(n)
        expect = inside & np.isfinite(P.T[lay, ar])
        both = expect & got[:, k]
        report("record %d: t differs in bits from layer's" % k, both & (bits(hits["t"][:, k]) != bits(P.T[lay, ar])))
        among = (hits["prim"][:, k][:, None] == P.prims[lay, ar]).any(1)
        report("record %d: prim is none of its layer's" % k, both & (P.count[lay, ar] <= 8) & ~among)
        idx = np.nonzero(got[:, k] & ok)[0]
        if len(idx):
            prim = hits["prim"][idx, k]
            inrange = prim < len(tris)
            bad = np.zeros(n, bool); bad[idx[~inrange]] = True
            report("record %d: prim beyond the scene's triangles" % k, bad)
            idx, prim = idx[inrange], prim[inrange]
            T = tris[prim]
            v0, v1, v2 = (T[c].astype(np.float64) for c in ("v0", "v1", "v2"))
            b1 = hits["b1"][idx, k].astype(np.float64)[:, None]; b2 = hits["b2"][idx, k].astype(np.float64)[:, None]
            p = v0 + b1 * (v1 - v0) + b2 * (v2 - v0)
            q = o64[idx] + hits["t"][idx, k].astype(np.float64)[:, None] * d64[idx]
            err = np.abs(p - q).max(1) / np.maximum(1.0, np.abs(q).max(1))
            bad = np.zeros(n, bool); bad[idx[~(err < 1e-5)]] = True
            report("record %d: b1, b2 do not rebuild o + t d within 1e-5" % k, bad)
    if counts is not None:
        report("outCount is not the oracle's crossing count", P.done & (counts.astype(np.int64) != P.total))
        report("outCount is below the peeled layers' sum", ~P.done & (counts.astype(np.int64) < P.total))
        report("outCount is below the number of records", counts.astype(np.int64) < nhit)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def case_rays(name, tris):
    """the rays of tests/test_gpu_ray_query_intervals.py, fewer of them"""
    import test_gpu_ray_query as base
    rng = np.random.RandomState(11)
    if name == "cornell":
        rays = base._vertex_edge_rays(tris)
        step = max(1, len(rays) // N_RAYS[name])
        return np.ascontiguousarray(rays[::step][:N_RAYS[name]])
    if name == "soup":
        return np.ascontiguousarray(base._random_rays(rng, 20000, -4.0, 4.0)[:N_RAYS[name]])
    if name == "room":
        return np.ascontiguousarray(base._random_rays(rng, 20000, (-0.9, 0.1, -0.9), (0.9, 1.9, 0.9))[:N_RAYS[name]])
    return np.ascontiguousarray(base._random_rays(rng, 8000, (-0.9, 0.1, -0.9), (0.9, 1.9, 3.0))[:N_RAYS[name]])


def write_stack(path):
    """Five parallel unit quads at z = 0 ... -4, each listed three times (30 triangles): rays along -z from z = 1 hit at t = 1, 2, 3, 4, 5 exactly, three
    triangles at each, six where the ray runs through the quads' diagonal."""
    lines, k = ["o stack\n"], 0
    for z in range(5):
        for _ in range(3):
            for q in ((0, 0), (1, 0), (1, 1), (0, 1)):
                lines.append("v %d %d %d\n" % (q[0], q[1], -z))
            lines.append("f %d %d %d\nf %d %d %d\n" % (k + 1, k + 2, k + 3, k + 1, k + 3, k + 4))
            k += 4
    with open(path, "w") as f:
        f.write("".join(lines))
    return path


def stack_rays():
    """49 rays off the diagonal, 7 on it (x == y: both triangles of a quad hold the point)"""
    g = (np.arange(7, dtype=np.float32) + 1) / 8
    xs, ys = np.meshgrid(g, g)
    o = np.stack([xs.ravel(), ys.ravel(), np.ones(49, np.float32)], 1).astype(np.float32)
    d = np.zeros((49, 3), np.float32); d[:, 2] = -1.0
    return helpers.rays8(o, d, 0.0, helpers.F32_MAX)


class Case:
    def __init__(self, name, ses, osc, tris, rays, P):
        self.name, self.ses, self.osc, self.tris, self.rays, self.P = name, ses, osc, tris, rays, P


def make_cases(lib, oracle, workdir, names):
    """name -> Case: the session, the oracle's scene of the same flat triangles, the rays and their peel (with the excused cap asserted).  The caller closes
    Case.ses and destroys Case.osc."""
    from raylib_amd import binding
    d = os.path.join(str(workdir), "ray_query_all_%d" % os.getpid()); os.makedirs(d, exist_ok=True)
    S = {}
    for name in names:
        sub = os.path.join(d, name); os.makedirs(sub, exist_ok=True)
        loader = None
        if name == "soup":
            obj = helpers.scenes.soup(os.path.join(sub, "soup.obj"))[0]
        elif name == "room":
            obj = helpers.scenes.cornell(os.path.join(sub, "room.obj"), tess=24, displace_fraction=0.2)[0]
        elif name == "cutout8":
            obj = helpers.scenes.cutout(os.path.join(sub, "cutout8.obj"), tess=4)[0]
            loader = helpers.texture_loader
        elif name == "cornell":
            obj = helpers.scenes.cornell(os.path.join(sub, "cornell.obj"))[0]
        else:
            obj = write_stack(os.path.join(sub, "stack.obj"))
        ses = binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
        flat = helpers.objflat.load_obj(obj, oracle, texture_loader=loader) if loader else helpers.objflat.load_obj(obj, oracle)
        tris, mats = ses.export_flat()   # the oracle's triangle k is the query's prim k
        assert tris.tobytes() == flat.triangles.tobytes() and mats.tobytes() == flat.materials.tobytes(), name
        osc = oracle.scene_create(flat, 1)
        rays = stack_rays() if name == "stack" else case_rays(name, tris)
        P = Peel(oracle, osc, rays)
        assert_excused_cap(name, P)
        S[name] = Case(name, ses, osc, tris, rays, P)
    return S


def tri_order(lib, ses):
    import ctypes as C
    n = lib.RaylibAMD_SceneNumTriangles(ses.scene)
    order = np.zeros(n, np.uint32)
    assert lib.RaylibAMD_SceneExportTriOrder(ses.scene, order.ctypes.data_as(C.POINTER(C.c_uint32))) == 1
    return order
