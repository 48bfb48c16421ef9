"""Batched ray queries over any [tMin, tMax] against an answer that owes nothing to the library: oracle_interval_hits (oracle/oracle.cc) tests every primitive
of the scene against each ray's own interval, with no tree and no box culling.  tests/test_gpu_ray_query.py holds the queries to RaylibAMD_ClosestHit, which
runs the same walk over one interval; here the interval starts behind the first surface, lies between two surfaces, is a point, is empty, has special values
for bounds or a negative tMin, on every tree the scene carries, for triangles with and without cut-outs, spheres and a moving cube.

One check for every ray set (_check): CLOSEST misses exactly where the oracle's t is +inf and otherwise has the oracle's t in bits, a primitive among those
the oracle found at that t, and barycentrics that rebuild o + t d on that exported triangle; SURFACE has the same hit, t and primitive; ANY is 1 exactly where
the oracle hits; and the CLOSEST records of the scene's trees are byte-equal wherever one primitive alone lies at the least t.  No ray is excused.

The surfaces behind the first one come from peeling the rays through the oracle alone (helpers.peel): t_1 < t_2 < t_3 < t_4 per ray."""
import os

import numpy as np
import pytest

import helpers
from helpers import ffi, scenes, bits, nextup, nextdown, with_interval
import test_gpu_ray_query as base

pytestmark = pytest.mark.gpu

FLT_MAX = helpers.F32_MAX
DENORM = helpers.F32_DENORM
INF, NAN = np.float32(np.inf), np.float32(np.nan)
ORACLE_THREADS = 16
LAYERS = 4
# rays per scene: the brute force costs rays x triangles, and the file stays below about 2e9 primitive tests (room 20736 triangles, soup 10000)
N_RAYS = {"soup": 2000, "room": 1200, "cornell": 3800, "cutout8": 4000}
N_SPECIAL = 600
SMALL_N = (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 513)
SUNS = ((1.0, 1.0, -0.0), (-1.0, 0.0, 1.0), (0.0, -1.0, -1.0), (1.0, 0.0, 0.0), (-0.0, -0.0, -1.0), (0.0, 1.0, -0.0))   # tests/test_host_logic.py's six


class Scene:
    def __init__(self, name, ses, osc, tris, trees, rays=None):
        self.name, self.ses, self.osc, self.tris, self.trees, self.rays = name, ses, osc, tris, sorted(trees), rays
        self.T = None


def _procedural():
    mats = np.zeros(2, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    for k in ("texAlbedo", "texNormal", "texRoughness", "texMetallic", "texEmissive"):
        mats[k] = -1
    sph = np.zeros(3, ffi.SPHERE_DTYPE)
    sph[0] = ((0.0, 0.0, 0.0), 0.5, 0); sph[1] = ((1.5, 0.0, -1.0), 0.3, 1); sph[2] = ((0.0, 0.3, -3.0), 1.5, 1)   # the third one behind the others
    cub = np.zeros(1, ffi.CUBE_DTYPE)
    cub[0] = ((-2.0, -0.25, -0.25), (-1.5, 0.25, 0.25), 0.0, (0.0, 1.0, 0.0), 1)
    return mats, sph, cub


@pytest.fixture(scope="module")
def iscenes(gpu_lib, oracle, workdir, sessions):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "ray_query_intervals"); os.makedirs(d, exist_ok=True)
    made, S = [], {}

    def add(name, ses, flat, trees):
        tris, mats = ses.export_flat()   # the oracle's triangle k is the query's prim k: export order is the flat order
        assert tris.tobytes() == flat.triangles.tobytes() and mats.tobytes() == flat.materials.tobytes(), name
        sc = Scene(name, ses, oracle.scene_create(flat, 1), tris, trees)
        sc.rays = np.ascontiguousarray(base._case_rays(name, ses))
        step = max(1, len(sc.rays) // N_RAYS[name]) if name == "cornell" else 1   # (the vertex and edge rays come grouped by origin: take them evenly)
        sc.rays = np.ascontiguousarray(sc.rays[::step][:N_RAYS[name]])
        sc.T = helpers.peel(oracle, sc.osc, sc.rays, LAYERS, 1e-4)
        S[name] = sc

    soup = binding.SceneSession(gpu_lib, scenes.soup(os.path.join(d, "soup.obj"))[0], (0, 0, 6), (0, 0, 0), 45.0, 1.0)
    made.append(soup)
    add("soup", soup, helpers.objflat.load_obj(os.path.join(d, "soup.obj"), oracle), {2, 4, 8})
    room = binding.SceneSession(gpu_lib, scenes.cornell(os.path.join(d, "room.obj"), tess=24, displace_fraction=0.2)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    made.append(room)
    add("room", room, helpers.objflat.load_obj(os.path.join(d, "room.obj"), oracle), {2, 4, 8})
    cut = os.path.join(d, "cutout8"); os.makedirs(cut, exist_ok=True)
    cutout8 = binding.SceneSession(gpu_lib, scenes.cutout(os.path.join(cut, "cutout8.obj"), tess=4)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    made.append(cutout8)
    flat = helpers.objflat.load_obj(os.path.join(cut, "cutout8.obj"), oracle, texture_loader=helpers.texture_loader)
    assert len(flat.triangles) == 608 and (flat.materials["texAlbedo"] >= 0).any() and len(flat.textures) > 0
    add("cutout8", cutout8, flat, {2, 4, 8})
    add("cornell", sessions["cornell"], helpers.flat_for_case("cornell", os.path.join(d, "cornell_flat"), oracle)[2], {2, 4})
    mats, sph, cub = _procedural()
    proc = binding.ProceduralSession(gpu_lib, mats, sph, cub)
    made.append(proc)
    flat = ffi.FlatScene(np.zeros(0, ffi.TRI_DTYPE), mats, spheres=sph, cubes=cub, num_shapes=0)
    p = Scene("procedural", proc, oracle.scene_create(flat, 1), np.zeros(0, ffi.TRI_DTYPE), {2})
    rng = np.random.RandomState(2)
    o = np.zeros((3000, 3), np.float32); o[:, 2] = 3.0
    tgt = rng.uniform((-2.2, -0.8, -1.2), (2.0, 1.5, 0.6), (3000, 3)).astype(np.float32)
    p.rays = helpers.rays8(o, (tgt - o).astype(np.float32))
    S["procedural"] = p
    yield S
    for sc in S.values():
        oracle.scene_destroy(sc.osc)
    for ses in made:
        ses.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _check(lib, oracle, monkeypatch, sc, label, rays, ray_time=0.0, oracle_rays=None, problems=None):
    """The one check (module docstring).  oracle_rays: the rays the oracle is asked, where the header defines the query's interval as another than the ray's
    (tMin < 0).  Differences go to `problems`, one line per kind of difference and tree with its first ray; returns the oracle's records."""
    from raylib_amd import binding
    rays = np.ascontiguousarray(rays, np.float32)
    want = oracle.interval_hits(sc.osc, rays if oracle_rays is None else oracle_rays, ray_time, ORACLE_THREADS)
    hit = np.isfinite(want["t"])
    print("%-10s %-34s rays %5d  hits %5d  ties %4d  nearerRejected %4d  trees %s" % (
        sc.name, label, len(rays), hit.sum(), (want["count"] > 1).sum(), int(want["nearerRejected"].sum()), sc.trees))
    if (want["count"] > 8).any():
        print("%-10s %-34s %d rays with more than 8 primitives at the least t (largest count %d): their prim is not checked" % (
            sc.name, label, (want["count"] > 8).sum(), want["count"].max()))
    if not len(rays):
        return want
    o64, d64 = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    records = {}

    def report(tree, what, bad, extra=None):
        if bad.any():
            i = int(np.argmax(bad))
            problems.append("%s / %s / tree %d: %s on %d of %d rays; first ray %d %s (bits %s) rayTime %g: oracle %s%s" % (
                sc.name, label, tree, what, bad.sum(), len(rays), i, rays[i].tolist(), [hex(b) for b in bits(rays[i])], ray_time, want[i],
                "" if extra is None else ", device %s" % (extra[i],)))

    for tree in sc.trees:
        base._force(lib, monkeypatch, sc.ses, str(tree))
        closest = binding.trace_rays(lib, sc.ses.scene, rays, binding.QUERY_CLOSEST, ray_time)
        surf, sprim = binding.trace_rays(lib, sc.ses.scene, rays, binding.QUERY_SURFACE, ray_time, with_prim=True)
        anyhit = binding.trace_rays(lib, sc.ses.scene, rays, binding.QUERY_ANY, ray_time)
        records[tree] = closest
        got = closest["prim"] >= 0
        report(tree, "CLOSEST hits where the oracle misses", got & ~hit, closest)
        report(tree, "CLOSEST misses where the oracle hits", ~got & hit, closest)
        both = got & hit
        report(tree, "CLOSEST t differs in bits", both & (bits(closest["t"]) != bits(want["t"])), closest)
        miss = ~got
        report(tree, "CLOSEST miss record is not (0, -1, 0, 0)", miss & ((bits(closest["t"]) != 0) | (closest["prim"] != -1) | (bits(closest["b1"]) != 0) | (bits(closest["b2"]) != 0)), closest)
        among = (closest["prim"][:, None] == want["prims"]).any(1)
        report(tree, "CLOSEST prim is none of the oracle's", both & (want["count"] <= 8) & ~among, closest)
        # the barycentrics rebuild o + t d on the exported triangle
        tri = both & (closest["prim"] < binding.PRIM_SPHERE)
        if tri.any():
            idx = np.nonzero(tri)[0]
            inrange = closest["prim"][idx] < len(sc.tris)
            report(tree, "CLOSEST prim beyond the scene's triangles", np.isin(np.arange(len(rays)), idx[~inrange]), closest)
            idx = idx[inrange]
            T = sc.tris[closest["prim"][idx]]
            v0, v1, v2 = (T[k].astype(np.float64) for k in ("v0", "v1", "v2"))
            b1 = closest["b1"][idx].astype(np.float64)[:, None]; b2 = closest["b2"][idx].astype(np.float64)[:, None]
            p = v0 + b1 * (v1 - v0) + b2 * (v2 - v0)
            q = o64[idx] + closest["t"][idx].astype(np.float64)[:, None] * d64[idx]
            err = np.abs(p - q).max(1) / np.maximum(1.0, np.abs(q).max(1))
            bad = np.zeros(len(rays), bool); bad[idx[~(err < 1e-5)]] = True
            report(tree, "b1, b2 do not rebuild o + t d within 1e-5 (worst %.3g)" % err.max(), bad, closest)
        other = both & ~tri
        report(tree, "a sphere's or cube's b1, b2 are not 0", other & ((closest["b1"] != 0) | (closest["b2"] != 0)), closest)
        report(tree, "SURFACE hit differs from the oracle's", (surf["hit"] == 1) != hit, surf)
        report(tree, "SURFACE t differs in bits", hit & (surf["hit"] == 1) & (bits(surf["t"]) != bits(want["t"])), surf)
        report(tree, "SURFACE outPrim is not CLOSEST's prim", sprim != closest["prim"], sprim)
        report(tree, "ANY is not 1 exactly where the oracle hits", anyhit != hit.astype(np.uint32), anyhit)
    single = want["count"] == 1
    first = records[sc.trees[0]].view(np.uint8).reshape(len(rays), -1)
    for tree in sc.trees[1:]:
        other = records[tree].view(np.uint8).reshape(len(rays), -1)
        report(tree, "CLOSEST record differs in bytes from tree %d's with one primitive at the least t" % sc.trees[0], single & (first != other).any(1), records[tree])
    return want


def _layer_sets(sc):
    """Sets 1 to 4 from the peeled layers"""
    T, out = sc.T, []
    for k in range(LAYERS - 1):
        a, b = T[k], T[k + 1]
        have = np.isfinite(a)
        two = have & np.isfinite(b)
        out.append(("1 behind surface %d" % (k + 1), with_interval(sc.rays[have], nextup(a[have]), FLT_MAX), "some"))
        out.append(("2 point interval at surface %d" % (k + 1), with_interval(sc.rays[have], a[have], a[have]), "all"))
        out.append(("3 between surfaces %d and %d" % (k + 1, k + 2), with_interval(sc.rays[two], nextup(a[two]), nextdown(b[two])), "none"))
        out.append(("4 from surface %d to %d" % (k + 1, k + 2), with_interval(sc.rays[two], a[two], b[two]), "all"))
    return out


TRIANGLE_SCENES = ["soup", "room", "cornell", "cutout8"]


@pytest.mark.parametrize("name", TRIANGLE_SCENES)
def test_surfaces_behind_the_first(gpu_lib, oracle, iscenes, monkeypatch, name):
    """Sets 1, 3, 4 and 5: the interval starts just behind surface k, lies strictly between two surfaces, runs from one to the next, is random."""
    sc, problems = iscenes[name], []
    assert np.isfinite(sc.T[0]).sum() > len(sc.rays) // 10
    for label, rays, expect in _layer_sets(sc):
        if label.startswith("2"):
            continue
        want = _check(gpu_lib, oracle, monkeypatch, sc, label, rays, problems=problems)
        hits = np.isfinite(want["t"])
        if expect == "all":        # from one surface to the next: one of the two at least is in range
            assert hits.all(), (name, label, (~hits).sum())
        elif expect == "none":     # nothing lies strictly between two consecutive surfaces
            assert not hits.any(), (name, label, hits.sum())
        elif label.endswith("surface 1"):   # coverage: behind the first surface at least 5 % of the scene's rays meet a second one
            assert hits.sum() >= 0.05 * len(sc.rays), (name, label, hits.sum(), len(sc.rays))
            assert (want["t"][hits] > sc.T[0][np.isfinite(sc.T[0])][hits]).all()
    rng = np.random.RandomState(17)
    a = rng.uniform(0.0, 8.0, len(sc.rays)).astype(np.float32); b = rng.uniform(0.0, 8.0, len(sc.rays)).astype(np.float32)
    _check(gpu_lib, oracle, monkeypatch, sc, "5 random [a, b]", with_interval(sc.rays, a, b), problems=problems)
    _check(gpu_lib, oracle, monkeypatch, sc, "5 random [b, a]", with_interval(sc.rays, b, a), problems=problems)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", TRIANGLE_SCENES)
def test_point_interval_at_a_surface_hits_it(gpu_lib, oracle, iscenes, monkeypatch, name):
    """Set 2: [t_k, t_k].  The device must give the oracle's answer, and every ray with a surface at t_k must hit it.  (With the render's candidate rule,
    whose own-box test rejects when the box's exit lies below tMin by as little as an ulp, the oracle and every tree of the device missed 117 of 956 first
    surfaces of the room, 318 of 3696 of the Cornell box and 236 of 2067 of the cut-out scene -- flat boxes of axis-aligned triangles; none of the soup.  The
    query unit widens that one comparison, csrc/rl_dev_walk.h OwnBoxPassBox, and oracle.cc CandidateRule follows it.)"""
    sc, problems, missed = iscenes[name], [], []
    for label, rays, expect in _layer_sets(sc):
        if not label.startswith("2"):
            continue
        want = _check(gpu_lib, oracle, monkeypatch, sc, label, rays, problems=problems)
        hits = np.isfinite(want["t"])
        print("%-10s %-34s %d of %d rays miss their own surface" % (name, label, (~hits).sum(), len(rays)))
        if not hits.all():
            i = int(np.argmax(~hits))
            missed.append("%s / %s: the oracle misses on %d of %d rays, first %s" % (name, label, (~hits).sum(), len(rays), [hex(b) for b in bits(rays[i])]))
    assert not problems, "\n".join(problems)
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("name", TRIANGLE_SCENES + ["procedural"])
def test_special_bounds(gpu_lib, oracle, iscenes, monkeypatch, name):
    """Set 6: zeros of either sign, the least denormal, infinities, FLT_MAX, NaN and a negative tMax as bounds of otherwise ordinary rays.  A NaN bound gives
    a miss (include/raylib_amd.h)."""
    sc, problems = iscenes[name], []
    rays = sc.rays[:N_SPECIAL]
    for tmin in (np.float32(0.0), np.float32(-0.0), DENORM, INF, NAN):
        want = _check(gpu_lib, oracle, monkeypatch, sc, "6 tMin %r" % float(tmin), with_interval(rays, tmin, FLT_MAX), problems=problems)
        if not np.isfinite(tmin):
            assert not np.isfinite(want["t"]).any()
        else:
            assert np.isfinite(want["t"]).sum() > len(rays) // 10
    for tmax in (np.float32(0.0), DENORM, FLT_MAX, INF, NAN, np.float32(-1.0)):
        want = _check(gpu_lib, oracle, monkeypatch, sc, "6 tMax %r" % float(tmax), with_interval(rays, 0.0, tmax), problems=problems)
        if tmax != tmax or tmax < 0:
            assert not np.isfinite(want["t"]).any()
    both = with_interval(rays, NAN, NAN)
    _check(gpu_lib, oracle, monkeypatch, sc, "6 tMin nan tMax nan", both, problems=problems)
    assert not problems, "\n".join(problems)


def test_second_generation_rays_in_the_planes_of_the_room(gpu_lib, oracle, iscenes, monkeypatch):
    """Set 7: origins on the room's surfaces (first-hit points), directions with exact +0 and -0 components, so that rays lie in the planes of the walls and of
    the boxes of every tree.  At these distances the header's exception for products beyond 1e30 does not apply: every tree gives the oracle's answer."""
    sc, problems = iscenes["room"], []
    have = np.isfinite(sc.T[0])
    o, d, t = sc.rays[have, 0:3], sc.rays[have, 4:7], sc.T[0][have]
    p = (o + t[:, None] * d).astype(np.float32)[:N_SPECIAL]     # Triangle::Hit's own p = o + t d, in float32
    for k, sun in enumerate(SUNS):
        sd = np.asarray(sun, np.float32)
        sd = np.where(sd == 0, sd, sd / np.float32(np.sqrt(float((sd * sd).sum())))).astype(np.float32)     # (keeps the signed zeros)
        for tmin in (0.0, 1e-4):
            rays = helpers.rays8(p, np.repeat(sd[None], len(p), 0), tmin, FLT_MAX)
            want = _check(gpu_lib, oracle, monkeypatch, sc, "7 sun %d tMin %g" % (k, tmin), rays, problems=problems)
            assert np.isfinite(want["t"]).sum() > len(p) // 4
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", TRIANGLE_SCENES + ["procedural"])
def test_negative_tmin_is_raised_to_zero(gpu_lib, oracle, iscenes, monkeypatch, name):
    """Set 8: a query never reports a hit behind the origin -- tMin < 0 is read as +0 (include/raylib_amd.h; the candidate rule's and the box tests' slack assume
    t >= 0, tests/test_ray_query_host.py pins what the rule does to negative t).  The expectation is the oracle's on the rays with that raise applied here.
    (Before the raise, tMin = -10 and -inf: another t than this expectation on 208 of 1200 rays of the room, 1176 of 2000 of the soup, the same rays on
    every tree; tMin = -1e-3: one ray of the soup.)"""
    sc, problems = iscenes[name], []
    for tmin in (np.float32(-1e-3), np.float32(-10.0), -INF):
        rays = with_interval(sc.rays, tmin, FLT_MAX)
        raised = with_interval(sc.rays, np.where(rays[:, 3] < 0, np.float32(0.0), rays[:, 3]), FLT_MAX)
        want = _check(gpu_lib, oracle, monkeypatch, sc, "8 tMin %r" % float(tmin), rays, oracle_rays=raised, problems=problems)
        assert np.isfinite(want["t"]).sum() > len(rays) // 10 and (want["t"] >= 0).all()
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", ["soup", "room", "cutout8", "cornell"])
def test_small_ray_counts_on_every_tree(gpu_lib, oracle, iscenes, monkeypatch, name):
    """Set 9: the host entry with fewer rays than a wave, a chunk, two chunks -- the 8-wide kernel hands rays out between steps (take, rank, drained) -- on the
    rays of set 1, whose answer is not the full-range one."""
    sc, problems = iscenes[name], []
    have = np.isfinite(sc.T[0])
    rays = with_interval(sc.rays[have], nextup(sc.T[0][have]), FLT_MAX)
    assert len(rays) >= max(SMALL_N)
    for n in SMALL_N:
        want = _check(gpu_lib, oracle, monkeypatch, sc, "9 n = %d" % n, rays[:n], problems=problems)
    assert np.isfinite(want["t"]).sum() >= 0.05 * max(SMALL_N)
    assert not problems, "\n".join(problems)


def test_spheres_and_a_moving_cube(gpu_lib, oracle, iscenes, monkeypatch):
    """Set 10, with sets 1 to 5 on the analytic scene: a sphere's interval is open -- with tMax exactly its t it is dropped, and whatever lies behind it is out
    of range; a cube's is closed -- at rayTime 0, 0.5 and 1, where the cube has moved."""
    from raylib_amd import binding
    sc, problems = iscenes["procedural"], []
    for ray_time in (0.0, 0.5, 1.0):
        full = _check(gpu_lib, oracle, monkeypatch, sc, "10 rayTime %g full range" % ray_time, sc.rays, ray_time, problems=problems)
        kinds = full["prims"][:, 0] & ~0x0fffffff
        sphere = np.isfinite(full["t"]) & (kinds == binding.PRIM_SPHERE)
        cube = np.isfinite(full["t"]) & (kinds == binding.PRIM_CUBE)
        assert sphere.sum() > 200 and cube.sum() > 50, (ray_time, sphere.sum(), cube.sum())
        at = _check(gpu_lib, oracle, monkeypatch, sc, "10 rayTime %g tMax at a sphere" % ray_time, with_interval(sc.rays[sphere], None, full["t"][sphere]), ray_time, problems=problems)
        assert not np.isfinite(at["t"]).any()                                                       # dropped, and nothing else is in range
        at = _check(gpu_lib, oracle, monkeypatch, sc, "10 rayTime %g tMax at a cube" % ray_time, with_interval(sc.rays[cube], None, full["t"][cube]), ray_time, problems=problems)
        assert np.array_equal(bits(at["t"]), bits(full["t"][cube])) and (at["prims"][:, 0] == binding.PRIM_CUBE).all()   # kept
        above = _check(gpu_lib, oracle, monkeypatch, sc, "10 rayTime %g tMax an ulp behind" % ray_time, with_interval(sc.rays, None, nextup(full["t"])), ray_time, problems=problems)
        assert np.array_equal(bits(above["t"]), bits(full["t"]))
        sc.T = helpers.peel(oracle, sc.osc, sc.rays, LAYERS, 1e-4, ray_time)
        assert np.isfinite(sc.T[1]).sum() > 200                                                     # a far root or the sphere behind
        for label, rays, expect in _layer_sets(sc):
            want = _check(gpu_lib, oracle, monkeypatch, sc, "%s rayTime %g" % (label, ray_time), rays, ray_time, problems=problems)
            if expect == "none":
                assert not np.isfinite(want["t"]).any()
            # (set 2 and set 4 end at a surface: a sphere there is out of its open interval, so not every ray hits)
    rng = np.random.RandomState(17)
    a = rng.uniform(0.0, 8.0, len(sc.rays)).astype(np.float32); b = rng.uniform(0.0, 8.0, len(sc.rays)).astype(np.float32)
    _check(gpu_lib, oracle, monkeypatch, sc, "5 random [a, b]", with_interval(sc.rays, a, b), 0.5, problems=problems)
    _check(gpu_lib, oracle, monkeypatch, sc, "5 random [b, a]", with_interval(sc.rays, b, a), 0.5, problems=problems)
    assert not problems, "\n".join(problems)
