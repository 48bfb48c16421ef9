"""Spheres and cubes at their degenerate rays, on the device: SphereHit / CubeHit (csrc/rl_dev_walk.h) and BuildSurface's sphere and cube branches
(csrc/rl_dev_shade.h) as the PRIMS instances of the closest-hit hook and of the ray queries inline them, against the CPU oracle, which
tests/test_analytic_host.py holds to the reference on the same rays (tests/analytic_cases.py).

One comparison for every ray set (_compare): RaylibAMD_ClosestHit and RaylibAMD_TraceRays(SURFACE) give oracle.closest_hit's record byte for byte (NaN meets
NaN), at ray time tau that of the time-shifted scene; CLOSEST misses exactly where oracle.interval_hits' t is +inf and otherwise has its t in bits, one of
its primitives and b1 == b2 == 0; ANY is 1 exactly where it hits.  Two kinds of ray are treated apart, by a condition and never by a tolerance:
  * excused (analytic_cases.Excuser): a primitive the float test accepts fails the box test on its own box -- the answer depends on the tree;
  * tied: the brute force finds two primitives at the least t.  The reference's winner depends on its random tree (out of scope); the device must still
    hit, at that t by value (the one tie of unequal bits is +0 against -0) with one of the tied primitives, and the surface record is not compared.
Every set runs in several wave layouts (analytic_cases.layouts), and an ordinary ray's record must not depend on the wave it is in."""
import ctypes as C

import numpy as np
import pytest

import helpers
from helpers import ffi, bits, nextup, nextdown
import analytic_cases as ac
import test_gpu_ray_query as base
import test_gpu_ray_query_intervals as iv

pytestmark = pytest.mark.gpu

F = np.float32
SEQUENCE = (ac.TAUS[0], ac.TAUS[1], ac.TAUS[2], ac.TAUS[3], ac.TAUS[4], ac.TAUS[5], ac.TAUS[6], ac.TAUS[7], ac.TAUS[0])   # 0, 0.25 and its neighbours, 0.5, 1, 2, -1, 0


class Dev:
    """A scene of analytic_cases on the device, its elements added in the scene's order, and in the oracle with the device's material numbers (every element
    brings its own material: csrc/rl_scene.cc Scene::Finalize)."""

    def __init__(self, lib, oracle, sc):
        from raylib_amd import binding
        self.lib, self.oracle, self.sc, self.name = lib, oracle, sc, sc.name
        rows = ac.material_array(ffi.MAT_DTYPE)
        fp = lambda a: np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
        self.mats, self.elems = [], []
        sph, cub = sc.spheres.copy(), sc.cubes.copy()
        for kind, i in sc.order:
            m = binding.create_material(lib, rows[ac.MAT_SPHERE if kind == "s" else ac.MAT_CUBE]); self.mats.append(m)
            if kind == "s":
                s = sc.spheres[i]; sph["material"][i] = len(self.elems)
                self.elems.append(lib.RaylibAMD_CreateSphere(float(s["center"][0]), float(s["center"][1]), float(s["center"][2]), float(s["radius"]), m))
            else:
                c = sc.cubes[i]; cub["material"][i] = len(self.elems)
                self.elems.append(lib.RaylibAMD_CreateCube(f3(c["minBounds"]), f3(c["maxBounds"]), float(c["timeStartMove"]), f3(c["velocity"]), m))
        for v, n, uv, _ in sc.triangles:
            m = binding.create_material(lib, rows[ac.MAT_TRI]); self.mats.append(m)
            self.elems.append(lib.RaylibAMD_CreateTriangle(fp(v[0]), fp(v[1]), fp(v[2]), fp(n[0]), fp(n[1]), fp(n[2]), fp(uv), m))
        assert all(self.mats) and all(self.elems)
        self.scene = lib.Raylib_CreateScene()
        for e in self.elems:
            lib.Raylib_AddSceneElement(self.scene, e)
        lib.Raylib_FinalizeScene(self.scene)
        for kind in (binding.QUERY_ANY, binding.QUERY_CLOSEST, binding.QUERY_SURFACE):
            rc, plan = binding.plan_ray_query(lib, self.scene, kind)
            assert rc == 1 and plan["prims"] == 1 and plan["treeWidth"] == 2, (sc.name, plan)     # the binary tree is the only one that carries primitives
        self.tris, self.matrows = binding.SceneSession.export_flat(self)
        assert len(self.tris) == len(sc.triangles)
        self.dsc = ac.Scene(sc.name, sph, cub, sc.order, sc.triangles)
        self.handles = {}
        self.osc = self.at(0.0)
        self.excuser = ac.Excuser(oracle, self.dsc, lambda s: ffi.FlatScene(np.zeros(0, ffi.TRI_DTYPE), self.matrows, spheres=s.spheres, cubes=s.cubes, num_shapes=0))
        self.q = iv.Scene(sc.name, self, self.osc, self.tris, {2})      # for test_gpu_ray_query_intervals._check

    def at(self, tau):
        """The oracle's scene whose ray time 0 is this scene's ray time tau"""
        key = bits(F(tau)).item()
        if key not in self.handles:
            s = self.dsc.at(tau) if key != 0 else self.dsc
            flat = ffi.FlatScene(self.tris, self.matrows, spheres=s.spheres, cubes=s.cubes, num_shapes=None if len(self.tris) else 0)
            self.handles[key] = self.oracle.scene_create(flat, 1)
        return self.handles[key]

    def close(self):
        lib = self.lib
        self.excuser.close()
        for h in self.handles.values():
            self.oracle.scene_destroy(h)
        lib.Raylib_DestroyScene(self.scene)
        for e in self.elems:
            lib.RaylibAMD_DestroySceneElement(e)
        for m in self.mats:
            lib.RaylibAMD_DestroyMaterial(m)


@pytest.fixture(scope="module")
def S():
    return ac.scenes()


@pytest.fixture(scope="module")
def fams(S):
    return ac.families(S)


@pytest.fixture(scope="module")
def devs(gpu_lib, oracle, S):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Dev(gpu_lib, oracle, S[name])
        return made[name]
    yield get
    for d in made.values():
        d.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _rows(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _compare(lib, dev, r6, tmin, tau, label, problems, hook=False):
    """The one comparison (module docstring) of rays6 `r6` over [tmin, FLT_MAX] at ray time tau.  Differences go to `problems`; returns (the device's CLOSEST
    and SURFACE records, the brute force's records, the excused rays)."""
    from raylib_amd import binding
    oracle = dev.oracle
    r6 = np.ascontiguousarray(r6, F)
    r8 = ac.rays8(r6, tmin)
    brute = oracle.interval_hits(dev.osc, r8, float(tau))
    want = ac.canonical(oracle.closest_hit(dev.at(tau), r6, tmin))
    excused = dev.excuser(r8, tau)
    hit, tied = np.isfinite(brute["t"]), brute["count"] > 1
    ok = ~excused
    closest = binding.trace_rays(lib, dev.scene, r8, binding.QUERY_CLOSEST, float(tau))
    surf, sprim = binding.trace_rays(lib, dev.scene, r8, binding.QUERY_SURFACE, float(tau), with_prim=True)
    anyhit = binding.trace_rays(lib, dev.scene, r8, binding.QUERY_ANY, float(tau))

    def report(what, bad, extra=None):
        if bad.any():
            i = int(np.argmax(bad))
            problems.append("%s / %s / tMin %r / rayTime %r: %s on %d of %d rays; first ray %d %s (bits %s): brute force %s, tree walk %s%s" % (
                dev.name, label, float(tmin), float(tau), what, bad.sum(), len(r6), i, r6[i].tolist(), [hex(b) for b in bits(r6[i])], brute[i], want[i],
                "" if extra is None else ", device %s" % (extra[i],)))

    got = closest["prim"] >= 0
    report("CLOSEST hits where the oracle misses", ok & got & ~hit, closest)
    report("CLOSEST misses where the oracle hits", ok & ~got & hit, closest)
    both = ok & got & hit
    report("CLOSEST t differs in bits", both & ~tied & (bits(closest["t"]) != bits(brute["t"])), closest)
    report("CLOSEST t differs in value at a tie", both & tied & ~(closest["t"] == brute["t"]), closest)
    report("CLOSEST prim is none of the oracle's", both & (brute["count"] <= 8) & ~(closest["prim"][:, None] == brute["prims"]).any(1), closest)
    prim = both & (closest["prim"] >= ac.PRIM_SPHERE)
    report("a sphere's or cube's b1, b2 are not +0", prim & ((bits(closest["b1"]) != 0) | (bits(closest["b2"]) != 0)), closest)
    report("CLOSEST miss record is not (0, -1, 0, 0)", ~got & ((bits(closest["t"]) != 0) | (closest["prim"] != -1) | (bits(closest["b1"]) != 0) | (bits(closest["b2"]) != 0)), closest)
    report("ANY is not 1 exactly where the oracle hits", ok & (anyhit != hit.astype(np.uint32)), anyhit)
    report("ANY differs from CLOSEST", anyhit != got.astype(np.uint32), anyhit)
    report("SURFACE outPrim is not CLOSEST's prim", sprim != closest["prim"], sprim)
    differs = (_rows(ac.canonical(surf)) != _rows(want)).any(1)
    report("SURFACE record differs from oracle.closest_hit's in bytes", ok & ~tied & differs, surf)
    report("SURFACE hit or t differs at a tie", ok & tied & ((surf["hit"] != 1) | ~(surf["t"] == brute["t"])), surf)
    if hook:
        assert float(tau) == 0.0
        hk = base._hook(lib, dev.scene, r8, float(tmin))
        report("RaylibAMD_ClosestHit's record differs from TraceRays(SURFACE)'s in bytes", (_rows(ac.canonical(hk)) != _rows(ac.canonical(surf))).any(1), hk)
    return closest, surf, brute, excused


GROUPS = {"sphere1": ac.SPHERE_FAMILIES, "cube1": ac.CUBE_FAMILIES, "cube1m": tuple(k + "_m" for k in ac.CUBE_FAMILIES), "many": ("special", "regular_many"),
          "huge": ("flt_max",)}


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_records_equal_the_oracles_in_every_layout(gpu_lib, devs, fams, name):
    """Every family of the scene at tMin 1e-4, 0 and -0 in every wave layout; the hook at 1e-4 and 0.  An ordinary ray gives the record it gives alone."""
    dev, problems = devs(name), []
    mine = {k: fams[k][1] for k in GROUPS[name]}
    assert all(fams[k][0] == name for k in mine)
    reg = ac.regular(dev.sc, 1024)
    alone = {}
    for tmin in ac.TMINS:
        alone[bits(tmin).item()] = _compare(gpu_lib, dev, reg, tmin, 0.0, "ordinary rays", problems)[:2]
    n = x = 0
    for label, r6, src in ac.layouts(mine, reg):
        for tmin in ac.TMINS:
            closest, surf, brute, excused = _compare(gpu_lib, dev, r6, tmin, 0.0, label, problems, hook=bits(tmin).item() != 0x80000000)
            n += len(r6); x += int(excused.sum())
            r = src >= 0
            a = alone[bits(tmin).item()]
            if (_rows(closest)[r] != _rows(a[0])[src[r]]).any() or (_rows(ac.canonical(surf))[r] != _rows(ac.canonical(a[1]))[src[r]]).any():
                problems.append("%s / %s / tMin %r: an ordinary ray's record depends on its wave" % (name, label, float(tmin)))
        print("%-8s %-28s %6d rays, %5d hits at tMin 0" % (name, label, len(r6), np.isfinite(brute["t"]).sum()))
    print("%s: %d rays asked, %d excused" % (name, n, x))
    assert x <= 0.001 * n
    assert not problems, "\n".join(problems[:12])


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_intervals_end_at_the_hit(gpu_lib, oracle, devs, fams, monkeypatch, name):
    """The hitting rays of every family again with tMax at the oracle's t, at the float above and at the float below, and with tMin at t: a sphere's interval
    is open, a cube's closed (test_gpu_ray_query_intervals._check on the rays that are neither excused nor tied at +-0)."""
    dev, problems = devs(name), []
    kinds = {"sphere": 0, "cube": 0}
    for k in GROUPS[name]:
        r6 = fams[k][1]
        for tmin in ac.TMINS:
            full = oracle.interval_hits(dev.osc, ac.rays8(r6, tmin), 0.0)
            for label, r8 in ac.interval_sets(r6, tmin, full["t"]):
                pre = oracle.interval_hits(dev.osc, r8, 0.0)
                keep = ~dev.excuser(r8) & ~((pre["count"] > 1) & (pre["t"] == 0))
                want = iv._check(gpu_lib, oracle, monkeypatch, dev.q, "%s tMin %r %s" % (k, float(tmin), label), r8[keep], problems=problems)
                if label == "tMax = t":       # what is left is a cube, or a sphere's far root ... never the sphere the ray met at t
                    t = full["t"][np.isfinite(full["t"])][keep]
                    first = full["prims"][np.isfinite(full["t"])][keep][:, 0]
                    alone = full["count"][np.isfinite(full["t"])][keep] == 1
                    sphere, cube = alone & (first >= ac.PRIM_SPHERE) & (first < ac.PRIM_CUBE), alone & (first >= ac.PRIM_CUBE)
                    kinds["sphere"] += int(sphere.sum()); kinds["cube"] += int(cube.sum())
                    assert not ((want["t"] == t) & sphere).any(), (k, label)
                    assert np.array_equal(bits(want["t"][cube]), bits(t[cube])), (k, label)
    print(name, kinds)
    assert not problems, "\n".join(problems[:12])


def test_a_cube_at_tmax_is_not_shadowed_by_a_sphere_at_tmax(gpu_lib, oracle, devs, S, monkeypatch):
    """A sphere of radius 1 and a cube whose face touches it, met by an axis ray at one float t, in six directions and both orders of adding them.  tMax = t
    leaves the cube alone in range (its interval is closed, the sphere's open): the query must report it whichever leaf the walk reaches first.  With
    tMax an ulp above either primitive is accepted -- the walk's first wins, printed -- and both orders must occur; an ulp below, a miss."""
    from raylib_amd import binding
    problems, winners = [], {}
    for name in ac.TIE_SCENES:
        dev = devs(name)
        r6 = ac.tie_rays(S[name])
        full = oracle.interval_hits(dev.osc, ac.rays8(r6, 0.0), 0.0)
        assert (full["count"] == 2).all()
        t = full["t"]
        up = binding.trace_rays(gpu_lib, dev.scene, ac.rays8(r6, 0.0, nextup(t)), binding.QUERY_CLOSEST, 0.0)
        winners[name] = sorted(set("sphere" if p < ac.PRIM_CUBE else "cube" for p in up["prim"]))
        print("%-10s tMax = nextup(t): the walk's first is the %s" % (name, " and the ".join(winners[name])))
        iv._check(gpu_lib, oracle, monkeypatch, dev.q, "tMax = nextup(t)", ac.rays8(r6, 0.0, nextup(t)), problems=problems)
        iv._check(gpu_lib, oracle, monkeypatch, dev.q, "full range", ac.rays8(r6, 0.0), problems=problems)
        below = iv._check(gpu_lib, oracle, monkeypatch, dev.q, "tMax = nextdown(t)", ac.rays8(r6, 0.0, nextdown(t)), problems=problems)
        assert not np.isfinite(below["t"]).any()
        at = ac.rays8(r6, 0.0, t)
        want = iv._check(gpu_lib, oracle, monkeypatch, dev.q, "tMax = t", at, problems=problems)
        assert (want["count"] == 1).all() and (want["prims"][:, 0] == ac.PRIM_CUBE).all()
        got = binding.trace_rays(gpu_lib, dev.scene, at, binding.QUERY_CLOSEST, 0.0)
        surf = binding.trace_rays(gpu_lib, dev.scene, at, binding.QUERY_SURFACE, 0.0)
        anyhit = binding.trace_rays(gpu_lib, dev.scene, at, binding.QUERY_ANY, 0.0)
        if not ((got["prim"] == ac.PRIM_CUBE).all() and np.array_equal(bits(got["t"]), bits(t)) and (surf["hit"] == 1).all() and (anyhit == 1).all()):
            problems.append("%s: with tMax == t the cube is not reported: prim %s" % (name, got["prim"].tolist()))
    firsts = set(w for v in winners.values() for w in v)
    assert firsts == {"sphere", "cube"}, "the arrangements reach one order only: %s" % winners
    assert not problems, "\n".join(problems[:12])


def test_a_quad_on_a_cube_face_and_a_triangle_tangent_to_a_sphere(gpu_lib, oracle, devs, S, monkeypatch):
    dev, problems = devs("mixed"), []
    r6 = ac.mixed_rays(S["mixed"])
    for tmin in ac.TMINS:
        r8 = ac.rays8(r6, tmin)
        keep = ~dev.excuser(r8)
        want = iv._check(gpu_lib, oracle, monkeypatch, dev.q, "mixed tMin %r" % float(tmin), r8[keep], problems=problems)
        tri = (want["prims"] >= 0) & (want["prims"] < ac.PRIM_SPHERE)
        with_cube = (want["count"] == 2) & tri.any(1) & (want["prims"] >= ac.PRIM_CUBE).any(1)
        with_sphere = (want["count"] == 2) & tri.any(1) & ((want["prims"] >= ac.PRIM_SPHERE) & (want["prims"] < ac.PRIM_CUBE)).any(1)
        assert (with_cube & (want["t"] == 2.5)).sum() >= 40 and (with_sphere & (want["t"] == 2.5)).sum() >= 1, (with_cube.sum(), with_sphere.sum())   # the vertical rays
        for label, q in ac.interval_sets(r6[keep], tmin, want["t"]):
            iv._check(gpu_lib, oracle, monkeypatch, dev.q, "mixed tMin %r %s" % (float(tmin), label), q[~dev.excuser(q)], problems=problems)
    assert not problems, "\n".join(problems[:12])


@pytest.mark.parametrize("name", ["cube1m", "many"])
def test_ray_times_in_sequence(gpu_lib, devs, fams, name):
    """One scene asked at ray time 0, 0.25 and the floats beside it, 0.5, 1, 2 (beyond the interval its boxes were built for), -1, then 0 again: each against
    the time-shifted oracle scene, the cube families built on the cube's bounds at that time; the last call gives the first call's bytes."""
    from raylib_amd import binding
    dev, problems = devs(name), []
    reg = ac.regular(dev.sc, 2048)
    fixed = np.concatenate([reg] + [fams[k][1][ac.subsample(len(fams[k][1]), 2048, 9)] for k in GROUPS[name]])
    first = None
    for step, tau in enumerate(SEQUENCE):
        sets = [("fixed", fixed)]
        if name == "cube1m":
            sets += sorted(ac.moved_cube_families(tau).items())
        for label, r6 in sets:
            for tmin in (ac.TMINS[0], ac.TMINS[1]):
                closest, surf, brute, excused = _compare(gpu_lib, dev, r6, tmin, tau, "step %d %s" % (step, label), problems)
                assert excused.sum() <= 0.001 * len(r6) + 1
                if label == "fixed" and bits(tmin).item() == 0:
                    anyhit = binding.trace_rays(gpu_lib, dev.scene, ac.rays8(r6, tmin), binding.QUERY_ANY, float(tau))
                    blob = closest.tobytes() + surf.tobytes() + anyhit.tobytes()
                    print("%s step %d rayTime %-12r %5d of %d rays hit" % (name, step, float(tau), np.isfinite(brute["t"]).sum(), len(r6)))
                    if step == 0:
                        first = blob
                    elif step == len(SEQUENCE) - 1:
                        assert blob == first, "ray time 0 after the sequence does not give the bytes it gave before"
    assert not problems, "\n".join(problems[:12])
