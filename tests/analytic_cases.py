"""Scenes and ray families that hold the two analytic primitives -- SphereHit / CubeHit (csrc/rl_dev_walk.h) and the sphere and cube branches of BuildSurface
(csrc/rl_dev_shade.h) -- to the reference at their degenerate rays: tangents, origins on and inside a primitive, zero and negative-zero direction
components, rays in a cube's face planes and through its edges and corners, a sphere's poles, special values, and a sphere and a cube at the same float t.

NumPy only, deterministic (np.random.RandomState).  tests/test_analytic_host.py, tests/test_gpu_analytic_edges.py and tests/golden/gen_golden.py import it.
A checker (oracle.ffi.Checker) is only ever an argument.

Every scene has at most 8 primitives.  Spheres carry material 0, cubes material 1, triangles material 2: a record says which kind it met."""
import hashlib

import numpy as np

F = np.float32
FLT_MAX = F(3.4028235e38)
DENORM = F(1e-45)
MAT_SPHERE, MAT_CUBE, MAT_TRI = 0, 1, 2
PRIM_SPHERE, PRIM_CUBE = 0x10000000, 0x20000000

SPHERE_DTYPE = np.dtype([("center", "f4", 3), ("radius", "f4"), ("material", "i4")])                                                              # = oracle.ffi's
CUBE_DTYPE = np.dtype([("minBounds", "f4", 3), ("maxBounds", "f4", 3), ("timeStartMove", "f4"), ("velocity", "f4", 3), ("material", "i4")])

TMINS = (F(1e-4), F(0.0), F(-0.0))
TAUS = (F(0.0), F(0.25), np.nextafter(F(0.25), F(1)), np.nextafter(F(0.25), F(0)), F(0.5), F(1.0), F(2.0), F(-1.0))
SUBSAMPLE = 256          # rays per family whose reference records tests/golden/analytic_edges.npz stores


def nudge(x, k):
    """x moved by k units in the last place (x != 0)"""
    return (np.asarray(x, F).view(np.int32) + np.asarray(k, np.int32) * np.where(np.asarray(x, F) < 0, -1, 1).astype(np.int32)).view(F)


def spheres(*rows):
    a = np.zeros(len(rows), SPHERE_DTYPE)
    for i, (c, r) in enumerate(rows):
        a[i] = (c, r, MAT_SPHERE)
    return a


def cubes(*rows):
    a = np.zeros(len(rows), CUBE_DTYPE)
    for i, (mn, mx, t0, v) in enumerate(rows):
        a[i] = (mn, mx, t0, v, MAT_CUBE)
    return a


class Scene:
    """spheres, cubes: the records; order: the elements in the order they are added to a device scene ("s", i) / ("c", i) -- the flat scene of the oracle
    has no order; triangles: (v (3, 3), n (3, 3), uv (6,), material) rows for RaylibAMD_CreateTriangle."""

    def __init__(self, name, sph=None, cub=None, order=None, triangles=()):
        self.name = name
        self.spheres = spheres() if sph is None else sph
        self.cubes = cubes() if cub is None else cub
        self.order = order or [("s", i) for i in range(len(self.spheres))] + [("c", i) for i in range(len(self.cubes))]
        self.triangles = list(triangles)
        assert len(self.spheres) + len(self.cubes) <= 8

    def at(self, tau):
        """The scene whose cubes compute at ray time 0 the float32 movement this scene's compute at ray time tau: timeStartMove' = -fl(tau - timeStartMove),
        0 where that is not positive (CubeHit: velocity * max(0, rayTime - timeStartMove))."""
        c = self.cubes.copy()
        dt = (F(tau) - c["timeStartMove"]).astype(F)
        c["timeStartMove"] = np.where(dt > 0, -dt, F(0.0)).astype(F)
        return Scene("%s@%r" % (self.name, float(tau)), self.spheres, c, self.order, self.triangles)

    def movement(self, tau):
        """(cubes, 3) float32: velocity * max(0, tau - timeStartMove), in CubeHit's order of operations"""
        s = np.maximum(F(0.0), (F(tau) - self.cubes["timeStartMove"]).astype(F)).astype(F)
        return (self.cubes["velocity"] * s[:, None]).astype(F)

    def boxes(self, tau=0.0):
        """(spheres + cubes, 6) float32: each primitive's own box at ray time tau, spheres first"""
        m = self.movement(tau)
        sb = np.concatenate([self.spheres["center"] - self.spheres["radius"][:, None], self.spheres["center"] + self.spheres["radius"][:, None]], 1).astype(F)
        cb = np.concatenate([self.cubes["minBounds"] + m, self.cubes["maxBounds"] + m], 1).astype(F)
        return np.concatenate([sb.reshape(-1, 6), cb.reshape(-1, 6)])

    def singles(self):
        """One scene per primitive, in the order of boxes()"""
        return [Scene("%s/s%d" % (self.name, i), sph=self.spheres[i:i + 1]) for i in range(len(self.spheres))] + \
               [Scene("%s/c%d" % (self.name, i), cub=self.cubes[i:i + 1]) for i in range(len(self.cubes))]

    def bounds(self):
        b = self.boxes(0.0)
        b = b[np.isfinite(b).all(1)]
        return b[:, :3].min(0), b[:, 3:].max(0)


def materials():
    """three Lambertian materials as oracle.ffi.MAT_DTYPE rows (the caller gives the dtype)"""
    rows = []
    for albedo in ((0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.3, 0.3, 0.8)):
        rows.append(dict(type=0, albedo=albedo, roughness=1.0, ior=1.5))
    return rows


def material_array(dtype):
    m = np.zeros(3, dtype)
    for i, r in enumerate(materials()):
        m[i]["type"] = r["type"]; m[i]["albedo"] = r["albedo"]; m[i]["roughness"] = r["roughness"]; m[i]["ior"] = r["ior"]
        for k in ("texAlbedo", "texNormal", "texRoughness", "texMetallic", "texEmissive"):
            m[i][k] = -1
    return m


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
C1, R1 = np.array((0.25, -0.5, 0.125), F), F(0.75)
MN1, MX1 = np.array((-0.5, -0.25, -0.375), F), np.array((0.75, 0.5, 0.5), F)      # extents 1.25, 0.75, 0.875: eighths, so that power-of-two offsets stay exact
V1 = (0.5, -0.25, 0.125)
AXES = [(a, s) for a in range(3) for s in (1, -1)]


def _tie(axis, sign, cube_first):
    mn, mx = np.full(3, -0.25, F), np.full(3, 0.25, F)
    mn[axis], mx[axis] = (0.5, 1.0) if sign > 0 else (-1.0, -0.5)
    order = [("c", 0), ("s", 0)] if cube_first else [("s", 0), ("c", 0)]
    return Scene("tie_%s%s_%s" % ("+" if sign > 0 else "-", "xyz"[axis], "cs" if cube_first else "sc"), spheres(((0, 0, 0), 1.0)), cubes((mn, mx, 0.0, (0, 0, 0))), order)


def _quad(corners, normal):
    p = np.asarray(corners, F)
    n = np.tile(np.asarray(normal, F), (3, 1))
    return [(p[[0, 1, 2]], n, np.asarray([0, 0, 1, 0, 1, 1], F), MAT_TRI), (p[[0, 2, 3]], n, np.asarray([0, 0, 1, 1, 0, 1], F), MAT_TRI)]


def scenes():
    S = {}
    S["sphere1"] = Scene("sphere1", spheres((C1, R1)))
    S["cube1"] = Scene("cube1", cub=cubes((MN1, MX1, 0.0, (0, 0, 0))))
    S["cube1m"] = Scene("cube1m", cub=cubes((MN1, MX1, 0.0, V1)))
    S["many"] = Scene("many",
                      spheres((C1, R1), ((1.5, 0.0, -1.0), 0.3), ((0.0, 0.3, -4.0), 2.0), ((-1.0, 1.0, 0.5), 0.0), ((1.0, 1.0, 0.5), 1e-3)),
                      cubes(((-2.0, -0.25, -0.25), (-1.5, 0.25, 0.25), 0.0, (0.0, 1.0, 0.0)),
                            ((1.25, -1.5, -0.5), (1.75, -1.0, 0.25), 0.25, (-0.5, 0.25, 0.125)),
                            ((-0.75, 1.0, -0.5), (-0.75, 1.5, 0.5), 0.0, (0.0, 0.0, 0.0))))      # zero thickness: min.x == max.x
    # FLT_MAX as a hit distance (flt_max below): a sphere of radius 2^58 around the origin, a cube whose -x face is the float below 2
    S["huge"] = Scene("huge", spheres(((0, 0, 0), 2.0 ** 58)), cubes(((np.nextafter(F(2), F(0)), -1.0, -1.0), (3.0, 1.0, 1.0), 0.0, (0, 0, 0))))
    for axis, sign in AXES:
        for cube_first in (False, True):
            sc = _tie(axis, sign, cube_first)
            S[sc.name] = sc
    # a quad coincident with a cube's +z face, a triangle tangent to a sphere at its +z pole, one free sphere, one free cube
    tris = _quad(((1, -0.5, 0.5), (2, -0.5, 0.5), (2, 0.5, 0.5), (1, 0.5, 0.5)), (0, 0, 1))
    tris.append((np.asarray(((-2.5, -1, 0.5), (-0.5, -1, 0.5), (-1.5, 1.5, 0.5)), F), np.tile(np.asarray((0, 0, 1), F), (3, 1)), np.asarray([0, 0, 1, 0, 0.5, 1], F), MAT_TRI))
    S["mixed"] = Scene("mixed", spheres(((-1.5, 0.0, 0.0), 0.5), ((0.0, 1.5, 0.0), 0.4)),
                       cubes(((1.0, -0.5, -0.5), (2.0, 0.5, 0.5), 0.0, (0, 0, 0)), ((-0.3, -2.0, -0.3), (0.3, -1.4, 0.3), 0.0, (0, 0, 0))), triangles=tris)
    return S


TIE_SCENES = ["tie_%s%s_%s" % ("+" if s > 0 else "-", "xyz"[a], o) for a, s in AXES for o in ("sc", "cs")]


# ---- rays ------------------------------------------------------------------------------------------------------------------------------
def rays6(o, d):
    o, d = np.asarray(o, F), np.asarray(d, F)
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(o, d.shape), d], 1), F)


def rays8(r6, tmin=1e-4, tmax=FLT_MAX):
    """n x (org, tMin, dir, tMax), the layout of RaylibAMDRay"""
    r = np.zeros((len(r6), 8), F)
    r[:, 0:3] = r6[:, 0:3]; r[:, 3] = tmin; r[:, 4:7] = r6[:, 3:6]; r[:, 7] = tmax
    return r


def r6_of(r8):
    return np.ascontiguousarray(np.concatenate([r8[:, 0:3], r8[:, 4:7]], 1), F)


def _unit(rng, n):
    """n unit vectors, uniform on the sphere, by rejection from the cube: additions, multiplications, a square root and a division, each correctly
    rounded everywhere -- the rays must come out the same bytes on every machine (the fixture holds their hash, not the rays)"""
    v = rng.uniform(-1.0, 1.0, (3 * n + 64, 3))
    q = (v * v).sum(1)
    v, q = v[(q <= 1.0) & (q > 1e-4)][:n], q[(q <= 1.0) & (q > 1e-4)][:n]
    assert len(v) == n
    return v / np.sqrt(q)[:, None]


def _perp(u, rng):
    w = np.cross(u, _unit(rng, len(u)))
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def regular(sc, n, seed=101):
    """Ordinary rays of a scene: origins on a sphere around it, aimed into its bounds"""
    rng = np.random.RandomState(seed)
    lo, hi = sc.bounds()
    mid, ext = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.5)
    o = (mid + _unit(rng, n) * (2.5 * np.linalg.norm(ext))).astype(F)
    tgt = rng.uniform(mid - 1.2 * ext, mid + 1.2 * ext, (n, 3)).astype(F)
    return rays6(o, (tgt - o).astype(F))


def tangent_axis():
    """Axis-parallel rays past sphere1 at r +- 64 ulp from the axis through its centre, from distances 3, 10 and 100; per group of 129 consecutive
    rays only the offset moves, one ulp per ray."""
    ks = np.arange(-64, 65)
    rk = nudge(np.full(129, R1, F), ks)
    rdk = nudge(np.full(129, F(R1 / np.sqrt(2.0)), F), ks)
    out = []
    for axis, sign in AXES:
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for dist in (3.0, 10.0, 100.0):
            for su, sv, off in ((1, 0, rk), (-1, 0, rk), (0, 1, rk), (0, -1, rk), (1, 1, rdk), (1, -1, rdk), (-1, 1, rdk), (-1, -1, rdk)):
                o = np.zeros((129, 3), F); d = np.zeros((129, 3), F)
                o[:, axis] = C1[axis] + F(sign * dist)
                o[:, u] = C1[u] + F(su) * off
                o[:, v] = C1[v] + F(sv) * off
                d[:, axis] = -sign
                out.append(rays6(o, d))
    return np.concatenate(out)


def tangent_generic(n=20000, seed=102):
    """Pairs of rays from distances 1 to 100 aimed at sphere1's tangent points moved in or out by 1e-9 .. 1e-3 of the radius; the second ray of a pair
    aims one ulp (of the target's largest component) beside the first."""
    rng = np.random.RandomState(seed)
    m = n // 2
    u = _unit(rng, m); w = _perp(u, rng)
    dist = np.array((1.0, 10.0))[rng.randint(0, 2, m)] * rng.uniform(1.0, 10.0, m)        # (no exp, log or pow: see _unit)
    o = (C1 + u * dist[:, None]).astype(F)
    sin_a = np.minimum(R1 / dist, 1.0); cos_a = np.sqrt(1.0 - sin_a * sin_a)
    eps = np.array((1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4))[rng.randint(0, 6, m)] * rng.uniform(1.0, 10.0, m) * rng.choice((-1.0, 1.0), m)
    p = (C1 + (R1 * (1.0 + eps))[:, None] * (sin_a[:, None] * u + cos_a[:, None] * w)).astype(F)
    k = np.argmax(np.abs(p), 1)
    p2 = p.copy()
    p2[np.arange(m), k] = nudge(p[np.arange(m), k], 1)
    d1, d2 = (p - o).astype(F), (p2 - o).astype(F)
    r = np.zeros((2 * m, 6), F)
    r[0::2] = rays6(o, d1); r[1::2] = rays6(o, d2)
    return r


def on_surface(n=4000, seed=103):
    """Origins on sphere1 as nearly as float32 allows; the last 120 at the six axis points, where c = |oc|^2 - r^2 is exactly 0 and one root is t = 0"""
    rng = np.random.RandomState(seed)
    o = (C1 + R1 * _unit(rng, n)).astype(F)
    for i, (axis, sign) in enumerate(AXES):
        o[n - 120 + 20 * i:n - 100 + 20 * i] = C1
        o[n - 120 + 20 * i:n - 100 + 20 * i, axis] = C1[axis] + F(sign) * R1
    d = _unit(rng, n).astype(F)
    for i, (axis, sign) in enumerate(AXES):
        d[n - 120 + 20 * i] = 0; d[n - 120 + 20 * i, axis] = sign
        d[n - 119 + 20 * i] = 0; d[n - 119 + 20 * i, axis] = -sign
    return rays6(o, d)


def inside(n=4000, seed=104):
    rng = np.random.RandomState(seed)
    rho = rng.uniform(0, 1, (n, 3)).max(1)[:, None]      # distributed as the cube root of a uniform number
    return rays6((C1 + R1 * rho * 0.999 * _unit(rng, n)).astype(F), _unit(rng, n).astype(F))


def centre(n=4000, seed=105):
    rng = np.random.RandomState(seed)
    return rays6(np.tile(C1, (n, 1)), _unit(rng, n).astype(F))


def poles(seed=106):
    """3000 rays aimed at sphere1's six axis points: from within 45 degrees of the axis, from the axis itself (p lands on the pole: atan(0 / 0) at +-z), from a
    coordinate plane through the axis.  (No grazing rays, which the tangent families hold: next to a pole -- a point ON the face of the sphere's box -- the
    discriminant's cancellation put 6 of 3000 roots of grazing rays further outside the box than the walks' box slack, twice the excused set's cap.)"""
    rng = np.random.RandomState(seed)
    out = []

    def around(e, n):
        u = _unit(rng, n)
        u = np.where((u @ e)[:, None] < 0, -u, u) + e
        return u / np.linalg.norm(u, axis=1, keepdims=True)
    for axis, sign in AXES:
        e = np.zeros(3); e[axis] = sign
        pole = C1.copy(); pole[axis] = C1[axis] + F(sign) * R1
        o = (pole + around(e, 250) * rng.uniform(1, 4, (250, 1))).astype(F)
        out.append(rays6(o, (pole - o).astype(F)))
        o = np.tile(C1, (125, 1)); o[:, axis] = C1[axis] + (sign * rng.choice((1.0, 1.5, 2.0, 3.0, 4.75, 10.0), 125)).astype(F)
        d = np.zeros((125, 3), F); d[:, axis] = -sign * rng.choice((1.0, 0.5, 2.0, 0.75), 125)
        out.append(rays6(o, d))
        o = (pole + around(e, 125) * rng.uniform(1, 4, (125, 1))).astype(F)
        o[:, (axis + 1) % 3] = C1[(axis + 1) % 3]
        out.append(rays6(o, (pole - o).astype(F)))
    return np.concatenate(out)


DIR_COMPONENTS = np.array((0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30, 0.5, -0.25), F)


def cube_axis(mn, mx, n=60000, seed=107):
    """Every origin coordinate from the cube's planes +- 2 ulp, the middle or outside; every direction component from DIR_COMPONENTS"""
    rng = np.random.RandomState(seed)
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    o = np.zeros((n, 3), F)
    for a in range(3):
        cand = np.concatenate([nudge(np.full(5, mn[a], F), np.arange(-2, 3)), nudge(np.full(5, mx[a], F), np.arange(-2, 3)),
                               np.array(((mn[a] + mx[a]) / 2, mn[a] - 1, mx[a] + 1), F)]).astype(F)
        o[:, a] = cand[rng.randint(0, len(cand), n)]
    d = DIR_COMPONENTS[rng.randint(0, len(DIR_COMPONENTS), (n, 3))]
    return rays6(o, d)


def cube_corner(mn, mx):
    """Rays through the 8 corners and the 12 edge midpoints from power-of-two offsets: on the static cube the entry planes tie exactly (t1 == t3 == t5 at a
    corner, two of them at an edge); along an edge the direction component is +0, -0 or +-1/8"""
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    B = (mn, mx)
    E = (0.5, 1.0, 2.0, 4.0)
    o, d = [], []
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                X = np.array((B[cx][0], B[cy][1], B[cz][2]), F)
                s = np.array((2 * cx - 1, 2 * cy - 1, 2 * cz - 1), F)
                for i in E:
                    for j in E:
                        for k in E:
                            off = (s * np.array((i, j, k), F)).astype(F)
                            o.append((X + off).astype(F)); d.append(-off)
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for cu in (0, 1):
            for cv in (0, 1):
                X = ((mn + mx) / 2).astype(F); X[u] = B[cu][u]; X[v] = B[cv][v]
                for i in E:
                    for j in E:
                        for along in (0.0, -0.0, 0.125, -0.125):
                            off = np.zeros(3, F); off[u] = (2 * cu - 1) * i; off[v] = (2 * cv - 1) * j
                            dd = -off; dd[axis] = along
                            o.append((X + off - np.where(np.arange(3) == axis, F(along), F(0))).astype(F)); d.append(dd.astype(F))
    return rays6(np.array(o, F), np.array(d, F))


def _some_axis_parallel(rng, d, share=0.2):
    z = rng.uniform(0, 1, len(d)) < share
    a = rng.randint(0, 3, len(d))
    d[z, a[z]] = rng.choice((0.0, -0.0), int(z.sum()))
    return d.astype(F)


def cube_inside(mn, mx, n=5000, seed=108):
    rng = np.random.RandomState(seed)
    mn, mx = np.asarray(mn, np.float64), np.asarray(mx, np.float64)
    o = (mn + (mx - mn) * rng.uniform(0.01, 0.99, (n, 3))).astype(F)
    return rays6(o, _some_axis_parallel(rng, _unit(rng, n)))


def cube_onface(mn, mx, n=5000, seed=109):
    rng = np.random.RandomState(seed)
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    o = (mn + (mx - mn).astype(np.float64) * rng.uniform(0.01, 0.99, (n, 3))).astype(F)
    a, hi = rng.randint(0, 3, n), rng.randint(0, 2, n)
    o[np.arange(n), a] = np.where(hi == 1, mx[a], mn[a])
    return rays6(o, _some_axis_parallel(rng, _unit(rng, n)))


SPECIAL = np.array((0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 1e-20, -1e-20, 1e20, -1e20, 3e38, -3e38, np.inf, -np.inf, np.nan), F)


def special(sc, n=40000, seed=110):
    """Ordinary rays of `sc` with each component replaced, one time in two, by a special value"""
    rng = np.random.RandomState(seed)
    r = regular(sc, n, seed + 1000)
    pick = rng.uniform(0, 1, r.shape) < 0.5
    r[pick] = SPECIAL[rng.randint(0, len(SPECIAL), int(pick.sum()))]
    return np.ascontiguousarray(r, F)


def flt_max():
    """Scene `huge`: the sphere's far root from inside, (-b + sqrt(D)) / a with a = 2^-140, is FLT_MAX exactly -- outside the open interval -- and the float
    below it from twice as far off centre; the cube's entry (nextdown(2) - 0) / 2^-127 is FLT_MAX exactly -- inside the closed interval -- and +inf
    from half the direction.  Every operand is a power of two or one ulp from it: nothing rounds."""
    o, d = [], []
    for axis, sign in AXES:
        for z in (2.0 ** 34, 2.0 ** 35, 2.0 ** 33):
            oo = np.zeros(3, F); oo[axis] = sign * z
            dd = np.zeros(3, F); dd[axis] = sign * 2.0 ** -70
            o.append(oo); d.append(dd)
    for s in (2.0 ** -127, 2.0 ** -128, 2.0 ** -126):
        o.append(np.zeros(3, F)); d.append(np.array((s, 0, 0), F))
    return rays6(np.array(o, F), np.array(d, F))


def tie_rays(sc):
    """Rays along the axis through a tie scene's common point, from five distances with four direction lengths: every operand and every result of both
    primitives' tests is a small dyadic number, so both are at exactly the same float t"""
    cube = sc.cubes[0]
    axis = int(np.argmax(np.abs((cube["minBounds"] + cube["maxBounds"]))))
    sign = 1.0 if cube["maxBounds"][axis] > 0.75 else -1.0
    o, d = [], []
    for k in (2.0, 1.0, 0.5, 4.0, 8.0):
        for s in (1.0, 0.5, 2.0, 0.25):
            oo = np.zeros(3, F); oo[axis] = sign * (1.0 + k)
            dd = np.zeros(3, F); dd[axis] = -sign * s
            o.append(oo); d.append(dd)
    return rays6(np.array(o, F), np.array(d, F))


def mixed_rays(sc, seed=111):
    """Vertical rays from z = 3 over a grid of eighths (the quad and the cube's face, the tangent triangle and the sphere's pole: at t = 2.5 exactly),
    and ordinary ones"""
    g = np.arange(-3.0, 2.5 + 1e-9, 0.125)
    x, y = np.meshgrid(g, np.arange(-2.25, 2.25 + 1e-9, 0.125))
    o = np.stack([x.ravel(), y.ravel(), np.full(x.size, 3.0)], 1).astype(F)
    return np.concatenate([rays6(o, np.tile(np.array((0, 0, -1), F), (len(o), 1))), regular(sc, 1500, seed)])


SPHERE_FAMILIES = ("tangent_axis", "tangent_generic", "on_surface", "inside", "centre", "poles")
CUBE_FAMILIES = ("cube_axis", "cube_corner", "cube_inside", "cube_onface")


def families(S=None):
    """{family: (scene name, rays6)} -- the cube families on the static cube and, as "<family>_m", on the moving one (the same rays at ray time 0)"""
    S = S or scenes()
    out = {"tangent_axis": ("sphere1", tangent_axis()), "tangent_generic": ("sphere1", tangent_generic()), "on_surface": ("sphere1", on_surface()),
           "inside": ("sphere1", inside()), "centre": ("sphere1", centre()), "poles": ("sphere1", poles())}
    cube = {"cube_axis": cube_axis(MN1, MX1), "cube_corner": cube_corner(MN1, MX1), "cube_inside": cube_inside(MN1, MX1), "cube_onface": cube_onface(MN1, MX1)}
    for k, r in cube.items():
        out[k] = ("cube1", r)
        out[k + "_m"] = ("cube1m", r)
    out["special"] = ("many", special(S["many"]))
    out["regular_many"] = ("many", regular(S["many"], 4000))
    out["flt_max"] = ("huge", flt_max())
    for k, (_, r) in out.items():
        assert len(r) <= 60000 and r.dtype == F, k
    return out


def moved_cube_families(tau):
    """The four cube families built on cube1m's bounds at ray time tau (float32, CubeHit's own arithmetic): the planes' +- 2 ulp follow the cube"""
    sc = scenes()["cube1m"]
    b = sc.boxes(tau)[0]
    return {"cube_axis": cube_axis(b[:3], b[3:], 6000), "cube_corner": cube_corner(b[:3], b[3:]), "cube_inside": cube_inside(b[:3], b[3:], 1000),
            "cube_onface": cube_onface(b[:3], b[3:], 2000)}


def sha256(rays):
    return hashlib.sha256(np.ascontiguousarray(rays, F).tobytes()).hexdigest()


def subsample(n, k=SUBSAMPLE, seed=7):
    """The fixed rays of a family whose reference records the fixture stores"""
    return np.sort(np.random.RandomState(seed).permutation(n)[:k]) if n > k else np.arange(n)


def canonical(records):
    """Hit records with every NaN as 0x7fc00000 (a NaN's sign and payload are not part of parity: helpers.same) -- for byte comparisons and hashes"""
    r = np.array(records, copy=True)
    w = r.view(np.uint32).reshape(len(r), -1)
    f = r.view(F).reshape(len(r), -1)
    cols = [1, 2, 3, 4, 5, 6, 7, 8, 9]      # t, p, n, paramU, paramV of HIT_DTYPE (hit and material are integers)
    for c in cols:
        w[np.isnan(f[:, c]), c] = 0x7fc00000
    return r


def records_sha256(records):
    return hashlib.sha256(canonical(records).tobytes()).hexdigest()


def closest(checker, handle, r6, tmin):
    """checker.closest_hit with a cube's paramU / paramV as 0 (Cube::Hit leaves them unset: the reference's record holds whatever was there) and every
    NaN canonical"""
    rec = checker.closest_hit(handle, r6, tmin)
    cube = rec["material"] == MAT_CUBE
    rec["paramU"][cube] = 0.0; rec["paramV"][cube] = 0.0
    return canonical(rec)


def recorded(checker, ffi):
    """What tests/golden/analytic_edges.npz holds, from `checker` (the reference when the fixture is written, the oracle when it is checked):
    "<family>/rays" the SHA-256 of the family's ray bytes; "<family>/<k>/sub" the records of the family's fixed subsample at TMINS[k] and
    "<family>/<k>/all" the SHA-256 of the records of all its rays; "tau<j>/<family>/..." the same for the cube families built on the moving cube's
    bounds at ray time TAUS[j], asked at ray time 0 of the time-shifted scene (Scene.at), tMin 0."""
    S, out = scenes(), {}
    handles = {}

    def handle(sc):
        if sc.name not in handles:
            handles[sc.name] = checker.scene_create(flat_scene(sc, ffi), 1)
        return handles[sc.name]

    def put(key, sc, r6, tmins):
        out[key + "/rays"] = np.array(sha256(r6))
        sub = subsample(len(r6))
        for k, tmin in tmins:
            rec = closest(checker, handle(sc), r6, tmin)
            out["%s/%d/sub" % (key, k)] = rec[sub]
            out["%s/%d/all" % (key, k)] = np.array(hashlib.sha256(rec.tobytes()).hexdigest())

    for name, (sn, r6) in families(S).items():
        put(name, S[sn], r6, list(enumerate(TMINS)))
    for j, tau in enumerate(TAUS):
        for name, r6 in moved_cube_families(tau).items():
            put("tau%d/%s" % (j, name), S["cube1m"].at(tau), r6, [(1, TMINS[1])])
    for h in handles.values():
        checker.scene_destroy(h)
    return out


# ---- the excused set ---------------------------------------------------------------------------------------------------------------------
def box_hit(boxes, r8):
    """oracle.cc BoxHit (reference geom/aabb.h:39-54) in float32, with each ray's own [tMin, tMax]; boxes (6,) or (n, 6).  tests/test_analytic_host.py
    holds it to oracle.aabb_hit."""
    boxes = np.broadcast_to(np.asarray(boxes, F), (len(r8), 6))
    lo, hi = r8[:, 3].copy(), r8[:, 7].copy()
    ok = np.ones(len(r8), bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            inv = (F(1.0) / r8[:, 4 + a]).astype(F)
            t0 = ((boxes[:, a] - r8[:, a]).astype(F) * inv).astype(F)
            t1 = ((boxes[:, 3 + a] - r8[:, a]).astype(F) * inv).astype(F)
            sw = inv < 0
            t0, t1 = np.where(sw, t1, t0), np.where(sw, t0, t1)
            lo = np.where(t0 > lo, t0, lo); hi = np.where(t1 < hi, t1, hi)
            ok &= ~(hi < lo)
    return ok


BOX_WIDEN = F(1.00001)      # csrc/rl_dev_walk.h RL_BOX_WIDEN


def slab_hit(boxes, r8):
    """The box test of this library's walks (csrc/rl_dev_walk.h Slab) on each ray's own interval: entry and exit as in box_hit, a NaN keeps the old bound,
    the search's upper end is the float above tMax (rl_k_query.inl) clamped to FLT_MAX, and the box is missed only if exit * RL_BOX_WIDEN < entry."""
    boxes = np.broadcast_to(np.asarray(boxes, F), (len(r8), 6))
    with np.errstate(all="ignore"):
        lo = r8[:, 3].copy()
        hi = np.minimum(np.nextafter(r8[:, 7], F(np.inf)), FLT_MAX)
        hi = np.where(np.isnan(r8[:, 7]), r8[:, 7], hi)
        for a in range(3):
            inv = (F(1.0) / r8[:, 4 + a]).astype(F)
            t0 = ((boxes[:, a] - r8[:, a]).astype(F) * inv).astype(F)
            t1 = ((boxes[:, 3 + a] - r8[:, a]).astype(F) * inv).astype(F)
            sw = inv < 0
            t0, t1 = np.where(sw, t1, t0), np.where(sw, t0, t1)
            lo = np.where(t0 > lo, t0, lo); hi = np.where(t1 < hi, t1, hi)
        return ~((hi * BOX_WIDEN).astype(F) < lo)


class Excuser:
    """A ray is excused only if some primitive that the float test accepts in the ray's interval -- the oracle on a scene of that primitive alone -- fails the
    box test on its own box at the ray time: whether a tree walk ever reaches such a primitive depends on the tree.  Two box tests count.  The reference's
    (box_hit) over [tMin, FLT_MAX], as every box test of its closest-hit walk runs (t_max never shrinks there).  And, for a ray with a tMax of its own, the
    walks' own (slab_hit, with their slack) over the ray's interval: the float sphere test, whose discriminant cancels, reports roots up to 1e-4 of t away from
    the sphere -- outside its box -- and with tMax next to such a t the box begins beyond the interval.  (The reference's unwidened test over [tMin, tMax]
    fails there far more often -- a pole lies ON its box's face, the entry is the root's t up to an ulp -- and a walk that culled like that would be
    excused on 15 % of the pole rays; the condition here is the narrower one.)  A condition, not a tolerance."""

    def __init__(self, oracle, sc, make_flat):
        self.oracle, self.sc = oracle, sc
        self.handles = [oracle.scene_create(make_flat(s), 1) for s in sc.singles()]

    def __call__(self, r8, tau=0.0):
        r8 = np.ascontiguousarray(r8, F)
        ex = np.zeros(len(r8), bool)
        whole = r8.copy(); whole[:, 7] = FLT_MAX
        for h, box in zip(self.handles, self.sc.boxes(tau)):
            acc = np.isfinite(self.oracle.interval_hits(h, r8, float(tau))["t"])
            ex |= acc & ~(box_hit(box, whole) & slab_hit(box, r8))
        return ex

    def close(self):
        for h in self.handles:
            self.oracle.scene_destroy(h)


def flat_scene(sc, ffi, triangles=None):
    """The oracle's flat scene of `sc` (triangles: the device's export, oracle.ffi.TRI_DTYPE rows, for a scene that has any)"""
    assert SPHERE_DTYPE == ffi.SPHERE_DTYPE and CUBE_DTYPE == ffi.CUBE_DTYPE
    tris = np.zeros(0, ffi.TRI_DTYPE) if triangles is None else triangles
    return ffi.FlatScene(tris, material_array(ffi.MAT_DTYPE), spheres=sc.spheres, cubes=sc.cubes, num_shapes=0 if not len(tris) else None)


def interval_sets(r6, tmin, t):
    """The re-runs of a family's hitting rays (t: the oracle's t per ray, +inf on a miss): tMax at t, at the float above and at the float below, and tMin
    at t -- a sphere's interval is open at both ends, a cube's closed.  [(label, rays8)]"""
    hit = np.isfinite(t)
    r, t = r6[hit], np.asarray(t, F)[hit]
    with np.errstate(over="ignore"):
        up, down = np.nextafter(t, F(np.inf)), np.nextafter(t, F(-np.inf))
    return [("tMax = t", rays8(r, tmin, t)), ("tMax = nextup(t)", rays8(r, tmin, up)), ("tMax = nextdown(t)", rays8(r, tmin, down)), ("tMin = t", rays8(r, t, FLT_MAX))]


def layouts(fams, reg, seed=112):
    """Wave layouts of one scene's families (fams: {name: rays6}, reg: its ordinary rays), after tests/test_gpu_scatter_edges.py: [(label, rays6, src)] with
    src the row of `reg` a ray is, -1 for a family's ray.  Each family alone; one degenerate ray (the family's fixed subsample) among 63 ordinary ones at
    lane 0, 31 and 63; everything shuffled; the shuffled set cut to 1, 63, 64 and 65 rays."""
    rng = np.random.RandomState(seed)
    out = [("alone:" + k, r, np.full(len(r), -1)) for k, r in fams.items()]
    waves, src = [], []
    for k, r in fams.items():
        for j, i in enumerate(subsample(len(r))):
            pick = rng.randint(0, len(reg), 64)
            w = reg[pick].copy()
            lane = (0, 31, 63)[j % 3]
            w[lane] = r[i]; pick[lane] = -1
            waves.append(w); src.append(pick)
    out.append(("one_in_a_wave", np.ascontiguousarray(np.concatenate(waves), F), np.concatenate(src)))
    every = np.concatenate([r[subsample(len(r), 2048, 8)] for r in fams.values()] + [reg])
    m = np.full(len(every), -1); m[len(every) - len(reg):] = np.arange(len(reg))
    p = rng.permutation(len(every))
    out.append(("shuffled", np.ascontiguousarray(every[p], F), m[p]))
    for n in (1, 63, 64, 65):
        out.append(("shuffled[:%d]" % n, np.ascontiguousarray(every[p][:n], F), m[p][:n]))
    return out
