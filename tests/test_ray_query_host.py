"""Batched ray queries (RaylibAMD_TraceRays, include/raylib_amd.h) without a device: the record layouts, the planner's choice of tree
(csrc/rl_plan.cc PlanQuery) with the RAYLIB_QUERY_TREE switch and its fall-backs, and the refusals.  tests/test_gpu_ray_query.py checks the results.

Below them, the tree-free interval oracle the device's [tMin, tMax] answers are held to (oracle_interval_hits, tests/test_gpu_ray_query_intervals.py): against
the oracle's own tree walk, on known answers at the interval's edges, by peeling a ray's surfaces one after another, and the finding that made the query
raise a negative tMin to zero."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from helpers import scenes, ffi, bits

TREE_BVH2, TREE_GRID4, TREE_WIDE8 = 1, 3, 4
POOL8_MAXLEVELS = 16


def _write_soup(path, n_soup, n_chain):
    """As tests/test_render_plan_host.py: n_soup triangles of about the scene's size, then a chain of n_chain ever smaller triangles (a deep BVH2)."""
    rng = np.random.RandomState(3)
    lines, k = ["o soup\n"], 0
    tris = [c + rng.uniform(-1.0, 1.0, (3, 3)) for c in rng.uniform(-1.0, 1.0, (n_soup, 3))]
    for j in range(1, n_chain + 1):
        c = 2.0 ** -j
        tris.append(np.array([[c, 0, 0], [c + c / 2, 0, 0], [c, c / 2, 0]]))
    for p in tris:
        for q in p:
            lines.append("v %.9g %.9g %.9g\n" % tuple(q))
        lines.append("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))
        k += 1
    with open(path, "w") as f:
        f.write("".join(lines))
    return path


@pytest.fixture(scope="module")
def query_scenes(lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "ray_query_host"); os.makedirs(d, exist_ok=True)

    def obj(path):
        return binding.SceneSession(lib, path, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    S = {"cornell": obj(scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
         "soup": obj(_write_soup(os.path.join(d, "soup.obj"), 1000, 0)),
         "deep": obj(_write_soup(os.path.join(d, "deep.obj"), 1000, 72))}
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    S["spheres"] = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)],
                                             [dict(minBounds=(1, 0, 0), maxBounds=(1.5, 0.5, 0.5), timeStartMove=0.0, velocity=(0.0, 0.5, 0.0), material=0)])
    yield S
    for s in S.values():
        s.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _bvh(lib, ses):
    n, d, s = C.c_uint32(), C.c_uint32(), C.c_float()
    lib.RaylibAMD_SceneBVHInfo(ses.scene, C.byref(n), C.byref(d), C.byref(s))
    n4, st4 = C.c_uint32(), C.c_uint32()
    has4 = lib.RaylibAMD_SceneBVH4Info(ses.scene, C.byref(n4), C.byref(st4)) != 0
    n8, lv, s4, s8 = C.c_uint32(0), C.c_uint32(0), C.c_float(0), C.c_float(0)
    has8 = lib.RaylibAMD_SceneBVH8Info(ses.scene, C.byref(n8), C.byref(lv), C.byref(s4), C.byref(s8)) != 0
    return dict(depth=d.value, has4=has4, stack4=st4.value, has8=has8, levels8=lv.value)


def _plan(lib, ses, kind=1):
    from raylib_amd import binding
    rc, p = binding.plan_ray_query(lib, ses.scene, kind)
    assert rc == 1, rc
    return p


def test_record_layouts(lib):
    from raylib_amd import binding
    assert C.sizeof(binding.Ray) == 32 and C.sizeof(binding.HitT) == 16
    assert [getattr(binding.Ray, f).offset for f in ("org", "tMin", "dir", "tMax")] == [0, 12, 16, 28]
    assert [getattr(binding.HitT, f).offset for f in ("t", "prim", "b1", "b2")] == [0, 4, 8, 12]
    assert binding.HITT_DTYPE.itemsize == 16 and binding.SURFACE_DTYPE == ffi.HIT_DTYPE and binding.SURFACE_DTYPE.itemsize == 44
    assert (binding.QUERY_ANY, binding.QUERY_CLOSEST, binding.QUERY_SURFACE) == (0, 1, 2)
    assert (binding.PRIM_SPHERE, binding.PRIM_CUBE) == (0x10000000, 0x20000000)
    for name in ("RaylibAMD_TraceRays", "RaylibAMD_TraceRaysDevice", "RaylibAMD_PlanRayQuery"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


def test_plan_default_trees(lib, query_scenes):
    S = query_scenes
    # the soup carries an 8-wide tree of few levels: walked by every kind
    b = _bvh(lib, S["soup"])
    assert b["has8"] and b["levels8"] <= POOL8_MAXLEVELS, b
    for kind in (0, 1, 2):
        p = _plan(lib, S["soup"], kind)
        assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"], p["prims"]) == (TREE_WIDE8, 8, 80, 2 * POOL8_MAXLEVELS, 0), p
        assert p["early"] == (kind == 0)
    # Cornell has no 8-wide tree (the builder makes one only where rays are expected to take many steps): the grid-4 tree
    b = _bvh(lib, S["cornell"])
    assert not b["has8"] and b["has4"] and b["stack4"] <= 32, b
    for kind in (0, 1, 2):
        p = _plan(lib, S["cornell"], kind)
        assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"], p["prims"], p["early"]) == (TREE_GRID4, 4, 64, 32, 0, int(kind == 0)), p
    # spheres and cubes: the binary tree, and the occlusion query walks to the closest hit (a sphere's interval is open at tMax)
    for kind in (0, 1, 2):
        p = _plan(lib, S["spheres"], kind)
        assert (p["tree"], p["treeWidth"], p["stack"], p["prims"], p["early"]) == (TREE_BVH2, 2, 32, 1, 0), p


def test_plan_forced_trees_and_fallbacks(lib, query_scenes, monkeypatch):
    S = query_scenes
    b = _bvh(lib, S["soup"])
    assert b["has4"] and b["stack4"] <= 64 and b["depth"] <= 32, b
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "4")
    p = _plan(lib, S["soup"])
    assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"]) == (TREE_GRID4, 4, 64, 32 if b["stack4"] <= 32 else 64), p
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "2")
    p = _plan(lib, S["soup"])
    assert (p["tree"], p["treeWidth"], p["stack"]) == (TREE_BVH2, 2, 32), p
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "8")
    assert _plan(lib, S["soup"])["tree"] == TREE_WIDE8
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "5")          # not a tree: the default
    assert _plan(lib, S["soup"])["tree"] == TREE_WIDE8
    # the deep chain: BVH2 deeper than 32 and a 4-wide stack need above 64, but an 8-wide tree of few levels
    b = _bvh(lib, S["deep"])
    assert b["depth"] > 32 and b["stack4"] > 64 and b["levels8"] <= POOL8_MAXLEVELS, b
    monkeypatch.delenv("RAYLIB_QUERY_TREE")
    assert _plan(lib, S["deep"])["tree"] == TREE_WIDE8
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "4")          # no grid tree it could walk: the binary tree, 64 deep
    p = _plan(lib, S["deep"])
    assert (p["tree"], p["treeWidth"], p["stack"]) == (TREE_BVH2, 2, 64), p
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "2")
    assert (_plan(lib, S["deep"])["tree"], _plan(lib, S["deep"])["stack"]) == (TREE_BVH2, 64)
    # Cornell: 8 asked for, no 8-wide tree -- the grid; 2 -- the binary tree
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "8")
    assert _plan(lib, S["cornell"])["tree"] == TREE_GRID4
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "2")
    assert (_plan(lib, S["cornell"])["tree"], _plan(lib, S["cornell"])["stack"]) == (TREE_BVH2, 32)
    # spheres: whatever is asked for, the binary tree
    for v in ("8", "4", "2"):
        monkeypatch.setenv("RAYLIB_QUERY_TREE", v)
        assert _plan(lib, S["spheres"])["tree"] == TREE_BVH2


def test_plan_refusals(lib, query_scenes):
    from raylib_amd import binding
    S = query_scenes
    p = binding.QueryPlan()
    assert lib.RaylibAMD_PlanRayQuery(S["cornell"].scene, 3, C.byref(p)) == 0
    assert lib.RaylibAMD_PlanRayQuery(S["cornell"].scene, -1, C.byref(p)) == 0
    assert lib.RaylibAMD_PlanRayQuery(S["cornell"].scene, 1, None) == 0
    assert lib.RaylibAMD_PlanRayQuery(None, 1, C.byref(p)) == 0
    unfinished = lib.Raylib_CreateScene()
    assert lib.RaylibAMD_PlanRayQuery(unfinished, 1, C.byref(p)) == 0
    lib.Raylib_DestroyScene(unfinished)


def _rays(n):
    r = np.zeros((n, 8), np.float32)
    r[:, 1] = 1.0; r[:, 2] = 4.0; r[:, 6] = -1.0; r[:, 3] = 1e-4; r[:, 7] = 3.4028235e38
    return r


def test_trace_refuses_bad_arguments_before_the_device(lib, query_scenes):
    """Null pointers with n > 0, a negative n, an unknown kind, a ray time that is not finite and an unfinished scene are refused whether or not there is a device, and nothing is written."""
    from raylib_amd import binding
    ses = query_scenes["cornell"]
    rays = _rays(4)
    rp = rays.ctypes.data_as(C.POINTER(binding.Ray))
    out = np.full(4 * 16, 0x5a, np.uint8)
    for fn, extra in ((lib.RaylibAMD_TraceRays, ()), (lib.RaylibAMD_TraceRaysDevice, (None,))):
        assert fn(ses.scene, 1, None, 4, 0.0, out.ctypes.data, None, *extra) == 0
        assert fn(ses.scene, 1, rp, 4, 0.0, None, None, *extra) == 0
        assert fn(ses.scene, 1, rp, -1, 0.0, out.ctypes.data, None, *extra) == 0
        assert fn(ses.scene, 3, rp, 4, 0.0, out.ctypes.data, None, *extra) == 0
        for t in (float("nan"), float("inf"), float("-inf")):           # a ray time that is not finite
            assert fn(query_scenes["spheres"].scene, 1, rp, 4, t, out.ctypes.data, None, *extra) == 0
            assert fn(ses.scene, 1, rp, 4, t, out.ctypes.data, None, *extra) == 0
        assert fn(None, 1, rp, 4, 0.0, out.ctypes.data, None, *extra) == 0
        unfinished = lib.Raylib_CreateScene()
        assert fn(unfinished, 1, rp, 4, 0.0, out.ctypes.data, None, *extra) == 0
        lib.Raylib_DestroyScene(unfinished)
    assert (out == 0x5a).all()
    with pytest.raises(ValueError):
        binding.trace_rays(lib, ses.scene, rays, 7)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-device path: this machine may have a GPU")
def test_trace_without_a_device_returns_0(lib, query_scenes):
    from raylib_amd import binding
    ses = query_scenes["cornell"]
    rays = _rays(4)
    out = np.full(4, 7, np.uint32)
    for kind in (0, 1, 2):
        assert lib.RaylibAMD_TraceRays(ses.scene, kind, rays.ctypes.data_as(C.POINTER(binding.Ray)), 4, 0.0, out.ctypes.data, None) == 0
        assert lib.RaylibAMD_TraceRaysDevice(ses.scene, kind, rays.ctypes.data_as(C.POINTER(binding.Ray)), 4, 0.0, out.ctypes.data, None, None) == 0
    assert (out == 7).all()
    with pytest.raises(RuntimeError):
        binding.trace_rays(lib, ses.scene, rays, binding.QUERY_CLOSEST)


# ---- the interval oracle (oracle/oracle.cc oracle_interval_hits) ---------------------------------------------------------------------------
FLT_MAX = helpers.F32_MAX
ORACLE_THREADS = 16


def _inside_rays(rng, n, lo, hi, axis_third=False):
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    if axis_third:   # every third ray along an axis
        k = len(d[::3])
        d[::3] = np.eye(3, dtype=np.float32)[rng.randint(0, 3, k)] * rng.choice([-1, 1], (k, 1)).astype(np.float32)
    return helpers.rays8(o, d)


def _r6(rays):
    return np.ascontiguousarray(np.concatenate([rays[:, 0:3], rays[:, 4:7]], axis=1), np.float32)


@pytest.fixture(scope="module")
def interval_scenes(oracle, workdir):
    """name -> (oracle scene, flat scene, rays): soup, the displaced room, the cut-out scene with its textures, spheres and cubes"""
    d = os.path.join(str(workdir), "interval_host"); os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(1)
    S = {}
    flat = helpers.objflat.load_obj(scenes.soup(os.path.join(d, "soup.obj"), n_tris=1500)[0], oracle)
    S["soup"] = (flat, _inside_rays(rng, 1500, -4.0, 4.0))
    flat = helpers.objflat.load_obj(scenes.cornell(os.path.join(d, "room.obj"), tess=6, displace_fraction=0.2)[0], oracle)
    S["room"] = (flat, _inside_rays(rng, 1500, (-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), axis_third=True))
    _, _, flat = helpers.flat_for_case("cutout_sky", os.path.join(d, "cut"), oracle)
    assert len(flat.textures) >= 2 and (flat.materials["texAlbedo"] >= 0).any()
    S["cutout"] = (flat, _inside_rays(rng, 1500, (-0.9, 0.1, -0.9), (0.9, 1.9, 3.0)))
    flat, _ = helpers.procedural_flat()
    o = np.zeros((1500, 3), np.float32); o[:, 1] = 0.5; o[:, 2] = 3.0
    tgt = rng.uniform((-2.0, -0.6, -1.5), (2.0, 3.0, 0.8), (1500, 3)).astype(np.float32)
    S["procedural"] = (flat, helpers.rays8(o, tgt - o))
    out = {k: (oracle.scene_create(f, 1), f, r) for k, (f, r) in S.items()}
    yield out
    for sc, _, _ in out.values():
        oracle.scene_destroy(sc)


@pytest.mark.parametrize("name", ["soup", "room", "cutout", "procedural"])
def test_brute_force_equals_the_oracles_tree_walk(oracle, interval_scenes, name):
    """Over [tMin, FLT_MAX] the least t of the loop over every primitive is the t of closest_hit's tree walk, in bits; a ray may differ only where its own
    closest_hit reports a tie or a hit outside the triangle's own box, or where the record says the candidate rule rejected something nearer."""
    sc, flat, rays = interval_scenes[name]
    for tmin in (0.0, 1e-4, 0.7, 2.5):
        r = helpers.with_interval(rays, tmin, FLT_MAX)
        got = oracle.interval_hits(sc, r, 0.0, ORACLE_THREADS)
        r6 = _r6(r)
        tree = oracle.closest_hit(sc, r6, tmin)
        tt = np.where(tree["hit"] == 1, tree["t"], np.float32(np.inf)).astype(np.float32)
        differ = np.nonzero(bits(tt) != bits(got["t"]))[0]
        excused = 0
        for i in differ:
            oracle.closest_hit(sc, r6[i:i + 1], tmin)
            cn = oracle.counters(sc)
            assert cn["closest_hit_ties"] > 0 or cn["hits_outside_own_box"] > 0 or got["nearerRejected"][i] > 0, (name, tmin, int(i), r[i].tolist(), tt[i], got[i])
            excused += 1
        hits = np.isfinite(got["t"])
        assert hits.sum() > len(rays) // 20 or tmin > 1e-4, (name, tmin, hits.sum())   # (the room is 2 wide: little lies beyond 2.5)
        assert (got["count"][hits] >= 1).all() and (got["count"][~hits] == 0).all() and (got["prims"][~hits] == -1).all()
        first = got["prims"][hits, 0]
        if len(flat.triangles):
            assert ((first >= 0) & (first < len(flat.triangles))).all()
        else:
            kinds = set(np.unique(first & ~0x0fffffff))
            assert kinds <= {ffi.PRIM_SPHERE, ffi.PRIM_CUBE} and (tmin > 0.7 or kinds == {ffi.PRIM_SPHERE, ffi.PRIM_CUBE}), kinds
        print("%s tMin %g: %d rays, %d hits, %d differ from the tree walk (each excused), %d ties, nearerRejected on %d" % (
            name, tmin, len(rays), hits.sum(), excused, (got["count"] > 1).sum(), (got["nearerRejected"] > 0).sum()))


def _edge_scene(oracle):
    """A triangle at z = -2 in front of (0,0,0), a sphere of radius 1 at (5,0,-3) in front of (5,0,0) (roots 2 and 4), a static cube whose near face is at
    z = -2 in front of (-5,0,0), and a cube moving by -1 in z per unit of time in front of (-10,0,0) (t = 2 + rayTime): every t is exact."""
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = ffi.MAT_LAMBERTIAN; mats["albedo"] = (0.5, 0.5, 0.5)
    for k in ("texAlbedo", "texNormal", "texRoughness", "texMetallic", "texEmissive"):
        mats[k] = -1
    tri = np.zeros(1, ffi.TRI_DTYPE)
    tri["v0"] = (-1, -1, -2); tri["v1"] = (1, -1, -2); tri["v2"] = (0, 1, -2)
    tri["n0"] = tri["n1"] = tri["n2"] = (0, 0, 1)
    sph = np.zeros(1, ffi.SPHERE_DTYPE); sph[0] = ((5, 0, -3), 1.0, 0)
    cub = np.zeros(2, ffi.CUBE_DTYPE)
    cub[0] = ((-5.5, -0.5, -3), (-4.5, 0.5, -2), 0.0, (0, 0, 0), 0)
    cub[1] = ((-10.5, -0.5, -3), (-9.5, 0.5, -2), 0.0, (0, 0, -1), 0)
    flat = ffi.FlatScene(tri, mats, spheres=sph, cubes=cub, num_shapes=1)
    return oracle.scene_create(flat, 1), flat


def test_interval_edges_known_answers(oracle):
    sc, flat = _edge_scene(oracle)
    inf = np.float32(np.inf)
    two, four = np.float32(2.0), np.float32(4.0)
    TRI, SPH, CUBE, MOVING = 0, ffi.PRIM_SPHERE, ffi.PRIM_CUBE, ffi.PRIM_CUBE | 1
    org = {TRI: (0, 0, 0), SPH: (5, 0, 0), CUBE: (-5, 0, 0), MOVING: (-10, 0, 0)}

    def ask(prim, tmin, tmax, ray_time=0.0):
        got = oracle.interval_hits(sc, helpers.rays8([org[prim]], [(0, 0, -1)], tmin, tmax), ray_time, 1)[0]
        assert got["nearerRejected"] == 0
        if np.isfinite(got["t"]):
            assert got["count"] == 1 and got["prims"][0] == prim and (got["prims"][1:] == -1).all(), got
        else:
            assert got["count"] == 0 and (got["prims"] == -1).all(), got
        return got["t"]

    up, down = helpers.nextup(two), helpers.nextdown(two)
    for prim, closed in ((TRI, True), (CUBE, True), (SPH, False)):
        assert ask(prim, 0.0, FLT_MAX) == two and ask(prim, 0.0, inf) == two
        assert ask(prim, 0.0, up) == two                               # tMax an ulp behind the hit
        assert ask(prim, 0.0, down) == inf                             # an ulp in front: nothing, the sphere's far root lies beyond too
        assert ask(prim, 0.0, two) == (two if closed else inf)         # exactly at the hit: closed for triangle and cube, open for the sphere
        assert ask(prim, down, FLT_MAX) == two
        behind = four if prim == SPH else inf                          # what remains once the hit is excluded: the sphere's far root
        assert ask(prim, two, FLT_MAX) == (two if closed else behind)  # tMin exactly at the hit
        assert ask(prim, up, FLT_MAX) == behind
        assert ask(prim, two, two) == (two if closed else inf)         # the point interval
    # the sphere's far root while the near one lies below tMin; it is open at both ends as well
    assert ask(SPH, 3.0, FLT_MAX) == four and ask(SPH, 3.0, helpers.nextup(four)) == four and ask(SPH, 3.0, four) == inf
    assert ask(SPH, four, FLT_MAX) == inf and ask(SPH, helpers.nextdown(four), FLT_MAX) == four
    # the moving cube: its near face at 2 + rayTime; the static one stays
    for rt in (0.0, 0.5, 1.0):
        t = np.float32(2.0 + rt)
        assert ask(MOVING, 0.0, FLT_MAX, rt) == t and ask(MOVING, t, t, rt) == t
        assert ask(MOVING, 0.0, helpers.nextdown(t), rt) == inf and ask(MOVING, helpers.nextup(t), FLT_MAX, rt) == inf
        assert ask(CUBE, 0.0, FLT_MAX, rt) == two
    # a NaN bound gives a miss, whatever the primitive
    nan = np.float32(np.nan)
    for prim in (TRI, SPH, CUBE):
        assert ask(prim, nan, FLT_MAX) == inf and ask(prim, 0.0, nan) == inf and ask(prim, nan, nan) == inf
    oracle.scene_destroy(sc)


def _candidate_rule_numpy(T, r6, tmin, t):
    """The ray queries' candidate rule restated in float32 numpy (oracle.cc CandidateRule with the widened exit), for n rays against one triangle each"""
    with np.errstate(all="ignore"):
        mn = np.minimum(np.minimum(T["v0"], T["v1"]), T["v2"]); mx = np.maximum(np.maximum(T["v0"], T["v1"]), T["v2"])
        o = r6[:, 0:3]; inv = (np.float32(1) / r6[:, 3:6]).astype(np.float32)
        lo = np.full(len(r6), -np.inf, np.float32); hi = np.full(len(r6), FLT_MAX, np.float32)
        ok = np.ones(len(r6), bool)
        for a in range(3):
            t0 = ((mn[:, a] - o[:, a]) * inv[:, a]).astype(np.float32); t1 = ((mx[:, a] - o[:, a]) * inv[:, a]).astype(np.float32)
            neg = inv[:, a] < 0
            t0, t1 = np.where(neg, t1, t0), np.where(neg, t0, t1)
            lo = np.where(t0 > lo, t0, lo); hi = np.where(t1 < hi, t1, hi)
            ok &= ~(hi < lo)
        ok &= ~((hi * np.float32(1.00001)).astype(np.float32) < np.float32(tmin))
        lo = np.where(np.float32(tmin) > lo, np.float32(tmin), lo)
        return ok & ((t * np.float32(1.000009)).astype(np.float32) >= lo)


@pytest.mark.parametrize("name", ["soup", "room"])
def test_peeling_gives_every_surface_once_in_order(oracle, interval_scenes, name):
    """tMin = nextafter(t_prev, +inf) again and again: strictly increasing t, each the t of a candidate the ray has over [0, FLT_MAX], ending in a miss after
    at most as many layers as the ray has such candidates."""
    sc, flat, rays = interval_scenes[name]
    rays = rays[:300]
    r6 = _r6(rays)
    cand = [set() for _ in rays]
    ncand = np.zeros(len(rays), np.int64)
    for k in range(len(flat.triangles)):   # every triangle alone, with the rule restated here
        T = np.repeat(flat.triangles[k:k + 1], len(rays))
        h = oracle.triangle_hit(T, r6, 0.0, float(FLT_MAX))
        m = (h["hit"] == 1) & _candidate_rule_numpy(T, r6, 0.0, h["t"])
        ncand += m
        for i in np.nonzero(m)[0]:
            cand[i].add(int(bits(h["t"][i:i + 1])[0]))
    layers = 64
    T = helpers.peel(oracle, sc, rays, layers, 0.0)
    assert not np.isfinite(T[-1]).any(), "a ray with more than %d surfaces" % (layers - 1)
    depth = np.isfinite(T).sum(0)
    for i in range(len(rays)):
        t = T[:depth[i], i]
        assert not np.isfinite(T[depth[i]:, i]).any()
        assert (np.diff(t) > 0).all(), (i, t)
        assert depth[i] <= ncand[i], (i, depth[i], ncand[i])
        assert [int(b) for b in bits(t)] == sorted(cand[i], key=lambda b: np.array([b], np.uint32).view(np.float32)[0]), (i, t)
    assert depth.max() >= 3 and (depth >= 2).mean() >= 0.05, (depth.max(), (depth >= 2).mean())   # (the rays must have something to peel)
    print("%s: %d rays, up to %d layers, %d candidates in all" % (name, len(rays), depth.max(), ncand.sum()))


def test_negative_tmin_the_candidate_rule_rejects_what_the_reference_accepts(oracle, interval_scenes):
    """Why a query raises tMin < 0 to 0 (include/raylib_amd.h): from inside the room with tMin = -10 the reference's closest hit lies behind the
    origin for most rays, and the candidate rule -- t * slack >= the entry into the triangle's own box, a slack that assumes t >= 0 -- rejects most of those,
    so the brute-force answer with the raw negative tMin is not the reference's.  The oracle restates the device's rule; it is not the thing to change."""
    sc, flat, rays = interval_scenes["room"]
    r = helpers.with_interval(rays, -10.0, FLT_MAX)
    tree = oracle.closest_hit(sc, _r6(r), -10.0)
    got = oracle.interval_hits(sc, r, 0.0, ORACLE_THREADS)
    negative = (tree["hit"] == 1) & (tree["t"] < 0)
    assert negative.sum() > len(rays) // 2, negative.sum()
    differ = negative & (bits(tree["t"]) != bits(got["t"]))
    assert differ.sum() > negative.sum() // 2, (differ.sum(), negative.sum())
    assert (got["nearerRejected"][differ] > 0).all()
    # with tMin raised to zero, as the query does, nothing is rejected and the brute force is the tree walk again (test above, tMin 0)
    zero = oracle.interval_hits(sc, helpers.with_interval(rays, 0.0, FLT_MAX), 0.0, ORACLE_THREADS)
    assert (zero["nearerRejected"] == 0).all() and (zero["t"][np.isfinite(zero["t"])] >= 0).all()
    print("room, tMin -10: closest hit negative for %d of %d rays; the candidate rule rejects it for %d" % (negative.sum(), len(rays), differ.sum()))
