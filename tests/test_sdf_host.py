"""Signed distance fields (RaylibAMD_BakeDistanceField, include/raylib_amd.h statements V1 to V7) without a device: the host oracle
RaylibAMD_BakeDistanceFieldHost pinned from two independent sides, both exact -- its magnitudes and triangle indices against RaylibAMD_NearestPointsHost on
NumPy-computed centres, its signs against RaylibAMD_TraceRaysAllHost's crossings on NumPy-computed row rays -- then against geometry (the sphere's
half-spaces in float64), on the doubled mesh, at centres placed exactly on a cube's faces, and at every refusal.  tests/test_gpu_sdf.py holds the device to
the oracle byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers  # noqa: F401
from helpers import ffi
import nearest_cases as nc
import sdf_cases as sc
from raylib_amd import binding

POISON = 0x5a5a5a5a
DIMS = (13, 11, 10)
INF = float("inf")


@pytest.fixture(scope="module")
def S(lib, workdir):
    out = sc.make_sessions(lib, os.path.join(str(workdir), "sdf_host"))
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _oracle(lib, ses, origin, spacing, dims, max_dist, sign, prim=True):
    return sc.bake(lib, ses, origin, spacing, dims, max_dist, sign, prim=prim, host=True)


def test_exports_and_layout(lib):
    for name in ("RaylibAMD_BakeDistanceField", "RaylibAMD_BakeDistanceFieldDevice", "RaylibAMD_BakeDistanceFieldHost", "RaylibAMD_PlanDistanceField"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)
    assert C.sizeof(binding.DistanceFieldParams) == 44


@pytest.mark.parametrize("name", sc.MESHES)
@pytest.mark.parametrize("max_dist", [INF, 0.45, 0.0])
def test_distance_side_is_nearest_points(lib, S, name, max_dist):
    """V1, V2: abs(outDist) and outPrim are sqrt(dist2) and prim of CLOSEST on the NumPy centres, byte for byte; maxDist where nothing is in range."""
    ses = S[name]
    origin, spacing = sc.grid_around(DIMS, shift=sc.IRRATIONAL)
    pts = np.concatenate([sc.centres(origin, spacing, DIMS).reshape(-1, 3), np.full((int(np.prod(DIMS)), 1), max_dist, np.float32)], 1).astype(np.float32)
    near = binding.nearest_points(lib, ses.scene, pts, nc.CLOSEST, host=True)
    hit = near["prim"] >= 0
    want = np.where(hit, np.sqrt(near["dist2"]), np.float32(max_dist)).astype(np.float32)
    if max_dist == 0.45:
        assert 0.1 < (~hit).mean() < 0.9, "the band must cut"
    for sign in sc.SIGNS:
        dist, prim = _oracle(lib, ses, origin, spacing, DIMS, max_dist, sign)
        assert dist.shape == (DIMS[2], DIMS[1], DIMS[0]) and dist.dtype == np.float32
        assert np.abs(dist).reshape(-1).tobytes() == want.tobytes(), (name, max_dist, sign)
        assert prim.reshape(-1).tobytes() == near["prim"].tobytes(), (name, max_dist, sign)
        assert _oracle(lib, ses, origin, spacing, DIMS, max_dist, sign, prim=False).tobytes() == dist.tobytes(), "outPrim null changes no distance"
        if sign == sc.UNSIGNED:
            assert not np.signbit(dist).any()


@pytest.mark.parametrize("name", sc.MESHES)
def test_sign_side_is_the_crossing_parity(lib, S, name):
    """V3 to V5: the sign bit of outDist is the parity of RaylibAMD_TraceRaysAllHost's crossings ahead of each centre, per axis and for the majority."""
    ses = S[name]
    origin, spacing = sc.grid_around(DIMS, shift=sc.IRRATIONAL)
    inside = sc.oracle_inside(lib, ses, origin, spacing, DIMS)
    if name != "doubled":
        assert all(v.any() and not v.all() for v in inside), "every axis sees an inside and an outside"
    for sign in sc.SIGNS:
        dist = _oracle(lib, ses, origin, spacing, DIMS, INF, sign, prim=False)
        assert np.array_equal(np.signbit(dist), sc.inside_of_mode(inside, sign)), (name, sign)


def test_doubled_mesh_has_no_negative_voxel(lib, S):
    origin, spacing = sc.grid_around(DIMS, shift=sc.IRRATIONAL)
    single = _oracle(lib, S["sphere"], origin, spacing, DIMS, INF, sc.MAJORITY, prim=False)
    assert np.signbit(single).any()
    for sign in sc.SIGNS:
        dist = _oracle(lib, S["doubled"], origin, spacing, DIMS, INF, sign, prim=False)
        assert not np.signbit(dist).any(), "every crossing comes twice: the parity is even everywhere"
        assert np.abs(single).tobytes() == dist.tobytes(), "the magnitudes are the sphere's"


def _sphere_truth(origin, spacing, dims):
    """float64: for the sphere mesh's faces, whether each centre lies inside every face's half-space, and its distance to the surface."""
    verts, faces = sc.sphere_mesh()
    verts = verts.astype(np.float32).astype(np.float64)     # the vertices as the OBJ holds them
    tri = verts[np.asarray(faces)]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n *= np.sign((n * tri[:, 0]).sum(1))[:, None]            # outward, whatever the winding (the sphere is centred at the origin)
    P = sc.centres(origin, spacing, dims).reshape(-1, 3).astype(np.float64)
    inside = ((P[:, None, :] - tri[None, :, 0, :]) * n[None]).sum(2).max(1) < 0
    rec = np.zeros(len(tri), [("v0", "f8", 3), ("v1", "f8", 3), ("v2", "f8", 3)])
    rec["v0"], rec["v1"], rec["v2"] = tri[:, 0], tri[:, 1], tri[:, 2]
    dist = np.concatenate([nc.brute64(P[a:a + 1024], rec) for a in range(0, len(P), 1024)])
    return inside, dist


def test_sphere_sign_is_the_polyhedron(lib, S):
    """24 x 24 x 24 centres offset by an irrational fraction of a voxel: away from the surface (more than 1e-4 of the radius, in float64) the oracle's sign is the
    half-space test against the polyhedron's faces, and at most 2 % of the voxels are that near."""
    dims = (24, 24, 24)
    origin, spacing = sc.grid_around(dims, lo=-1.3, hi=1.3, shift=sc.IRRATIONAL)
    inside, d64 = _sphere_truth(origin, spacing, dims)
    far = d64 > 1e-4 * sc.SPHERE_RADIUS
    assert (~far).mean() <= 0.02, "too many centres on the surface: %g" % (~far).mean()
    assert 0.1 < inside.mean() < 0.5
    for sign in (sc.SIGN_X, sc.SIGN_Y, sc.SIGN_Z, sc.MAJORITY):
        dist = _oracle(lib, S["sphere"], origin, spacing, dims, INF, sign, prim=False).reshape(-1)
        bad = np.nonzero((np.signbit(dist) != inside) & far)[0]
        assert len(bad) == 0, (sign, len(bad), bad[:8], d64[bad[:8]])
        assert np.allclose(np.abs(dist)[far], d64[far], rtol=1e-4, atol=1e-6), "the magnitudes are the distances to the polyhedron"


def test_cube_centres_exactly_on_faces(lib, S):
    """The cube [-1, 1]^3 on a grid whose centres are the multiples of 0.5 from -2 to 2, exactly: a crossing at a centre is not ahead of it (V4), and m == 0
    is +0.0 outside and -0.0 inside (V5).  Voxels with |y| != |z| inside the face are taken: a row through a face's diagonal is a grazing row."""
    dims = (9, 9, 9)
    origin, spacing = np.full(3, -2.25, np.float32), np.full(3, 0.5, np.float32)
    c = sc.axis_centres(origin[0], spacing[0], 9)
    assert c.tolist() == [-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0]
    ses = S["cube"]
    inside = sc.oracle_inside(lib, ses, origin, spacing, dims)
    for sign in sc.SIGNS:
        dist = _oracle(lib, ses, origin, spacing, dims, INF, sign, prim=False)
        assert np.array_equal(np.signbit(dist), sc.inside_of_mode(inside, sign)), sign
    dx = _oracle(lib, ses, origin, spacing, dims, INF, sc.SIGN_X, prim=False)
    k, j = 4, 3            # z = 0, y = -0.5: inside the x faces, off their diagonals
    lo, hi = dx[k, j, 2], dx[k, j, 6]       # the centres on the faces x = -1 and x = +1
    assert lo == 0.0 and np.signbit(lo), "on the entry face: the exit face lies ahead, one crossing: inside, -0.0"
    assert hi == 0.0 and not np.signbit(hi), "on the exit face: its own crossing is at the centre, not ahead: outside, +0.0"
    assert (dx[k, j, 3:6] < 0).all() and (dx[k, j, :2] > 0).all() and (dx[k, j, 7:] > 0).all()
    assert dx[k, j, 4] == -0.5 and dx[k, j, 0] == 1.0
    un = _oracle(lib, ses, origin, spacing, dims, INF, sc.UNSIGNED, prim=False)
    assert not np.signbit(un).any() and np.abs(dx).tobytes() == un.tobytes()


def test_max_dist_minus_zero_is_zero(lib, S):
    origin, spacing = sc.grid_around(DIMS, shift=sc.IRRATIONAL)
    a = _oracle(lib, S["sphere"], origin, spacing, DIMS, -0.0, sc.UNSIGNED)
    b = _oracle(lib, S["sphere"], origin, spacing, DIMS, 0.0, sc.UNSIGNED)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and not np.signbit(a[0]).any()


def test_refusals_leave_the_outputs_untouched(lib, S):
    """Statement V7 without a device: the host entry and the plain entry, nothing written.  (A BVH deeper than 64 levels cannot be had from the builder, which
    stops at 61; the pointer and alignment refusals of the device entry need a device: tests/test_gpu_sdf.py.)"""
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    prims = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)],
                                      [dict(minBounds=(1, 0, 0), maxBounds=(1.5, 0.5, 0.5), timeStartMove=0.0, velocity=(0.0, 0.0, 0.0), material=0)])
    raw = lib.Raylib_CreateScene()
    scene = S["sphere"].scene
    P = lambda origin=(-1, -1, -1), spacing=(0.5, 0.5, 0.5), dims=(4, 4, 4), max_dist=INF, sign=sc.MAJORITY: binding.distance_field_params(origin, spacing, dims, max_dist, sign)
    nan = float("nan")
    cases = [("spheres and cubes", prims.scene, P()), ("not finalized", raw, P()), ("null scene", None, P()),
             ("dim 0", scene, P(dims=(4, 0, 4))), ("dim -1", scene, P(dims=(-1, 4, 4))), ("2^31 voxels", scene, P(dims=(2048, 2048, 512))),
             ("2^33 voxels", scene, P(dims=(2048, 2048, 2048))), ("spacing 0", scene, P(spacing=(0.5, 0.0, 0.5))), ("spacing < 0", scene, P(spacing=(-0.5, 0.5, 0.5))),
             ("spacing inf", scene, P(spacing=(0.5, 0.5, INF))), ("spacing NaN", scene, P(spacing=(nan, 0.5, 0.5))), ("origin NaN", scene, P(origin=(0, nan, 0))),
             ("origin inf", scene, P(origin=(0, 0, -INF))), ("last centre overflows", scene, P(origin=(3e38, 0, 0), spacing=(1e37, 1, 1), dims=(100, 1, 1))),
             ("maxDist NaN", scene, P(max_dist=nan)), ("maxDist -1", scene, P(max_dist=-1.0)), ("sign 5", scene, P(sign=5)), ("sign -1", scene, P(sign=-1))]
    try:
        for entry in ("RaylibAMD_BakeDistanceFieldHost", "RaylibAMD_BakeDistanceField"):
            f = getattr(lib, entry)
            dist = np.full(64, POISON, np.uint32); prim = np.full(64, POISON, np.uint32)
            for what, sh, p in cases:
                assert f(sh, C.byref(p), dist.ctypes.data, prim.ctypes.data) == 0, (entry, what)
                assert (dist == POISON).all() and (prim == POISON).all(), (entry, what)
            assert f(scene, None, dist.ctypes.data, prim.ctypes.data) == 0 and f(scene, C.byref(P()), None, prim.ctypes.data) == 0, (entry, "null params, null outDist")
            assert (dist == POISON).all() and (prim == POISON).all(), entry
        dist = np.full(64, POISON, np.uint32)
        assert lib.RaylibAMD_BakeDistanceFieldDevice(scene, C.byref(P(sign=7)), dist.ctypes.data, None, None) == 0 and (dist == POISON).all()
        assert lib.RaylibAMD_BakeDistanceFieldHost(scene, C.byref(P(dims=(1, 1, 1))), dist.ctypes.data, None) == 1, "one voxel is a grid"
        assert (dist[1:] == POISON).all() and dist[0] != POISON
        # the planner refuses what the entries refuse, and takes null plans
        a, b = binding.QueryPlan(), binding.QueryPlan()
        for what, sh, p in cases:
            assert lib.RaylibAMD_PlanDistanceField(sh, C.byref(p), C.byref(a), C.byref(b)) == 0, what
        assert lib.RaylibAMD_PlanDistanceField(scene, None, C.byref(a), C.byref(b)) == 0
        assert lib.RaylibAMD_PlanDistanceField(scene, C.byref(P()), None, None) == 1
    finally:
        lib.Raylib_DestroyScene(raw)
        prims.close()


@pytest.mark.parametrize("env,near,rows", [(None, 4, 8), ("2", 2, 2), ("4", 4, 2), ("8", 4, 8)])
def test_plan_is_the_two_walks_plans(lib, S, monkeypatch, env, near, rows):
    """The distance kernel walks what RaylibAMD_PlanNearest gives CLOSEST, the row kernel what RaylibAMD_PlanRayQueryAll gives (csrc/rl_plan.cc)."""
    if env is not None:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", env)
    origin, spacing = sc.grid_around(DIMS)
    for name in ("sphere", "torus", "doubled"):
        scene = S[name].scene
        rc, pn, pr = binding.plan_distance_field(lib, scene, origin, spacing, DIMS, INF, sc.MAJORITY)
        assert rc == 1 and (pn["treeWidth"], pr["treeWidth"]) == (near, rows), (name, pn, pr)
        rc1, closest = binding.plan_nearest(lib, scene, nc.CLOSEST)
        rc2, allp = binding.plan_ray_query_all(lib, scene, 1, True)
        assert rc1 == 1 and rc2 == 1 and pn == closest and pr == allp
