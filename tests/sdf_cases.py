"""What tests/test_sdf_host.py (no device) and tests/test_gpu_sdf.py share: the closed meshes a distance field is baked from (a cube, a UV sphere, a torus, the
sphere with every triangle written twice) and statements V1, V4 and V5 of include/raylib_amd.h (RaylibAMD_BakeDistanceField) restated in NumPy.

The restatement is elementwise float32 NumPy: NumPy does not fuse operations, so each + and * rounds once, as the library's -ffp-contract=off build does."""
import os

import numpy as np

import helpers  # noqa: F401  (puts the package on sys.path)
from raylib_amd import binding

F = np.float32
UNSIGNED, SIGN_X, SIGN_Y, SIGN_Z, MAJORITY = binding.SDF_UNSIGNED, binding.SDF_SIGN_X, binding.SDF_SIGN_Y, binding.SDF_SIGN_Z, binding.SDF_SIGN_MAJORITY
SIGNS = (UNSIGNED, SIGN_X, SIGN_Y, SIGN_Z, MAJORITY)
FLT_MAX = float(np.finfo(np.float32).max)
MAX_HITS = 16
SPHERE_RADIUS = 1.0


# ---- meshes ----
def _write(path, verts, faces):
    lines = ["o mesh\n"]
    lines += ["v %.9g %.9g %.9g\n" % tuple(float(x) for x in np.asarray(v, F)) for v in verts]
    lines += ["f %d %d %d\n" % (a + 1, b + 1, c + 1) for a, b, c in faces]
    with open(path, "w") as f:
        f.write("".join(lines))
    return path


def cube_mesh(half=1.0, centre=(0.0, 0.0, 0.0)):
    """An axis-aligned cube of 12 triangles, outward facing."""
    c = np.asarray(centre, np.float64)
    verts = [c + half * np.array([sx, sy, sz], np.float64) for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)]   # index = x + 2 y + 4 z
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    faces = []
    for a, b, cc, d in quads:
        faces += [(a, b, cc), (a, cc, d)]
    return np.array(verts), faces


def sphere_mesh(radius=SPHERE_RADIUS, stacks=16, slices=16, centre=(0.0, 0.0, 0.0)):
    """A UV sphere of 2 * slices * (stacks - 1) = 480 triangles, closed, outward facing: a convex polyhedron."""
    verts = [np.array([0.0, radius, 0.0])]
    for s in range(1, stacks):
        th = np.pi * s / stacks
        for k in range(slices):
            ph = 2 * np.pi * k / slices
            verts.append(radius * np.array([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)]))
    verts.append(np.array([0.0, -radius, 0.0]))
    ring = lambda s, k: 1 + (s - 1) * slices + k % slices
    faces = []
    for k in range(slices):
        faces.append((0, ring(1, k + 1), ring(1, k)))
        faces.append((len(verts) - 1, ring(stacks - 1, k), ring(stacks - 1, k + 1)))
    for s in range(1, stacks - 1):
        for k in range(slices):
            a, b, c, d = ring(s, k), ring(s, k + 1), ring(s + 1, k + 1), ring(s + 1, k)
            faces += [(a, b, c), (a, c, d)]
    return np.array(verts) + np.asarray(centre, np.float64), faces


def torus_mesh(major=1.0, minor=0.4, nu=20, nv=20):
    """A torus around the y axis, 2 * nu * nv = 800 triangles: not convex, a row through it crosses up to four times."""
    verts = []
    for i in range(nu):
        u = 2 * np.pi * i / nu
        for j in range(nv):
            v = 2 * np.pi * j / nv
            r = major + minor * np.cos(v)
            verts.append(np.array([r * np.cos(u), minor * np.sin(v), r * np.sin(u)]))
    at = lambda i, j: (i % nu) * nv + j % nv
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            faces += [(a, b, c), (a, c, d)]
    return np.array(verts), faces


def write_mesh(path, name, **kw):
    """cube, sphere, torus, or doubled: the sphere with every triangle written twice."""
    if name == "cube":
        return _write(path, *cube_mesh(**kw))
    if name == "torus":
        return _write(path, *torus_mesh(**kw))
    verts, faces = sphere_mesh(**kw)
    if name == "doubled":
        faces = [f for f in faces for _ in (0, 1)]
    else:
        assert name == "sphere", name
    return _write(path, verts, faces)


MESHES = ("cube", "sphere", "torus", "doubled")


def session(lib, obj):
    return binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0)


def make_sessions(lib, directory, names=MESHES):
    os.makedirs(directory, exist_ok=True)
    return {n: session(lib, write_mesh(os.path.join(directory, n + ".obj"), n)) for n in names}


def grid_around(dims, lo=-1.6, hi=1.6, shift=(0.0, 0.0, 0.0)):
    """(origin, spacing) of a grid of `dims` voxels over [lo, hi]^3, moved by `shift` voxels per axis; both as float32 values."""
    spacing = np.array([(hi - lo) / n for n in dims], np.float64).astype(F)
    origin = (lo + np.asarray(shift, np.float64) * spacing).astype(F)
    return origin, spacing


# an irrational fraction of a voxel per axis: no centre lies on a vertex, an edge or a face of the meshes above
IRRATIONAL = (np.sqrt(2.0) - 1.0, np.sqrt(3.0) - 1.0, np.sqrt(5.0) - 2.0)


# ---- V1, V4, V5 ----
def axis_t(spacing, n):
    """V1: t_a(i) for i < n."""
    return (np.arange(n).astype(F) + F(0.5)) * F(spacing)


def axis_centres(origin, spacing, n):
    """V1: c_a(i) for i < n."""
    return F(origin) + axis_t(spacing, n)


def centres(origin, spacing, dims):
    """V1: the (nz, ny, nx, 3) float32 voxel centres."""
    cx, cy, cz = (axis_centres(origin[a], spacing[a], dims[a]) for a in range(3))
    out = np.zeros((dims[2], dims[1], dims[0], 3), F)
    out[..., 0] = cx[None, None, :]; out[..., 1] = cy[None, :, None]; out[..., 2] = cz[:, None, None]
    return out


def row_rays(origin, spacing, dims, axis):
    """V3: the (rows, 8) rays of sign axis `axis` -- org, tMin, dir, tMax -- row (ib, ic) of the other two axes b < c at index ic * n_b + ib."""
    b, c = [a for a in range(3) if a != axis]
    cb, cc = axis_centres(origin[b], spacing[b], dims[b]), axis_centres(origin[c], spacing[c], dims[c])
    rays = np.zeros((dims[c], dims[b], 8), F)
    rays[..., axis] = F(origin[axis]); rays[..., b] = cb[None, :]; rays[..., c] = cc[:, None]
    rays[..., 3] = 0.0; rays[..., 4 + axis] = 1.0; rays[..., 7] = FLT_MAX
    return rays.reshape(-1, 8)


def inside_from_crossings(t_hits, counts, spacing, dims, axis):
    """V4: the (nz, ny, nx) bool volume of `axis` from its rows' crossings: t_hits (rows, K) with counts (rows,) of them valid, counts <= K."""
    b, c = [a for a in range(3) if a != axis]
    ta = axis_t(spacing[axis], dims[axis])
    valid = np.arange(t_hits.shape[1])[None, :] < counts[:, None]
    ahead = ((t_hits[:, None, :] > ta[None, :, None]) & valid[:, None, :]).sum(2)      # (rows, n_a)
    odd = (ahead & 1).astype(bool).reshape(dims[c], dims[b], dims[axis])               # [ic, ib, i]
    # to [k, j, i]: x rows are [k, j, i] as they stand, y rows [k, i, j], z rows [j, i, k]
    if axis == 0:
        return odd
    if axis == 1:
        return odd.transpose(0, 2, 1)
    return odd.transpose(2, 0, 1)


def inside_of_mode(inside_xyz, sign):
    """V5: which voxels are negative under `sign`, from the three axes' volumes."""
    if sign == UNSIGNED:
        return np.zeros_like(inside_xyz[0])
    if sign == MAJORITY:
        return (inside_xyz[0].astype(int) + inside_xyz[1] + inside_xyz[2]) >= 2
    return inside_xyz[sign - SIGN_X]


def oracle_inside(lib, ses, origin, spacing, dims):
    """The three axes' inside volumes from RaylibAMD_TraceRaysAllHost on the V3 rays (maxHits 16 and the count, which must not exceed it)."""
    out = []
    for axis in range(3):
        hits, counts = binding.trace_rays_all(lib, ses.scene, row_rays(origin, spacing, dims, axis), MAX_HITS, count=True, host=True)
        assert counts.max() <= MAX_HITS, "a row crosses more than %d times: %d" % (MAX_HITS, counts.max())
        out.append(inside_from_crossings(hits["t"], counts, spacing, dims, axis))
    return out


def bake(lib, ses, origin, spacing, dims, max_dist, sign, **kw):
    return binding.bake_distance_field(lib, ses.scene, origin, spacing, dims, max_dist, sign, **kw)
