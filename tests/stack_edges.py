"""Scenes that sit on the edges of the traversal stacks' capacities (csrc/rl_plan.cc: STACK 16 / 32 / 64 by the binary tree's depth, the 4-wide tree only
if its stackNeed4 fits, the 8-wide tree only up to RL_POOL8_MAXLEVELS levels), and rays that fill those stacks.  Shared by tests/test_stack_edges_host.py
(no device) and tests/test_gpu_stack_edges.py.

Three families:
  * the CONE: triangle j is the base triangle (1, -1, 1), (-1, -1, 1), (0, 1.5, 1) turned by 0.927 j about z and scaled towards the origin (the apex) by a
    fixed ratio per level or by a paced one (cone_scales), the whole thing scaled by `size`.  The SAH builder peels the largest triangle off at every level -- a nearly pure chain whose boxes all contain the
    axis -- and a ray from the apex side enters both boxes of every level: the far child is pushed at every level.  (With a flat chain, all in one plane, a ray
    meets a box only where it crosses the plane and the stack stays empty however deep the tree is.)
  * the CHAIN next to a SOUP (tests/test_render_plan_host.py _write_soup): the soup gives the 8-wide tree its expected steps, the chain the depth.
  * the TWIN CHAINS (twin_chain_triangles): two mirrored, tilted chains on one axis, which load the 8-wide walk's stack of groups to its levels - 1.
Every scene states the numbers the builder must report for it; tests assert them, so a builder change moves a scene off its edge loudly.

Arithmetic: a triangle's `denom` scales with size^4 -- below about 2^-31 of unit size it is no longer a normal float and the triangle cannot be hit, by
the reference either; below about 2^-15 the scene leaves the fast barycentric path; the default rayTMin of 1e-4 hides what is nearer.  Hence `size` 2^20, and 2^30 (the
largest at which uu * vv stays finite) for the cones that need sixty octaves.  Every triangle has a material of its own that emits its own colour: which
triangle a ray hit shows in the pixel at path length 1 already, and in the albedo mode."""
import ctypes as C
import os

import numpy as np

import helpers  # noqa: F401  (puts the package on sys.path)
from raylib_amd import binding

BASE = np.array([[1.0, -1.0, 1.0], [-1.0, -1.0, 1.0], [0.0, 1.5, 1.0]])
SIZE = float(2 ** 20)


def cone_scales(n, ratio=None, pace=None, size=SIZE):
    """The sizes of the cone's triangles, largest first.  ratio: a fixed ratio between neighbours -- the builder peels one triangle per level for about the
    last twenty (ratio 0.25), then several.  pace: the ratio at m triangles to go is min(0.5, sqrt(pace / m)) -- just small enough for the SAH to prefer
    "the largest | the rest" at every level (its cost, area x count, weighs the rest's box r^2 times m), which buys a pure chain of 33 levels inside the 61
    octaves in which a triangle can be hit."""
    s = [float(size)]
    for j in range(1, n):
        s.append(s[-1] * (ratio if pace is None else min(0.5, float(np.sqrt(pace / (n - j))))))
    return s


def _turns(n, c=0.6, s=0.8):
    """(cos, sin) of j turns by the angle whose cosine and sine are 3/5 and 4/5 (0.927 rad), j < n, by repeated complex multiplication: + - * only, so the
    same bits on every machine (a libm's cos / sin may differ in the last place, and the builder's numbers are asserted exactly)."""
    out, x, y = [], 1.0, 0.0
    for _ in range(n):
        out.append((x, y))
        x, y = x * c - y * s, x * s + y * c
    return out


def cone_triangles(n, ratio=None, pace=None, size=SIZE):
    out = np.zeros((n, 3, 3))
    for j, (sc, (c, s)) in enumerate(zip(cone_scales(n, ratio, pace, size), _turns(n))):
        rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        out[j] = (BASE @ rot.T) * sc
    return out.astype(np.float32).astype(np.float64)


def cone_rays(scales):
    """Rays down the chain (origin, direction): from the apex through a 41 x 41 grid of directions around the axis -- such a ray enters every level's boxes, and
    which triangles it misses decides in which stack entry its closest hit sits --, and parallel to the axis at 0.9 and 0.45 of every level's size in eight
    directions: the closest hit at every level in turn."""
    g = (np.arange(41) - 20) * 0.085
    dx, dy = np.meshgrid(g, g)
    d = np.stack([dx.ravel(), dy.ravel(), np.ones(dx.size)], 1)
    rays = [np.concatenate([np.zeros_like(d), d], 1)]
    around = _turns(8, 0.8, 0.6)
    for s in scales:
        for f in (0.9, 0.45):
            for (c, q) in around:
                rays.append(np.array([[f * s * c, f * s * q, 0.0, 0.0, 0.0, 1.0]]))
    return np.concatenate(rays).astype(np.float32)


def soup_chain_triangles(n_soup, n_chain):
    """tests/test_render_plan_host.py _write_soup's triangles."""
    rng = np.random.RandomState(3)
    tris = [c + rng.uniform(-1.0, 1.0, (3, 3)) for c in rng.uniform(-1.0, 1.0, (n_soup, 3))]
    for j in range(1, n_chain + 1):
        c = 2.0 ** -j
        tris.append(np.array([[c, 0, 0], [c + c / 2, 0, 0], [c, c / 2, 0]]))
    return np.array(tris).reshape(-1, 3, 3)


def twin_chain_triangles(n, ratio=0.6, tilt=0.5, size=float(2 ** 30)):
    """Two chains sharing the x axis, mirror images in y and z, each triangle tilted out of its plane so that its box has a volume: the 8-wide collapse gives
    a node two inner children, one per chain, at every level, and a ray from the apex along the axis meets both -- the 8-wide walk's stack of groups takes an
    entry per level."""
    tris, c = [], size
    for _ in range(n):
        c = c * ratio
        tris.append([[c, 0, 0], [c + c / 2, 0, tilt * c], [c, c / 2, tilt * c]])
        tris.append([[c, 0, -tilt * c], [c + c / 2, 0, 0], [c, -c / 2, -tilt * c]])
    return np.array(tris).astype(np.float32).astype(np.float64)


def twin_rays():
    """From the apex through an 81 x 81 grid of directions around the +x axis."""
    g = (np.arange(81) - 40) * 0.015
    dy, dz = np.meshgrid(g, g)
    d = np.stack([np.ones(dy.size), dy.ravel(), dz.ravel()], 1)
    return np.concatenate([np.zeros_like(d), d], 1).astype(np.float32)


def write_obj(path, tris):
    """OBJ + MTL: triangle k has material m<k> -- roughness 1, an albedo and an emission of its own."""
    base = os.path.splitext(path)[0]
    rng = np.random.RandomState(5)
    lines = ["mtllib %s.mtl\n" % os.path.basename(base), "o edge\n"]
    mtl = []
    for k, p in enumerate(tris):
        kd, ke = rng.uniform(0.2, 0.9, 3), rng.uniform(0.1, 2.0, 3)
        mtl.append("newmtl m%d\nNs 10\nKd %.6f %.6f %.6f\nKs 0 0 0\nKe %.6f %.6f %.6f\nillum 2\n\n" % (k, kd[0], kd[1], kd[2], ke[0], ke[1], ke[2]))
        for q in p:
            lines.append("v %.9g %.9g %.9g\n" % tuple(q))
        lines.append("usemtl m%d\nf %d %d %d\n" % (k, 3 * k + 1, 3 * k + 2, 3 * k + 3))
    with open(path, "w") as f:
        f.write("".join(lines))
    with open(base + ".mtl", "w") as f:
        f.write("".join(mtl))
    return path


# name -> how it is made and what the builder must say about it.  depth: the binary tree's; need4: the 4-wide tree's worst-case stack; levels8: the 8-wide
# tree's levels (None: the scene carries no such tree).  `sphere`: one sphere behind the cone (center, radius in units of `size`): the PRIMS instances.
SCENES = {}


def _cone(name, n, depth, need4, levels8=None, ratio=None, pace=None, size=SIZE, sphere=None):
    SCENES[name] = dict(kind="cone", n=n, ratio=ratio, pace=pace, size=size, depth=depth, need4=need4, levels8=levels8, sphere=sphere)


def _chain(name, n_soup, n_chain, depth, need4, levels8):
    SCENES[name] = dict(kind="chain", n_soup=n_soup, n_chain=n_chain, depth=depth, need4=need4, levels8=levels8, sphere=None)


def scene_triangles(spec):
    if spec["kind"] == "cone":
        return cone_triangles(spec["n"], spec["ratio"], spec["pace"], spec["size"])
    if spec["kind"] == "twin":
        return twin_chain_triangles(spec["n"], ratio=spec.get("ratio", 0.6))
    return soup_chain_triangles(spec["n_soup"], spec["n_chain"])


def scene_rays(spec):
    """The rays of a scene (origin, direction): down the cone; for the flat chain, whose boxes a ray meets only in its plane, rays in and across that plane."""
    if spec["kind"] == "cone":
        return cone_rays(cone_scales(spec["n"], spec["ratio"], spec["pace"], spec["size"]))
    if spec["kind"] == "twin":
        return twin_rays()
    rng = np.random.RandomState(11)
    n = 1500
    o = np.concatenate([rng.uniform(-2.0, 2.0, (n, 3)), np.stack([rng.uniform(1.0, 2.0, n), rng.uniform(-0.1, 0.6, n), np.zeros(n)], 1)])
    tgt = np.stack([2.0 ** -rng.uniform(1.0, 24.0, 2 * n), 2.0 ** -rng.uniform(3.0, 26.0, 2 * n), np.zeros(2 * n)], 1)
    d = tgt - o
    return np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(np.float32)


SIZE30 = float(2 ** 30)
SPHERE = ((0.0, 0.0, 1.6), 0.5)   # on the axis behind the largest triangle, in units of the cone's size: an analytic primitive (the PRIMS instances) whose box the rays
                                  # down the axis enter last -- one more entry on their stacks, at the root

# Found by search on the CPU with this tree's builder (RaylibAMD_SceneBVHInfo / BVH4Info / BVH8Info); tests/test_stack_edges_host.py asserts every number.
# On the cones a ray's stack reaches exactly `depth` entries on the binary tree and `need4` on the 4-wide one.
_cone("cone_d16", 17, 16, 16, ratio=0.25)                            # STACK 16 exactly full on the binary tree and on the 4-wide one
_cone("cone_d17", 18, 17, 17, ratio=0.25)                            # one past: STACK 32
_cone("cone_d32", 33, 32, 32, pace=1.1, size=SIZE30)                 # STACK 32 exactly full, both trees
_cone("cone_d33", 34, 33, 33, pace=1.1, size=SIZE30)                 # one past: STACK 64, no pool schedule
_cone("cone_n33", 41, 21, 33, ratio=0.45)                            # the 4-wide tree one past 32: the binary tree for k_trace, the 64 stack for the pool
_cone("cone_n64", 131, 25, 64, 10, ratio=0.74, size=SIZE30)           # the 4-wide tree's 64 stack exactly full
_cone("cone_n65", 132, 26, 65, 10, ratio=0.74, size=SIZE30)           # one past: no 4-wide walk at all
_cone("prims_d16", 17, 16, None, ratio=0.25, sphere=SPHERE)          # spheres: STACK 32 from the start
_cone("prims_d32", 33, 32, None, pace=1.1, size=SIZE30, sphere=SPHERE)
_cone("prims_d33", 34, 33, None, pace=1.1, size=SIZE30, sphere=SPHERE)
# the 8-wide walk's edge: its stack of groups holds at most one entry per level below the root, levels8 - 1; these rays reach exactly that
SCENES["twin_l16"] = dict(kind="twin", n=69, depth=24, need4=67, levels8=16, sphere=None, size=SIZE30)   # 15 groups: the most a tree the planner walks can need
SCENES["twin_l17"] = dict(kind="twin", n=73, depth=25, need4=70, levels8=17, sphere=None, size=SIZE30)   # one past: not walked (its rays would fill all 16 groups)
# ... and the same with a 4-wide need that fits 64, which a render needs before it may walk the 8-wide tree (rl_plan.cc Pick): the pool kernel's 8-wide instance
# with 15 groups in use -- 8 in LDS, 7 in its private overflow --, and one past, 17 levels: the 64-entry grid instance
SCENES["twin_p16"] = dict(kind="twin", n=67, ratio=0.65, depth=22, need4=61, levels8=16, sphere=None, size=SIZE30)
SCENES["twin_p17"] = dict(kind="twin", n=72, ratio=0.65, depth=23, need4=64, levels8=17, sphere=None, size=SIZE30)
_chain("chain_l16", 100, 88, 32, 81, 16)                             # the 8-wide tree at RL_POOL8_MAXLEVELS levels (ray queries walk it)
_chain("chain_l17", 100, 91, 33, 82, 17)                             # one past: not walked; its 4-wide need is above 64 too -- the binary tree, 64 deep
_chain("soup8", 1000, 60, 32, 62, 10)                                # rays expected to take 46 steps: the 8-wide pool instance by default


def deepest_triangles():
    """The deepest tree this generator drives the builder to: a pure chain (ratio 1/8) down to the depth at which the builder stops trusting the SAH
    (kMedianSplitDepth 36), then 4096 degenerate triangles on a line of 1e-30 steps, which it halves by count: 36 + log2 more levels.  The builder's own
    bound is 36 + 25 = 61, for the 2^25 primitives a leaf reference can address."""
    z = np.zeros((4096, 3, 3)); z[:, :, 0] = (np.arange(4096) * 1e-30)[:, None]
    return np.concatenate([cone_triangles(40, 0.125, size=SIZE30), z])


DEEPEST_DEPTH = 45


def scene_sphere(spec):
    if spec["sphere"] is None:
        return None
    (c, r), k = spec["sphere"], spec["size"]
    return (tuple(k * x for x in c), k * r)


def make_session(lib, spec, directory, name, **camera):
    os.makedirs(directory, exist_ok=True)
    obj = write_obj(os.path.join(directory, name + ".obj"), scene_triangles(spec))
    return EdgeSession(lib, obj, sphere=scene_sphere(spec), **camera), obj


def make_flat(oracle, ses, obj, spec, sun=(0, 0, 0), sun_dir=(0.0, -1.0, -0.5)):
    """The oracle's flat scene: the OBJ through the test-side loader, plus the sphere with the material record the library gave it (its last)."""
    from helpers import objflat, ffi
    flat = objflat.load_obj(obj, oracle, sun_illuminance=sun, sun_direction=sun_dir)
    if spec["sphere"] is None:
        return flat
    _, mats = ses.export_flat()
    assert len(mats) == len(flat.materials) + 1 and mats[:-1].tobytes() == flat.materials.tobytes()
    c, r = scene_sphere(spec)
    sph = np.zeros(1, ffi.SPHERE_DTYPE)
    sph[0] = (c, r, len(flat.materials))
    return ffi.FlatScene(flat.triangles, np.concatenate([flat.materials, mats[-1:].astype(ffi.MAT_DTYPE)]), num_shapes=1, spheres=sph,
                         sun_illuminance=sun, sun_direction=sun_dir)


class EdgeSession(binding.SceneSession):
    """binding.SceneSession with, optionally, one sphere element added before the scene is finalized (Raylib_AddSceneElement): render, render_views, stats and
    export_flat are SceneSession's."""

    def __init__(self, lib, obj_path, sphere=None, origin=(0, 0, -1), look_at=(0, 0, 1), fov=45.0, aspect=1.0, sun=(0, 0, 0), sun_dir=(0.0, -1.0, -0.5)):
        self.lib = lib
        self._images = []
        self.obj = lib.Raylib_LoadOBJModel(obj_path.encode())
        assert self.obj, obj_path
        lib.Raylib_FinalizeOBJModel(self.obj)
        self.scene = lib.Raylib_CreateScene()
        lib.Raylib_AddOBJModelToScene(self.scene, self.obj)
        self.mat = self.elem = None
        if sphere is not None:
            f3 = lambda *v: (C.c_float * 3)(*[float(x) for x in v])
            self.mat = lib.RaylibAMD_CreateMaterial(0, f3(0.7, 0.6, 0.5), 0.0, 0.0, None, 0.0, None, 0.0)
            (cx, cy, cz), rad = sphere
            self.elem = lib.RaylibAMD_CreateSphere(float(cx), float(cy), float(cz), float(rad), self.mat)
            assert self.mat and self.elem
            lib.Raylib_AddSceneElement(self.scene, self.elem)
        lib.Raylib_SetSunIlluminance(self.scene, *[float(x) for x in sun])
        lib.Raylib_SetSunDirection(self.scene, *[float(x) for x in sun_dir])
        lib.Raylib_FinalizeScene(self.scene)
        self.camera = binding.create_camera(lib, origin, look_at, fov, aspect)
        self.has_sky = False

    def close(self):
        binding.SceneSession.close(self)
        if self.elem:
            self.lib.RaylibAMD_DestroySceneElement(self.elem)
        if self.mat:
            self.lib.RaylibAMD_DestroyMaterial(self.mat)


def tree_numbers(lib, scene):
    n, d, s = C.c_uint32(), C.c_uint32(), C.c_float()
    assert lib.RaylibAMD_SceneBVHInfo(scene, C.byref(n), C.byref(d), C.byref(s)) == 1
    n4, st4 = C.c_uint32(0), C.c_uint32(0)
    has4 = lib.RaylibAMD_SceneBVH4Info(scene, C.byref(n4), C.byref(st4))
    assert has4 in (0, 1)
    n8, lv, s4, s8 = C.c_uint32(0), C.c_uint32(0), C.c_float(0), C.c_float(0)
    has8 = lib.RaylibAMD_SceneBVH8Info(scene, C.byref(n8), C.byref(lv), C.byref(s4), C.byref(s8))
    assert has8 in (0, 1)
    return dict(depth=d.value, need4=st4.value if has4 else None, levels8=lv.value if has8 else None, steps4=s4.value)


def walk_host(lib, scene, tree, rays6, tmin, capacity):
    """RaylibAMD_SceneWalkStackHost (tree 2 binary, 3 4-wide float boxes, 4 4-wide grid, 8 8-wide): (t per ray, high-water mark per ray)."""
    r = np.ascontiguousarray(rays6, np.float32).reshape(-1, 6)
    t = np.zeros(len(r), np.float32); hw = np.zeros(len(r), np.uint32)
    rc = lib.RaylibAMD_SceneWalkStackHost(scene, int(tree), r.ctypes.data_as(C.POINTER(C.c_float)), len(r), float(tmin), int(capacity),
                                          t.ctypes.data_as(C.POINTER(C.c_float)), hw.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 1, rc
    return t, hw


def instance_of(p):
    """The kernel instance rl_rt_frame.hip KernelFor / AovKernelFor name for a RaylibAMDRenderPlan (as a dict): ("trace", (STACK, PRIMS, FULL, LDS, PLAIN)),
    ("pool", (STACK, PRIMS, K, LSTACK, WIDE)) or ("aov", (STACK, PRIMS)).  Tree codes: 2 float boxes, 3 grid nodes, 4 the 8-wide tree."""
    if not p["pathTrace"]:
        return ("aov", (p["stack"], p["prims"]))
    if p["poolK"] > 0:
        return ("pool", (p["stack"], p["prims"], p["poolK"], p["lstack"], 3 if p["tree"] == 4 else 1 if p["tree"] == 3 else 0))
    if p["lds"] == 2:
        return ("trace", (16, 0, 1, 2, p["plain"]))
    if p["lds"] == 1:
        return ("trace", (16, 0, 1, 1, 0))
    return ("trace", (p["stack"], p["prims"], int(p["tree"] == 2), 0, 0))
