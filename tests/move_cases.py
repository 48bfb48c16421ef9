"""Scenes and plumbing of the moved-triangle tests (RaylibAMD_SceneMoveTriangles), shared by tests/test_move_host.py (no device), tests/test_gpu_move.py and
tests/test_gpu_refit_exact.py: the scenes, what a move is told, the refit of the binary tree restated in NumPy (refit_boxes), and the random sequences of
moves, rebuilds, reads and queries that are run against a model (Sequence, replay).

The oracle of every GPU test is a second scene created from the moved triangles through the ordinary C ABI -- the same file with other vertex lines, or the
same elements with other vertices -- finalized and given the same call.  What a move is told to do is read off that scene: its export over the range of
triangles in which the two scenes differ."""
import ctypes as C
import os
import re

import numpy as np

import helpers  # noqa: F401  (puts the package on sys.path)
import nearest_cases
import stack_edges
from raylib_amd import binding, scenes

W, H, SPP, MAX_PATH = 64, 48, 4, 5
F = np.float32


# ---- scenes ----
def soup_triangles(n=600, seed=5, spread=1.0, size=0.15):
    """n triangles around centres in [-spread, spread]^3, as float32 values: the smallest soup that carries every tree (more than 108 triangles for the 8-wide one)."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3))
    return (c + rng.uniform(-size, size, (n, 3, 3))).astype(F).astype(np.float64)


def soup_session(lib, directory, name, tris, normals=None, **camera):
    """The triangles as an OBJ in which each has three vertices and an emitting material of its own (stack_edges.write_obj), loaded and finalized.
    normals: (n, 9) float32 shading normals, written as vn lines of their own per corner (the loader takes them as they are); None: the loader's face normals."""
    os.makedirs(str(directory), exist_ok=True)
    obj = stack_edges.write_obj(os.path.join(str(directory), name + ".obj"), tris)
    if normals is not None:
        out, k = [], 0
        with open(obj) as f:
            for line in f:
                if line.startswith("usemtl"):
                    out += ["vn %.9g %.9g %.9g\n" % tuple(float(x) for x in normals[k][3 * j:3 * j + 3]) for j in range(3)]
                elif line.startswith("f "):
                    line = "f %d//%d %d//%d %d//%d\n" % tuple(3 * k + 1 + j // 2 for j in range(6)); k += 1
                out.append(line)
        assert k == len(normals) == len(tris)
        with open(obj, "w") as f:
            f.write("".join(out))
    camera.setdefault("origin", (0.2, 0.3, 4.0)); camera.setdefault("look_at", (0, 0, 0))
    return stack_edges.EdgeSession(lib, obj, **camera)


def edit_obj(src, dst, move_v=None, move_vn=None):
    """A copy of an OBJ (beside it: the MTL and the textures are found again) whose k-th vertex / normal line holds move_v(k, xyz) / move_vn(k, xyz) as float32."""
    out, kv, kn = [], 0, 0
    with open(src) as f:
        for line in f:
            tok = line.split()
            if tok and tok[0] == "v" and move_v is not None:
                p = np.asarray(move_v(kv, np.array(tok[1:4], np.float64).astype(F)), F); kv += 1
                line = "v %.9g %.9g %.9g\n" % tuple(float(x) for x in p)
            elif tok and tok[0] == "vn" and move_vn is not None:
                p = np.asarray(move_vn(kn, np.array(tok[1:4], np.float64).astype(F)), F); kn += 1
                line = "vn %.9g %.9g %.9g\n" % tuple(float(x) for x in p)
            out.append(line)
    with open(dst, "w") as f:
        f.write("".join(out))
    return dst


def case_session(lib, name, obj):
    c = helpers.CASES[name]
    return binding.SceneSession(lib, obj, c["origin"], c["look_at"], c["fov"], c["aspect"], sun=c["sun"], sun_dir=c["sun_dir"], aperture=c["aperture"], focal=c["focal"],
                                shutter=c["shutter"], sky_image=scenes.sky_panorama() if c["sky"] else None)


class ElementSession:
    """Loose triangles (v (3, 3), n (3, 3), uv (6,), material index) beside spheres and cubes (helpers.procedural_case's records) through the element ABI;
    render / stats / export_flat / close as binding.SceneSession's."""

    def __init__(self, lib, mats, triangles, spheres=(), cubes=(), origin=(0, 0.5, 3), look_at=(0, 0, -1), fov=45.0, aspect=W / H, shutter=(0.0, 0.0), sun=(0, 0, 0),
                 sun_dir=(0.0, -1.0, -0.5)):
        self.lib, self.has_sky = lib, False
        self.mats = [binding.create_material(lib, m) for m in mats]
        assert all(self.mats)
        self.scene = lib.Raylib_CreateScene()
        self.elems = []
        fp = lambda a: np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
        for s in spheres:
            self.elems.append(lib.RaylibAMD_CreateSphere(float(s["center"][0]), float(s["center"][1]), float(s["center"][2]), float(s["radius"]), self.mats[int(s["material"])]))
        for c in cubes:
            self.elems.append(lib.RaylibAMD_CreateCube(f3(c["minBounds"]), f3(c["maxBounds"]), float(c["timeStartMove"]), f3(c["velocity"]), self.mats[int(c["material"])]))
        for v, n, uv, m in triangles:
            v, n = np.asarray(v, F), np.asarray(n, F)
            self.elems.append(lib.RaylibAMD_CreateTriangle(fp(v[0]), fp(v[1]), fp(v[2]), fp(n[0]), fp(n[1]), fp(n[2]), fp(uv), self.mats[int(m)]))
        assert all(self.elems)
        for e in self.elems:
            lib.Raylib_AddSceneElement(self.scene, e)
        lib.Raylib_SetSunIlluminance(self.scene, *[float(x) for x in sun])
        lib.Raylib_SetSunDirection(self.scene, *[float(x) for x in sun_dir])
        lib.Raylib_FinalizeScene(self.scene)
        self.camera = binding.create_camera(lib, origin, look_at, fov, aspect, shutter=shutter)

    render = binding.SceneSession.render
    settings = binding.SceneSession.settings
    stats = binding.SceneSession.stats
    export_flat = binding.SceneSession.export_flat

    def close(self):
        lib = self.lib
        lib.Raylib_DestroyScene(self.scene); lib.Raylib_DestroyCamera(self.camera)
        for e in self.elems:
            lib.RaylibAMD_DestroySceneElement(e)
        for m in self.mats:
            lib.RaylibAMD_DestroyMaterial(m)


def quad_triangles(corners, normal, material):
    """Two triangles of a quad with the unit square as their lightmap UVs."""
    p = np.asarray(corners, F)
    n = np.tile(np.asarray(normal, F), (3, 1))
    return [(p[[0, 1, 2]], n, np.asarray([0, 0, 1, 0, 1, 1], F), material), (p[[0, 2, 3]], n, np.asarray([0, 0, 1, 1, 0, 1], F), material)]


# ---- what a move is told ----
def export(ses):
    return ses.export_flat()[0]


def pos9(t):
    return np.ascontiguousarray(np.concatenate([t["v0"], t["v1"], t["v2"]], 1), F)


def nrm9(t):
    return np.ascontiguousarray(np.concatenate([t["n0"], t["n1"], t["n2"]], 1), F)


def changed_range(a, b):
    """[first, end) over the triangles whose vertices or shading normals differ between two exports of the same topology."""
    assert len(a) == len(b) and a["material"].tobytes() == b["material"].tobytes() and a["st"].tobytes() == b["st"].tobytes()
    d = (helpers.bits(pos9(a)) != helpers.bits(pos9(b))).any(1) | (helpers.bits(nrm9(a)) != helpers.bits(nrm9(b))).any(1)
    idx = np.nonzero(d)[0]
    assert len(idx), "the two scenes are the same"
    return int(idx[0]), int(idx[-1]) + 1


def move_to(lib, ses, fresh, device=False):
    """Move `ses` to where `fresh` is: the range in which they differ, with normals only where those differ.  device: through torch tensors on the current
    stream.  Returns (the library's answer, first, end)."""
    a, b = export(ses), export(fresh)
    first, end = changed_range(a, b)
    P = pos9(b[first:end])
    N = nrm9(b[first:end]) if (helpers.bits(nrm9(a[first:end])) != helpers.bits(nrm9(b[first:end]))).any() else None
    if N is not None:
        # a triangle without area has no normal: the loader gives the fresh scene NaNs for it, which a move refuses; it keeps the normals it has (never hit, never shaded)
        lost = ~np.isfinite(N).all(1)
        N[lost] = nrm9(a[first:end])[lost]
    if device:
        import torch
        P = torch.from_numpy(P).cuda()
        N = None if N is None else torch.from_numpy(N).cuda()
    return binding.move_triangles(lib, ses.scene, first, P, N), first, end


def same_triangles(a, b):
    """Two exports agree: every word, the shading normals of triangles without area aside (NaN in a scene loaded with them: move_to)."""
    n = np.isfinite(nrm9(b)).all(1)
    rest = [k for k in a.dtype.names if k not in ("n0", "n1", "n2")]
    return all(a[k].tobytes() == b[k].tobytes() for k in rest) and helpers.bits(nrm9(a))[n].tobytes() == helpers.bits(nrm9(b))[n].tobytes()


def same_bits(a, b):
    return np.array_equal(helpers.bits(a), helpers.bits(b))


def check_trees(lib, scene):
    failed = C.c_uint32(99)
    return lib.RaylibAMD_SceneCheckTrees(scene, C.byref(failed)), failed.value


def bvh_info(lib, scene):
    n, d, s = C.c_uint32(), C.c_uint32(), C.c_float()
    ok = lib.RaylibAMD_SceneBVHInfo(scene, C.byref(n), C.byref(d), C.byref(s))
    return ok, n.value, d.value, s.value


NODE_DTYPE = np.dtype([("lmin", "f4", 3), ("lmax", "f4", 3), ("rmin", "f4", 3), ("rmax", "f4", 3), ("left", "i4"), ("right", "i4"), ("pad", "i4", 2)])


def bvh_nodes(lib, scene):
    """RaylibAMD_SceneExportBVHNodes: the binary tree's nodes, node 0 the root."""
    nodes = np.zeros(lib.RaylibAMD_SceneExportBVHNodes(scene, None), NODE_DTYPE)
    assert lib.RaylibAMD_SceneExportBVHNodes(scene, nodes.ctypes.data) == len(nodes) > 0
    return nodes


def tri_order(lib, scene):
    """RaylibAMD_SceneExportTriOrder: order[slot] = the export index of the triangle in that slot."""
    order = np.zeros(lib.RaylibAMD_SceneNumTriangles(scene), np.uint32)
    assert lib.RaylibAMD_SceneExportTriOrder(scene, order.ctypes.data_as(C.POINTER(C.c_uint32))) == 1
    return order


def compare_trees(lib, scene):
    return binding.compare_trees(lib, scene)


def assert_wide_trees_exact(lib, scene):
    """RaylibAMD_SceneCompareTrees: every wide format the device holds is the host's rule applied to the device's binary boxes, byte for byte."""
    rc, mask = compare_trees(lib, scene)
    assert (rc, mask) == (1, 0), "RaylibAMD_SceneCompareTrees returned %d, formats that differ (1 float-4, 2 grid-4, 4 leaf list, 8 8-wide, 16 records): %d" % (rc, mask)


# ---- the refit of the binary tree, restated (csrc/rl_k_refit.inl k_refit_level) ----
# the leaf reference's fields and the empty child, read from where the kernels take them
with open(os.path.join(helpers.ROOT, "software-raytracing_amd", "csrc", "rl_device.h")) as _f:
    _text = _f.read()
LEAF_FIRST_SHIFT, LEAF_KIND_SHIFT, LEAF_KIND_MASK, LEAF_COUNT_MASK = (int(re.search(r"\b%s = (\d+)u?\b" % k, _text).group(1))
                                                                      for k in ("LEAF_FIRST_SHIFT", "LEAF_KIND_SHIFT", "LEAF_KIND_MASK", "LEAF_COUNT_MASK"))
DNODE_EMPTY = -2 ** 31
assert re.search(r"#define DNODE_EMPTY \(\(int32_t\)0x80000000\)", _text)
FLT_MAX = np.finfo(F).max


def sel_min(a, b):
    """SelMin: the second operand only where it is strictly less (np.minimum would pick either zero)."""
    return np.where(b < a, b, a)


def sel_max(a, b):
    return np.where(a < b, b, a)


def node_levels(nodes):
    """The depth of every node; children follow their parent (the builder numbers the nodes in pre-order)."""
    depth = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):
        for ref in (int(nodes["left"][i]), int(nodes["right"][i])):
            if ref >= 0:
                assert i < ref < len(nodes), "the binary tree is not in pre-order"
                depth[ref] = depth[i] + 1
    return depth


def refit_boxes(nodes, tris, order):
    """k_refit_level in NumPy: the nodes (NODE_DTYPE: RaylibAMD_SceneExportBVHNodes) with every child box made again from the triangles (an export) in their
    slots (order: RaylibAMD_SceneExportTriOrder), level by level from the deepest.  A triangle leaf's box: from [FLT_MAX, -FLT_MAX], folded over its slots in
    order with SelMin(mn, SelMin(SelMin(v0, v1), v2)) and its mirror; an inner child's: SelMin(c.lmin, c.rmin) / SelMax(c.lmax, c.rmax) of that child node as
    the deeper level left it; an empty child, a sphere leaf and a cube leaf keep the box they have."""
    out = np.array(nodes, NODE_DTYPE, copy=True)
    V = np.stack([tris["v0"], tris["v1"], tris["v2"]], 1).astype(F)[np.asarray(order, np.int64)]       # (slot, vertex, axis)
    tmin, tmax = sel_min(sel_min(V[:, 0], V[:, 1]), V[:, 2]), sel_max(sel_max(V[:, 0], V[:, 1]), V[:, 2])
    depth = node_levels(out)
    for d in range(int(depth.max()), -1, -1):
        at = np.nonzero(depth == d)[0]
        for side, lo, hi in (("left", "lmin", "lmax"), ("right", "rmin", "rmax")):
            ref = out[side][at].astype(np.int64)
            inner = ref >= 0
            c = out[ref[inner]]
            mn, mx = out[lo][at], out[hi][at]
            mn[inner], mx[inner] = sel_min(c["lmin"], c["rmin"]), sel_max(c["lmax"], c["rmax"])
            code = (~ref) & 0xffffffff
            leaf = (ref < 0) & (ref != DNODE_EMPTY) & (((code >> LEAF_KIND_SHIFT) & LEAF_KIND_MASK) == 0)     # a triangle leaf
            first, count = code >> LEAF_FIRST_SHIFT, (code & LEAF_COUNT_MASK) + 1
            assert (first[leaf] + count[leaf] <= len(V)).all()
            lmn, lmx = np.full((int(leaf.sum()), 3), FLT_MAX, F), np.full((int(leaf.sum()), 3), -FLT_MAX, F)
            for k in range(LEAF_COUNT_MASK + 1):
                has = count[leaf] > k
                slot = first[leaf][has] + k
                lmn[has], lmx[has] = sel_min(lmn[has], tmin[slot]), sel_max(lmx[has], tmax[slot])
            mn[leaf], mx[leaf] = lmn, lmx
            out[lo][at], out[hi][at] = mn, mx
    return out


BOXES = ("lmin", "lmax", "rmin", "rmax")


def refit_of(lib, ses):
    """(the scene's binary nodes as the host holds them, refit_boxes of their topology over the scene's current triangles)."""
    nodes = bvh_nodes(lib, ses.scene)
    return nodes, refit_boxes(nodes, export(ses), tri_order(lib, ses.scene))


def assert_refit_exact(lib, ses, bits=True):
    """The binary tree's boxes are refit_boxes of its own topology and the scene's triangles.  bits: bit for bit -- the boxes were written by the device's refit
    (a move has happened since the last build); else as values, because the builder grows an inner node's box over its primitives and a zero's sign may differ
    (csrc/rl_k_refit.inl ChildBox)."""
    nodes, want = refit_of(lib, ses)
    for k in BOXES:
        same = (helpers.bits(nodes[k]) == helpers.bits(want[k])) if bits else (nodes[k] == want[k])
        assert same.all(), "%s of node %d: %r, restated %r" % (k, np.nonzero(~same.all(1))[0][0], nodes[k][~same.all(1)][0], want[k][~same.all(1)][0])
    assert all(nodes[k].tobytes() == want[k].tobytes() for k in ("left", "right", "pad"))


def render_camera(lib, ses, camera, w=W, h=H, spp=SPP):
    """Raylib_Render of the session's scene through another camera handle."""
    st = binding.RendererSettings(int(w), int(h), int(spp), MAX_PATH, 1e-4, 0)
    img = lib.Raylib_CreateImage(w, h)
    lib.Raylib_Render(C.byref(st), ses.scene, camera, img)
    out = np.zeros((h, w, 4), F)
    lib.RaylibAMD_DumpImageRGBA(img, out.ctypes.data_as(C.POINTER(C.c_float)))
    lib.Raylib_DestroyImage(img)
    return out


def query_rays(n=3000, seed=9, extent=2.5):
    r = helpers.random_rays(n, seed, extent)
    return helpers.rays8(r[:, :3], r[:, 3:])


# ---- random sequences of moves, rebuilds, reads and queries against a model (tests/test_gpu_refit_exact.py) ----
# The model is the scene's current triangles as float32 values: positions and shading normals, (n, 9) each, in export order.  Every op is applied to the model
# and to the scene; at a check a fresh scene is created from the model through the ordinary C ABI, and it is the yardstick.
FW, FH, FSPP = 32, 24, 2          # the frame of a check
N_RAYS = 512                      # rays and points of a check
N_OPS = 12
TIE_CAP = 0.01                    # the share of a check's rays that may be left out of the primitive comparison for an exact-t tie
SHUTTERS = ((0.0, 1.0), (0.0, 0.5), (0.25, 0.75), (0.0, 0.0))
ENTRIES = ("host", "device", "stream")
SHAPES = ("rigid", "jitter", "point", "segment", "shrink", "restore")
READS = ("export", "info", "hash", "lightmap")
ROTATIONS = [np.array(m, np.float64) for m in ([[0.6, -0.8, 0], [0.8, 0.6, 0], [0, 0, 1]], [[1, 0, 0], [0, 0.6, -0.8], [0, 0.8, 0.6]], [[0.6, 0, 0.8], [0, 1, 0], [-0.8, 0, 0.6]])]


def set_structure(name, structures):
    """The planner's switches of a structure (test_gpu_move.STRUCTURES) straight into the environment: move_cases.replay's, where no monkeypatch is at hand."""
    for k in ("RAYLIB_POOL", "RAYLIB_BVH4", "RAYLIB_BVH8", "RAYLIB_QUERY_TREE", "RAYLIB_LAZY_REFL", "RAYLIB_LEAF_LIST", "RAYLIB_LDS_SCENE"):
        os.environ.pop(k, None)
    os.environ.update(structures[name][0])


def procedural_quads():
    """Scene class 2: helpers.procedural_case's spheres and moving cube, and two quads (four triangles) beside them."""
    mats, sph, cub, cam = helpers.procedural_case()
    tris = quad_triangles([(-1.5, -0.45, 0.9), (-0.7, -0.45, 0.9), (-0.7, 0.5, 0.7), (-1.5, 0.5, 0.7)], (0, 0.2, 1), 2) + \
        quad_triangles([(0.6, -0.4, 0.8), (1.1, -0.4, 0.8), (1.1, 0.2, 0.6), (0.6, 0.2, 0.6)], (0, 0.3, 1), 4)
    return mats, sph, cub, cam, tris


def face_normals(P, rng):
    """Shading normals to give a move: each corner's the face normal, bent a little; a triangle without area gets a random unit vector."""
    p = P.reshape(-1, 3, 3).astype(np.float64)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    bad = ~(np.linalg.norm(n, axis=1) > 1e-30)
    n[bad] = rng.normal(size=(int(bad.sum()), 3))
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    n = n[:, None, :] + rng.uniform(-0.2, 0.2, (len(p), 3, 3))
    n = n / np.linalg.norm(n, axis=2, keepdims=True)
    return np.ascontiguousarray(n.reshape(-1, 9), F)


def tied_rays(host_rows):
    """Per ray: its row of RaylibAMD_TraceRaysAllHost records holds two hits at the same t (their order is the slots': a moved scene's and a fresh scene's may differ)."""
    valid = host_rows["prim"] >= 0
    return (valid[:, 1:] & valid[:, :-1] & (host_rows["t"][:, 1:] == host_rows["t"][:, :-1])).any(1)


class Sequence:
    """One random sequence: N_OPS ops drawn by np.random.RandomState(seed), each applied to the model and (unless dry) to the scene, with the checks of
    tests/test_gpu_refit_exact.py behind them.  klass 1: a soup of 300 triangles (materials and camera as soup_session's); klass 2: procedural_quads, where the
    ops are moves, renders, ray queries and shutter changes (a frame or a query at another time builds that scene again on the host: launched()).  Behind every
    op: the builder's checks on what the device holds, the wide formats as values (RaylibAMD_SceneCompareTrees), the binary boxes against refit_boxes, the
    topology hash; a move drawn quiet has none of that behind it -- nothing of the test's stands between it and the next op.  Behind every third op and the
    last, a fresh scene made from the model is asked for everything the scene is asked for; its BVHHash and TopologyHash are the scene's when a rebuild has
    happened and no move since.  dry: no device -- the model alone, and at every check the fresh scene's host oracle, from which
    the share of tied rays is taken (the generator is run this way before its seeds are committed).
    use_structure(name): sets the planner's switches (the test's monkeypatch, or set_structure)."""

    def __init__(self, lib, directory, seed, klass, use_structure, structures, dry=False):
        self.lib, self.dir, self.seed, self.klass, self.use_structure, self.structures, self.dry = lib, str(directory), int(seed), klass, use_structure, structures, dry
        self.rng = np.random.RandomState(self.seed)
        self.tag = "fz%d_%d%s" % (klass, self.seed, "d" if dry else "")
        self.log, self.keep, self.fresh_count, self.max_tied = [], [], 0, 0.0
        self.rays = query_rays(N_RAYS, seed=1000 + self.seed, extent=2.5)
        self.shutter = None
        if klass == 1:
            self.ses = soup_session(lib, self.dir, self.tag + "_a", soup_triangles(300, seed=100 + self.seed))
            self.amp = 0.5
        else:
            self.mats, self.sph, self.cub, self.cam, self.tris0 = procedural_quads()
            self.shutter = tuple(self.cam["shutter"])
            self.ses = self.element_session([t[0] for t in self.tris0], [t[1] for t in self.tris0])
            self.amp = 0.3
        t = export(self.ses)
        self.P, self.N = pos9(t), nrm9(t)
        self.n = len(t)
        self.saved = {}                     # (first, end) -> the positions a shrink took away, for the move that scales them back
        self.refitted = False               # the device's refit wrote the binary boxes last (else: the builder)
        self.clean_rebuild = False          # RaylibAMD_SceneRebuild has happened and no move since: the trees are a fresh scene's
        if not dry:
            import torch
            self.torch, self.stream = torch, torch.cuda.Stream()
            use_structure("binary")
            self.ses.render(FW, FH, 1, MAX_PATH)       # the scene is on the device, under the binary tree's switches, before anything moves
            self.topology = lib.RaylibAMD_SceneTopologyHash(self.ses.scene)
            if klass == 2:                             # nearest-point and multi-hit queries refuse a scene with spheres and cubes: said once per sequence
                for call in (lambda: binding.nearest_points(lib, self.ses.scene, np.zeros((4, 4), F), binding.NEAREST_CLOSEST),
                             lambda: binding.trace_rays_all(lib, self.ses.scene, self.rays[:4], 4)):
                    try:
                        call()
                    except RuntimeError:
                        continue
                    raise AssertionError("a query family that refuses spheres and cubes answered")

    # -- scenes from the model --
    def element_session(self, V, Nn):
        cam = self.cam
        tris = [(np.asarray(v, F).reshape(3, 3), np.asarray(n, F).reshape(3, 3), t0[2], t0[3]) for v, n, t0 in zip(V, Nn, self.tris0)]
        return ElementSession(self.lib, self.mats, tris, spheres=self.sph, cubes=self.cub, origin=cam["origin"], look_at=cam["look_at"], fov=cam["fov"], aspect=cam["aspect"],
                              shutter=self.shutter, sun=cam["sun"], sun_dir=cam["sun_dir"])

    def fresh_session(self):
        self.fresh_count += 1
        if self.klass == 1:
            return soup_session(self.lib, self.dir, "%s_b%d" % (self.tag, self.fresh_count), self.P.reshape(-1, 3, 3).astype(np.float64), normals=self.N)
        return self.element_session(self.P, self.N)

    # -- drawing an op: everything random about it, and its effect on the model --
    def draw(self):
        rng = self.rng
        kinds = (["move"] * 9 + ["refused"] * 2 + ["read"] * 3 + ["switch"] * 2 + ["rebuild"] * 2 + ["progressive"]) if self.klass == 1 else \
                (["move"] * 8 + ["refused"] * 2 + ["render"] * 2 + ["trace"] * 2 + ["shutter"] * 3)
        op = dict(kind=kinds[rng.randint(len(kinds))])
        if op["kind"] == "move":
            count = int(rng.randint(1, min(100, self.n) + 1))
            first = int(rng.randint(0, self.n - count + 1))
            shape = SHAPES[rng.randint(len(SHAPES))]
            if shape == "restore" and not self.saved:
                shape = "shrink"
            if shape == "restore":
                first, end = sorted(self.saved)[rng.randint(len(self.saved))]
                P = self.saved.pop((first, end))
            else:
                p = self.P[first:first + count].reshape(-1, 3, 3).astype(np.float64)
                if shape == "rigid":
                    p = p @ ROTATIONS[rng.randint(3)].T + rng.uniform(-self.amp, self.amp, 3)
                elif shape == "jitter":
                    p = p + rng.uniform(-0.05, 0.05, p.shape)
                elif shape == "point":
                    p = np.repeat(p.mean(1, keepdims=True), 3, 1)
                elif shape == "segment":          # v0, v0 + d, v0 + 2 d with v0 on a grid of 2^-10 and d = 2^-3 along one axis: exactly collinear in float32
                    v0 = np.round(p.mean(1) * 1024.0) / 1024.0
                    d = np.zeros(3); d[rng.randint(3)] = 0.125
                    p = np.stack([v0, v0 + d, v0 + 2 * d], 1)
                else:                              # by 2^-35 about the range's centroid: what is left of a triangle at this scale has a divisor below 2^-62, or none
                    self.saved[(first, first + count)] = self.P[first:first + count].copy()
                    c = p.reshape(-1, 3).mean(0)
                    p = c + (p - c) * 2.0 ** -35
                P = np.ascontiguousarray(p.reshape(-1, 9), F)
            count = len(P)
            # a range that takes only a part of a shrunk one forgets that one: it is scaled back as a whole or not at all
            for key in [k for k in self.saved if k[0] < first + count and first < k[1] and (shape == "restore" or k != (first, first + count))]:
                del self.saved[key]
            N = face_normals(P, rng) if rng.randint(2) else None
            entry = ENTRIES[rng.randint(len(ENTRIES))]
            quiet = entry == "stream" or rng.randint(3) == 0       # nothing of the test's between this move and the next op
            op.update(first=first, count=count, shape=shape, P=P, N=N, entry=entry, quiet=bool(quiet))
            self.P[first:first + count] = P
            if N is not None:
                self.N[first:first + count] = N
        elif op["kind"] == "refused":
            op["what"] = ("nan_host", "nan_stream", "past_end")[rng.randint(3)]
            count = int(rng.randint(1, min(8, self.n) + 1))
            op["count"] = count
            op["first"] = int(rng.randint(0, self.n - count + 1)) if op["what"] != "past_end" else self.n - count + 1 + int(rng.randint(0, 3))
            P = self.P[:count] + F(0.25)
            if op["what"] != "past_end":
                P[rng.randint(count), rng.randint(9)] = np.nan
            op["P"] = P
            op["quiet"] = op["what"] == "nan_stream"
        elif op["kind"] == "read":
            op["what"] = READS[rng.randint(len(READS))]
            op["first"] = int(rng.randint(0, self.n - 1))
        elif op["kind"] == "switch":
            op["structure"] = sorted(self.structures)[rng.randint(len(self.structures))]
        elif op["kind"] == "shutter":
            op["shutter"] = SHUTTERS[rng.randint(len(SHUTTERS))]
            self.shutter = op["shutter"]
        return op

    @staticmethod
    def describe(op):
        skip = ("P", "N", "kind")
        return op["kind"] + "(" + ", ".join("%s=%s" % (k, v) for k, v in op.items() if k not in skip) + (", normals" if op.get("N") is not None else "") + ")"

    # -- an op on the scene --
    def to_device(self, a, on_stream):
        if a is None:
            return None
        t = self.torch.from_numpy(np.ascontiguousarray(a, F))
        t = t.pin_memory().to("cuda", non_blocking=True) if on_stream else t.cuda()
        self.keep.append(t)
        return t

    def move(self, first, P, N, entry):
        lib, scene = self.lib, self.ses.scene
        if entry == "host":
            return binding.move_triangles(lib, scene, first, P, N)
        if entry == "device":       # torch's default stream: the library's own stream, synchronous
            return binding.move_triangles(lib, scene, first, self.to_device(P, False), self.to_device(N, False))
        with self.torch.cuda.stream(self.stream):      # the values reach the device on the caller's stream, the move goes behind them and returns at once
            return binding.move_triangles(lib, scene, first, self.to_device(P, True), self.to_device(N, True))

    def render(self, ses, spp=FSPP):
        img = ses.render(FW, FH, spp, MAX_PATH)
        self.launched()
        return img

    def launched(self):
        """(klass 2) A frame or a query at another time than the scene's boxes were built for builds the scene of a moving cube again on the host, from the moved
        triangles: behind either, the boxes may be the builder's and the topology another."""
        if self.klass == 2:
            self.refitted, self.topology = False, self.lib.RaylibAMD_SceneTopologyHash(self.ses.scene)

    def apply(self, op):
        lib, ses, kind = self.lib, self.ses, op["kind"]
        if kind == "move":
            assert self.move(op["first"], op["P"], op["N"], op["entry"]) == 1
            self.refitted, self.clean_rebuild = True, False
        elif kind == "refused":
            before = self.P.copy()
            if op["what"] == "nan_host":
                assert binding.move_triangles(lib, ses.scene, op["first"], op["P"]) == 0
            elif op["what"] == "nan_stream":
                assert self.move(op["first"], op["P"], None, "stream") == 1      # accepted; found out on the device, not applied
            else:
                assert self.move(op["first"], op["P"], None, ("host", "device")[op["first"] % 2]) == 0
            assert self.P.tobytes() == before.tobytes()
        elif kind == "read":
            if op["what"] == "export":
                t = export(ses)
                assert same_bits(pos9(t), self.P) and same_bits(nrm9(t), self.N), "the host's triangles are not the model's"
            elif op["what"] == "info":
                ok, nodes, depth, sah = bvh_info(lib, ses.scene)
                assert ok == 1 and np.isfinite(sah)
            elif op["what"] == "hash":
                assert lib.RaylibAMD_SceneBVHHash(ses.scene) not in (0, self.topology)
            else:
                _, _, k = binding.lightmap_points(lib, ses.scene, 16, 16, tri_first=op["first"], tri_count=2, host=True)
                assert k >= 0
        elif kind == "switch":       # the next launches walk that structure: a wide tree the device does not hold yet is uploaded from the host's copy, refitted first
            self.use_structure(op["structure"])
            self.render(ses, 1)
            binding.trace_rays(lib, ses.scene, self.rays[:64], binding.QUERY_CLOSEST)
        elif kind == "rebuild":
            assert lib.RaylibAMD_SceneRebuild(ses.scene) == 1
            self.refitted, self.clean_rebuild = False, True
            self.topology = lib.RaylibAMD_SceneTopologyHash(ses.scene)
        elif kind == "progressive":
            prog = binding.Progressive(ses, FW, FH, 8)
            assert prog.handle
            assert binding.move_triangles(lib, ses.scene, 0, self.P[:4]) == 0 and self.move(0, self.P[:4], None, "device") == 0, "a move while a progressive session is open"
            prog.close()
        elif kind == "render":
            self.render(ses)
        elif kind == "trace":
            binding.trace_rays(lib, ses.scene, self.rays[:64], binding.QUERY_CLOSEST)
            self.launched()
        elif kind == "shutter":
            lib.Raylib_CameraSetMotion(ses.camera, float(op["shutter"][0]), float(op["shutter"][1]))      # (the next frame builds the scene again, for this interval)

    # -- the checks --
    def check_cheap(self):
        lib, ses = self.lib, self.ses
        got = check_trees(lib, ses.scene)
        assert got == (1, 0), "RaylibAMD_SceneCheckTrees returned %d, the tree that failed: %d" % got
        assert_wide_trees_exact(lib, ses.scene)
        assert_refit_exact(lib, ses, bits=self.refitted)
        assert lib.RaylibAMD_SceneTopologyHash(ses.scene) == self.topology, "the topology changed without a rebuild"

    def tie_share(self, fresh):
        rows = binding.trace_rays_all(self.lib, fresh.scene, self.rays, binding.MAX_HITS, host=True)
        tied = tied_rays(rows)
        self.max_tied = max(self.max_tied, float(tied.mean()))
        assert tied.mean() <= TIE_CAP, "%d of %d rays meet two surfaces at one t: above the cap" % (tied.sum(), len(tied))
        return tied

    def check_fresh(self, index):
        lib, ses = self.lib, self.ses
        fresh = self.fresh_session()
        try:
            if self.klass == 1:
                tied = self.tie_share(fresh)
            if self.dry:
                return
            assert same_triangles(export(ses), export(fresh)), "export"
            assert same_bits(self.render(ses), self.render(fresh)), "frame"
            for kind in (binding.QUERY_ANY, binding.QUERY_CLOSEST, binding.QUERY_SURFACE):
                got = binding.trace_rays(lib, ses.scene, self.rays, kind, with_prim=(kind == binding.QUERY_SURFACE))
                want = binding.trace_rays(lib, fresh.scene, self.rays, kind, with_prim=(kind == binding.QUERY_SURFACE))
                assert [a.tobytes() for a in (got if isinstance(got, tuple) else (got,))] == [a.tobytes() for a in (want if isinstance(want, tuple) else (want,))], "trace_rays kind %d" % kind
            self.launched()
            if self.klass == 1:
                pts = nearest_cases.point_set(np.random.RandomState(2000 + 100 * self.seed + index), export(fresh), N_RAYS)
                for kind, p in ((binding.NEAREST_CLOSEST, pts), (binding.NEAREST_WITHIN, nearest_cases.with_max_dist(pts, 0.05))):
                    got, want, host = (binding.nearest_points(lib, s.scene, p, kind, host=h) for s, h in ((ses, False), (fresh, False), (fresh, True)))
                    assert got.tobytes() == want.tobytes() == host.tobytes(), "nearest kind %d" % kind
                for k in (1, 4, binding.MAX_HITS):
                    for count in (False, True):
                        got = binding.trace_rays_all(lib, ses.scene, self.rays, k, count=count)
                        want = binding.trace_rays_all(lib, fresh.scene, self.rays, k, count=count, host=True)
                        if count:
                            (got, got_n), (want, want_n) = got, want
                            assert np.array_equal(got_n, want_n), "multi-hit count, max_hits %d" % k
                        assert all(same_bits(got[f], want[f]) for f in ("t", "b1", "b2")), "multi-hit records, max_hits %d, count %d" % (k, count)
                        assert (got["prim"] == want["prim"])[~tied].all(), "multi-hit primitives, max_hits %d, count %d" % (k, count)
            if self.clean_rebuild:
                assert lib.RaylibAMD_SceneBVHHash(ses.scene) == lib.RaylibAMD_SceneBVHHash(fresh.scene), "BVHHash behind a rebuild"
                assert lib.RaylibAMD_SceneTopologyHash(ses.scene) == lib.RaylibAMD_SceneTopologyHash(fresh.scene), "TopologyHash behind a rebuild"
        finally:
            fresh.close()

    def run(self, upto=N_OPS):
        print("sequence: class %d, seed %d" % (self.klass, self.seed))
        for i in range(upto):
            op = self.draw()
            what = self.describe(op)
            print("  op %2d: %s" % (i, what))
            try:
                if not self.dry:
                    self.apply(op)
                    if not op.get("quiet"):
                        self.check_cheap()
                if i % 3 == 2 or i == upto - 1:
                    self.check_fresh(i)
                if i == upto - 1 and not self.dry:
                    self.check_cheap()
            except (AssertionError, RuntimeError) as e:
                raise AssertionError("class %d, seed %d, op %d, %s: %s" % (self.klass, self.seed, i, what, e)) from e
        if not self.dry:
            self.stream.synchronize()
        return self

    def close(self):
        self.keep = []
        self.ses.close()


def replay(seed, upto=N_OPS, klass=1, lib=None, directory=None, use_structure=None, structures=None, dry=False):
    """The first `upto` ops of a sequence, for cutting a failure down by hand: python -c "import move_cases; move_cases.replay(3, 7)" from tests/ (dry=True:
    no device, the model and the host oracle alone)."""
    if structures is None:
        import test_gpu_move
        structures = test_gpu_move.STRUCTURES
    if lib is None:
        lib = binding.load()
        assert dry or lib.Raylib_Initialize() == 1
    if directory is None:
        import tempfile
        directory = tempfile.mkdtemp()
    seq = Sequence(lib, directory, seed, klass, use_structure or (lambda name: set_structure(name, structures)), structures, dry=dry)
    try:
        return seq.run(upto)
    finally:
        seq.close()
