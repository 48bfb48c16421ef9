"""Scenes and plumbing of the moved-triangle tests (RaylibAMD_SceneMoveTriangles), shared by tests/test_move_host.py (no device) and tests/test_gpu_move.py.

The oracle of every GPU test is a second scene created from the moved triangles through the ordinary C ABI -- the same file with other vertex lines, or the
same elements with other vertices -- finalized and given the same call.  What a move is told to do is read off that scene: its export over the range of
triangles in which the two scenes differ."""
import ctypes as C
import os

import numpy as np

import helpers  # noqa: F401  (puts the package on sys.path)
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


def soup_session(lib, directory, name, tris, **camera):
    """The triangles as an OBJ in which each has three vertices and an emitting material of its own (stack_edges.write_obj), loaded and finalized."""
    os.makedirs(str(directory), exist_ok=True)
    obj = stack_edges.write_obj(os.path.join(str(directory), name + ".obj"), tris)
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
