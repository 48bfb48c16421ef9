#!/usr/bin/env python3
"""What the host BVH builder (csrc/rl_bvh.cc) makes of a fixed list of scenes, one line per fact: RaylibAMD_SceneBVHHash, the numbers and return codes of
RaylibAMD_SceneBVHInfo / BVH4Info / BVH8Info / SceneLeafListInfo, and SHA-256 digests of the raw outputs of RaylibAMD_SceneWalk8Host and of
RaylibAMD_SceneWalkStackHost (every tree, capacity 64 and capacity 3) on a fixed set of rays.  Two builds of the library that print the same lines build the
same trees and walk them the same way, bit for bit: the acceptance test of a change to the builder that must not move a result.  No GPU.

usage: [RAYLIB_LIB=path/to/libraylib.so] python tools/bvh_hashes.py > hashes.txt
Scenes: the Cornell box at tess 1 and 3 and the room (a fifth of its triangles displaced) at tess 24 and 64 (64 also with split leaves, with the greedy
8-wide collapse and with 5 build threads), a 6000-triangle soup, the colonnade at tess 3, every scene of tests/stack_edges.py (with its own rays), an empty
scene and a single triangle.  Result lines only: the library's log is silenced (RAYLIB_QUIET=1)."""
import ctypes as C
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["RAYLIB_QUIET"] = "1"
for _k in ("RAYLIB_BUILD_THREADS", "RAYLIB_W8_SPLIT", "RAYLIB_WIDE_GREEDY", "RAYLIB_W8_TRI_COST", "RAYLIB_BUILD_TIMING"):
    os.environ.pop(_k, None)

import stack_edges  # noqa: E402  (puts the package on sys.path)
from raylib_amd import binding, scenes  # noqa: E402

FLT_MAX = 3.4028235e38
N_RAYS = 4096


def box_rays(lo, hi, seed=17):
    """N_RAYS rays (origin, direction) from a shell around the box [lo, hi] towards points inside it, and from inside it in all directions."""
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    mid, ext = 0.5 * (lo + hi), np.maximum(0.5 * (hi - lo), 1e-3)
    n = N_RAYS // 2
    out_dir = rng.normal(size=(n, 3)); out_dir /= np.linalg.norm(out_dir, axis=1, keepdims=True)
    o = np.concatenate([mid + 3.0 * np.linalg.norm(ext) * out_dir, mid + ext * rng.uniform(-0.95, 0.95, (n, 3))])
    tgt = mid + ext * rng.uniform(-1.0, 1.0, (2 * n, 3))
    d = tgt - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
    return np.concatenate([o, d], 1).astype(np.float32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:32]


def report(lib, name, scene, rays, tmin=1e-4):
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    print("%s hash %016x" % (name, lib.RaylibAMD_SceneBVHHash(scene)))
    n, d, s = C.c_uint32(), C.c_uint32(), C.c_float()
    rc = lib.RaylibAMD_SceneBVHInfo(scene, C.byref(n), C.byref(d), C.byref(s))
    print("%s bvh rc %d nodes %u depth %u sah %s" % (name, rc, n.value, d.value, float(s.value).hex()))
    n4, st4 = C.c_uint32(), C.c_uint32()
    rc = lib.RaylibAMD_SceneBVH4Info(scene, C.byref(n4), C.byref(st4))
    print("%s bvh4 rc %d nodes %u stack %u" % (name, rc, n4.value, st4.value))
    n8, lv, s4, s8 = C.c_uint32(), C.c_uint32(), C.c_float(), C.c_float()
    rc = lib.RaylibAMD_SceneBVH8Info(scene, C.byref(n8), C.byref(lv), C.byref(s4), C.byref(s8))
    print("%s bvh8 rc %d nodes %u levels %u steps4 %s steps8 %s" % (name, rc, n8.value, lv.value, float(s4.value).hex(), float(s8.value).hex()))
    leaves = C.c_uint32()
    rc = lib.RaylibAMD_SceneLeafListInfo(scene, C.byref(leaves))
    print("%s leaflist rc %d leaves %u" % (name, rc, leaves.value))
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    tmax = np.full(len(r), FLT_MAX, np.float32)
    t, steps = np.zeros(len(r), np.float32), np.zeros(len(r), np.uint32)
    rc = lib.RaylibAMD_SceneWalk8Host(scene, r.ctypes.data_as(fp), len(r), float(tmin), tmax.ctypes.data_as(fp), t.ctypes.data_as(fp), steps.ctypes.data_as(up))
    print("%s walk8 rays %d rc %d %s" % (name, len(r), rc, digest(t, steps) if rc == 1 else "-"))
    for tree in (2, 3, 4, 8):
        for cap in (64, 3):
            t, hw = np.zeros(len(r), np.float32), np.zeros(len(r), np.uint32)
            rc = lib.RaylibAMD_SceneWalkStackHost(scene, tree, r.ctypes.data_as(fp), len(r), float(tmin), cap, t.ctypes.data_as(fp), hw.ctypes.data_as(up))
            print("%s walkstack tree %d capacity %d rc %d %s" % (name, tree, cap, rc, digest(t, hw) if rc == 1 else "-"))
    sys.stdout.flush()


def obj_scene(lib, name, obj, env=None):
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        ses = binding.SceneSession(lib, obj, (0.0, 1.0, 4.0), (0.0, 1.0, -1.0), 45.0, 1.0)
    finally:
        for k in (env or {}):
            del os.environ[k]
    tris, _ = ses.export_flat()
    v = np.concatenate([tris["v0"], tris["v1"], tris["v2"]])
    report(lib, name, ses.scene, box_rays(v.min(0), v.max(0)))
    ses.close()


def main():
    lib = binding.load()
    f3 = lambda *v: (C.c_float * 3)(*[float(x) for x in v])
    with tempfile.TemporaryDirectory() as d:
        for tess in (1, 3, 24, 64):   # from tess 24 on as the BASELINE-size room: a fifth of the triangles displaced into it
            obj, _ = scenes.cornell(os.path.join(d, "cornell%d.obj" % tess), tess=tess, displace_fraction=0.2 if tess >= 24 else 0.0)
            obj_scene(lib, ("room_tess%d" if tess >= 24 else "cornell_tess%d") % tess, obj)
        for tag, env in (("split", {"RAYLIB_W8_SPLIT": "1"}), ("greedy", {"RAYLIB_WIDE_GREEDY": "1"}), ("threads5", {"RAYLIB_BUILD_THREADS": "5"})):
            obj_scene(lib, "room_tess64_" + tag, obj, env)
        obj, _ = scenes.soup(os.path.join(d, "soup.obj"), n_tris=6000, seed=9)
        obj_scene(lib, "soup6000", obj)
        obj, _ = scenes.colonnade(os.path.join(d, "colonnade.obj"), tess=3)
        obj_scene(lib, "colonnade_tess3", obj)
        for name, spec in stack_edges.SCENES.items():
            ses, _ = stack_edges.make_session(lib, spec, os.path.join(d, name), name)
            report(lib, name, ses.scene, stack_edges.scene_rays(spec))
            ses.close()
        # the builder's two smallest trees: the root of no primitive at all, and the root whose left child is the only leaf
        scene = lib.Raylib_CreateScene()
        lib.Raylib_FinalizeScene(scene)
        report(lib, "empty", scene, box_rays((-1, -1, -1), (1, 1, 1)))
        lib.Raylib_DestroyScene(scene)
        mat = lib.RaylibAMD_CreateMaterial(0, f3(0.5, 0.5, 0.5), 0.5, 0.0, f3(0, 0, 0), 1.5, f3(1, 1, 1), 0.0)
        nrm = f3(0, 0, 1)
        tri = lib.RaylibAMD_CreateTriangle(f3(0, 0, 0), f3(1, 0, 0), f3(0, 1, 0), nrm, nrm, nrm, None, mat)
        assert mat and tri
        scene = lib.Raylib_CreateScene()
        lib.Raylib_AddSceneElement(scene, tri)
        lib.Raylib_FinalizeScene(scene)
        report(lib, "one_triangle", scene, box_rays((0, 0, -0.5), (1, 1, 0.5)))
        lib.Raylib_DestroyScene(scene)
        lib.RaylibAMD_DestroySceneElement(tri)
        lib.RaylibAMD_DestroyMaterial(mat)


if __name__ == "__main__":
    main()
