#!/usr/bin/env python3
"""A move of a finalized scene's triangles measured against what a caller does without it (RaylibAMD_SceneMoveTrianglesDevice, RaylibAMD_SceneRebuild;
include/raylib_amd.h), a fifth of the triangles moved:

  a   RaylibAMD_SceneMoveTrianglesDevice on the library's stream, to completion (host clock around the synchronous call: records, the refit of every tree the
      device holds, the status read-back); the first move of the scene, which also makes and uploads its tables, apart
  b   destroy the scene, create it again from the loaded model, Raylib_FinalizeScene, and the first upload (a one-ray query): host clock
  c   the frame (kernelMs of Raylib_Render) on the trees as built, on the refitted trees, and after RaylibAMD_SceneRebuild -- the trees of a scene created from the
      moved triangles (tests/test_gpu_move.py: the same hash), so the fresh scene's frame

RUNS runs of every item after a warm-up (a's 2 RUNS moves go back and forth; c's three states follow one another: a state cannot alternate with the others without
moving or rebuilding in between).  One process; every GPU step runs under a time limit of its own, after which the process ends with status 124.

usage: python tools/gpu_move.py [--tess 91] [--width 1920] [--height 1080] [--spp 16] [--runs 5] [--out PATH]
The scene is raylib_amd.scenes.textured (298 116 triangles at its default size), camera "breakfast", as tools/gpu_gather_adaptive.py.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import torch    # before the library is loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("RAYLIB_QUIET", "1")

from gpu_gather_adaptive import Limit   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tess", type=int, default=91)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from raylib_amd import binding, scenes
    lib = binding.load()
    with Limit(120, "initialising the device"):
        assert lib.Raylib_Initialize() == 1, "no HIP device"
    lib.RaylibAMD_SetSeed(1)
    lib.RaylibAMD_BuildId.restype = C.c_char_p
    d = tempfile.mkdtemp()
    obj, n_tris = scenes.textured(os.path.join(d, "textured.obj"), tess=a.tess)
    cam = scenes.CONFIG_CAMERAS["breakfast"]
    ses = binding.SceneSession(lib, obj, cam["origin"], cam["look_at"], cam["fov"], a.width / a.height, sun=cam["sun"], sun_dir=cam["sun_dir"])
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def frame():
        with Limit(300, "Raylib_Render"):
            ses.render(a.width, a.height, a.spp)
        st = ses.stats()
        return st.kernelMs, st.treeWidth

    def one_ray():
        binding.trace_rays(lib, ses.scene, np.asarray([[0, 1, 0, 1e-4, 0, 0, -1, 3e38]], np.float32), binding.QUERY_CLOSEST)

    frame(); one_ray()                                  # the warm-up: the scene's upload, the work buffers
    tris = ses.export_flat()[0]
    count = n_tris // 5
    base = np.ascontiguousarray(np.concatenate([tris["v0"], tris["v1"], tris["v2"]], 1)[:count], np.float32)
    there = torch.from_numpy(base + np.tile(np.asarray([0.05, 0.02, 0.03], np.float32), 3)).cuda()
    back = torch.from_numpy(base).cuda()
    torch.cuda.synchronize()

    def move(p):
        t0 = time.perf_counter()
        with Limit(120, "RaylibAMD_SceneMoveTrianglesDevice"):
            ok = lib.RaylibAMD_SceneMoveTrianglesDevice(ses.scene, 0, count, C.c_void_p(p.data_ptr()), None, None)
        assert ok == 1
        return (time.perf_counter() - t0) * 1e3

    def recreate():
        t0 = time.perf_counter()
        with Limit(300, "destroy, create, finalize, first upload"):
            lib.Raylib_DestroyScene(ses.scene)
            ses.scene = lib.Raylib_CreateScene()
            lib.Raylib_AddOBJModelToScene(ses.scene, ses.obj)
            lib.Raylib_SetSunIlluminance(ses.scene, *[float(x) for x in cam["sun"]])
            lib.Raylib_SetSunDirection(ses.scene, *[float(x) for x in cam["sun_dir"]])
            lib.Raylib_FinalizeScene(ses.scene)
            one_ray()
        return (time.perf_counter() - t0) * 1e3

    built = [frame() for _ in range(a.runs)]
    first_move = move(there)
    moves = []
    for _ in range(a.runs):                             # back and forth on the one upload: every call after the first finds the scene's tables in place
        moves.append(move(back)); moves.append(move(there))
    refit = [frame() for _ in range(a.runs)]
    with Limit(300, "RaylibAMD_SceneRebuild"):
        t0 = time.perf_counter()
        assert lib.RaylibAMD_SceneRebuild(ses.scene) == 1
        one_ray()
        rebuild_ms = (time.perf_counter() - t0) * 1e3
    rebuilt = [frame() for _ in range(a.runs)]
    recreated = [recreate() for _ in range(a.runs)]
    say("build %s: scenes.textured tess %d (%d triangles), %d of them moved (a fifth), frames %d x %d at %d spp, maxPathLength 5; %d runs of every item after a warm-up"
        % (lib.RaylibAMD_BuildId().decode(), a.tess, n_tris, count, a.width, a.height, a.spp, a.runs))
    say("a  first move of an upload (tables made and uploaded, then the move): %.3f ms" % first_move)
    say("a  RaylibAMD_SceneMoveTrianglesDevice, library's stream, to completion | ms: %s | median %.3f" % (" ".join("%.3f" % v for v in moves), statistics.median(moves)))
    say("b  destroy + create + Raylib_FinalizeScene + first upload              | ms: %s | median %.3f" % (" ".join("%.1f" % v for v in recreated), statistics.median(recreated)))
    say("   RaylibAMD_SceneRebuild + first upload (once)                        | ms: %.1f" % rebuild_ms)
    for name, rows in (("as built", built), ("refitted", refit), ("rebuilt = fresh", rebuilt)):
        ms = [r[0] for r in rows]
        say("c  frame on the trees %-16s (treeWidth %d) | ms: %s | fastest %.3f median %.3f slowest %.3f" % (name, rows[0][1], " ".join("%.3f" % v for v in ms), min(ms), statistics.median(ms), max(ms)))
    say("a / b = %.5f (medians); frame refitted / frame fresh = %.4f (medians)"
        % (statistics.median(moves) / statistics.median(recreated), statistics.median([r[0] for r in refit]) / statistics.median([r[0] for r in rebuilt])))
    ses.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
