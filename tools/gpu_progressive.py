#!/usr/bin/env python3
"""Progressive rendering timings: the Cornell frame as one Raylib_Render and as progressive sessions of k passes of
spp / k samples, interleaved, medians of wall time per frame (the Step calls, each synchronous).  Run it under rocprofv3 --kernel-trace --stats
for the resolve and compaction kernel times.

usage: tools/gpu_progressive.py [width height spp reps]        (default 1920 1080 64 5)"""
import ctypes as C
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
os.environ.setdefault("RAYLIB_QUIET", "1")
import numpy as np  # noqa: E402
from raylib_amd import binding, scenes  # noqa: E402

w, h, spp, reps = (int(a) for a in (sys.argv[1:5] + ["1920", "1080", "64", "5"][len(sys.argv[1:5]):]))
lib = binding.load()
assert lib.Raylib_Initialize() == 1
lib.RaylibAMD_SetSeed(1)
obj, _ = scenes.cornell(os.path.join(tempfile.mkdtemp(), "cornell.obj"))
ses = binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, w / h)
st = ses.settings(w, h, spp)
img = lib.Raylib_CreateImage(w, h)


def one_shot():
    t = time.perf_counter()
    lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, img)
    return (time.perf_counter() - t) * 1e3, 1


def passes(k):
    def run():
        P = binding.Progressive(ses, w, h, spp, image=img)
        t = time.perf_counter()
        for _ in range(k):
            P.step(spp // k)
        ms = (time.perf_counter() - t) * 1e3
        P.close()
        return ms, k
    return run


variants = [("one Raylib_Render", one_shot), ("%d x %d spp" % (8, spp // 8), passes(8)), ("%d x %d spp" % (spp, 1), passes(spp))]
for _, f in variants:   # warm-up: uploads, allocations, first launches
    f()
times = {name: [] for name, _ in variants}
for r in range(reps):
    for name, f in variants:
        times[name].append(f()[0])
base = float(np.median(times[variants[0][0]]))
print("Cornell %dx%d, %d spp, %d interleaved repetitions (wall ms per frame)" % (w, h, spp, reps))
for name, f in variants:
    med = float(np.median(times[name]))
    k = 1 if name.startswith("one") else int(name.split()[0])
    extra = "" if k == 1 else "  overhead per pass %.3f ms" % ((med - base) / k)
    print("  %-20s median %8.3f  min %8.3f  max %8.3f  (x %.3f)%s" % (name, med, min(times[name]), max(times[name]), med / base, extra))
lib.Raylib_DestroyImage(img)
ses.close()
