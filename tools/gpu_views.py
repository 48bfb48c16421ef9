#!/usr/bin/env python3
"""A batch of N views (RaylibAMD_RenderViewsDevice, one launch per sample batch) against N sequential one-view renders (RaylibAMD_RenderDevice) of the same
cameras: wall ms and the trace kernels' ms (RaylibAMDStats.traceKernelMs, summed over the sequential calls), median of --runs, the two interleaved.

usage: python tools/gpu_views.py [--views 1,2,6,16] [--sizes 256x256,1920x1080] [--spp 64] [--runs 5] [--scenes cornell,room]
The cameras circle the scene (a turntable).  Prints one table row per point and, with --json PATH, writes the rows there.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("RAYLIB_QUIET", "1")

from raylib_amd import binding, scenes  # noqa: E402


def session(lib, name, d):
    if name == "cornell":
        obj, _ = scenes.cornell(os.path.join(d, "cornell.obj"))
        return binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    obj, _ = scenes.cornell(os.path.join(d, "room.obj"), tess=91, displace_fraction=0.2)   # the tessellated room of the bench (298 k triangles)
    return binding.SceneSession(lib, obj, (0, 1, 5), (0, 1, -1), 60.0, 1.0, sun=(20, 20, 20), sun_dir=(-1.0, -1.0, 0.0))


def turntable(lib, n, aspect, radius):
    cams = []
    for i in range(n):
        a = 2.0 * math.pi * i / max(1, n) * 0.25 - 0.4   # a quarter turn in front of the open side of the room
        cams.append(binding.create_camera(lib, (radius * math.sin(a), 1.0, radius * math.cos(a)), (0.0, 1.0, -1.0), 45.0, aspect))
    return cams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="1,2,6,16")
    ap.add_argument("--sizes", default="256x256,1920x1080")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scenes", default="cornell,room")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1, "no device"
    lib.RaylibAMD_SetSeed(1)
    d = tempfile.mkdtemp()
    rows = []
    print("%-8s %-10s %3s %4s | %10s %10s | %10s %10s | %6s %6s" % ("scene", "size", "N", "spp", "batch ms", "seq ms", "batch kms", "seq kms", "wall x", "kern x"))
    for name in a.scenes.split(","):
        ses = session(lib, name, d)
        for size in a.sizes.split(","):
            w, h = [int(x) for x in size.split("x")]
            for n in [int(x) for x in a.views.split(",")]:
                cams = turntable(lib, n, w / h, 4.0)
                st = ses.settings(w, h, a.spp)
                arr = binding.handle_array(cams)
                bw, bk, sw, sk = [], [], [], []
                for r in range(a.runs + 1):   # (the first round warms up: uploads, allocations, occupancy queries)
                    assert lib.RaylibAMD_RenderViewsDevice(C.byref(st), ses.scene, arr, n, None) == 1
                    s = ses.stats()
                    if r:
                        bw.append(s.wallMs); bk.append(s.traceKernelMs)
                    tw = tk = 0.0
                    for c in cams:
                        assert lib.RaylibAMD_RenderDevice(C.byref(st), ses.scene, c, 0, 1, None) == 1
                        s = ses.stats()
                        tw += s.wallMs; tk += s.traceKernelMs
                    if r:
                        sw.append(tw); sk.append(tk)
                med = lambda v: sorted(v)[len(v) // 2]
                row = dict(scene=name, w=w, h=h, views=n, spp=a.spp, batch_wall_ms=med(bw), seq_wall_ms=med(sw), batch_trace_ms=med(bk), seq_trace_ms=med(sk),
                           batch_wall_all=bw, seq_wall_all=sw)
                rows.append(row)
                print("%-8s %-10s %3d %4d | %10.2f %10.2f | %10.2f %10.2f | %6.3f %6.3f" % (name, size, n, a.spp, row["batch_wall_ms"], row["seq_wall_ms"],
                      row["batch_trace_ms"], row["seq_trace_ms"], row["seq_wall_ms"] / row["batch_wall_ms"], row["seq_trace_ms"] / max(1e-9, row["batch_trace_ms"])), flush=True)
                for c in cams:
                    lib.Raylib_DestroyCamera(c)
        ses.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
