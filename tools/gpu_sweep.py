#!/usr/bin/env python3
"""Standalone swept-sphere query rates (RaylibAMD_SweepSpheresDevice on device-resident queries, the library's stream, HIP-event time of the kernel) for each
kind, tree and move length, beside RaylibAMD_NearestPointsDevice CLOSEST at the same origins.

usage: python tools/gpu_sweep.py [--size 1024] [--runs 20] [--radius 0.01] [--moves 0.01,0.1,1] [--log PATH]
The scene is the tessellated room of the bench (298 k triangles, a fifth of them displaced), seen from inside.  The origins are the hit points of the camera
rays of a size x size pinhole view (1 M at the default), two radii off the surface along the normal: a sphere resting just clear of the geometry, as a particle
or a character sphere is between steps.  The radius is --radius scene extents; the moves have uniform random directions and a length of each of --moves scene
extents.  Per row: after two warm-up calls the median, the least and the greatest kernel time of --runs calls (the event pair of the synchronous entry brackets
the kernel alone), node and triangle records per query from the call's counters, and the share of queries that hit.  The rows of one (move, kind) alternate
between the trees call by call.  Every row carries the library's build id.
"""
import argparse
import ctypes as C
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("RAYLIB_QUIET", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--radius", type=float, default=0.01)
    ap.add_argument("--moves", default="0.01,0.1,1")
    ap.add_argument("--tess", type=int, default=91)
    ap.add_argument("--log")
    args = ap.parse_args()
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
    from gpu_ray_query import camera_rays
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1, "no HIP device"
    d = tempfile.mkdtemp()
    obj, _ = scenes.cornell(os.path.join(d, "room.obj"), tess=args.tess, displace_fraction=0.2)
    cam = ((0, 1, 0.9), (0, 1, -1), 60.0)
    ses = binding.SceneSession(lib, obj, cam[0], cam[1], cam[2], 1.0)
    tris, _ = ses.export_flat()
    lo = np.minimum(np.minimum(tris["v0"].min(0), tris["v1"].min(0)), tris["v2"].min(0))
    hi = np.maximum(np.maximum(tris["v0"].max(0), tris["v1"].max(0)), tris["v2"].max(0))
    ext = float((hi - lo).max())
    r = np.float32(args.radius * ext)
    surf = binding.trace_rays(lib, ses.scene, camera_rays(np, args.size, args.size, *cam), binding.QUERY_SURFACE)
    h = surf["hit"] == 1
    org = (surf["p"][h] + 2 * r * surf["n"][h]).astype(np.float32)
    n = len(org)
    rng = np.random.RandomState(1)
    dirs = rng.normal(size=(n, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    out_lines = []

    def say(s):
        print(s); out_lines.append(s)

    say("# tools/gpu_sweep.py: %d triangles, extent %.3f, %d queries, radius %g extents, build %s" % (len(tris), ext, n, args.radius, lib.RaylibAMD_BuildId().decode()))
    say("# kernel ms from the synchronous entry's event pair: median, least and greatest of %d calls after 2 warm-up calls; nodes and tris per query" % args.runs)
    say("%-10s %-8s %-6s %5s %9s %9s %9s %10s %8s %8s %6s" % ("call", "move", "tree", "stack", "ms", "min", "max", "Mquery/s", "nodes", "tris", "hit"))

    def measure(calls):
        """calls: name -> function returning the entry's return code; the calls take turns.  name -> (ms list, last stats)."""
        got = {k: ([], None) for k in calls}
        for it in range(args.runs + 2):
            for k, f in calls.items():
                assert f() == 1
                st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
                if it >= 2:
                    got[k][0].append(st.kernelMs)
                got[k] = (got[k][0], st)
        return got

    trees = []
    for tree in ("2", "4"):
        os.environ["RAYLIB_QUERY_TREE"] = tree
        rc, plan = binding.plan_sweep(lib, ses.scene, 1)
        if rc == 1 and str(plan["treeWidth"]) == tree:
            trees.append((tree, {"2": "bvh2", "4": "grid4"}[tree], plan["stack"]))
    # the yardstick: NearestPoints CLOSEST at the same origins, maxDist +inf
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([org, np.full((n, 1), np.inf, np.float32)], 1))).cuda()
    near_out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def nearest_call(tree):
        def f():
            os.environ["RAYLIB_QUERY_TREE"] = tree
            return lib.RaylibAMD_NearestPointsDevice(ses.scene, 1, C.c_void_p(pts.data_ptr()), n, C.c_void_p(near_out.data_ptr()), None)
        return f
    got = measure({t[0]: nearest_call(t[0]) for t in trees})
    for tree, tname, stack in trees:
        ms, st = got[tree]
        say("%-10s %-8s %-6s %5d %9.3f %9.3f %9.3f %10.1f %8.2f %8.2f %6s" % ("nearest", "-", tname, stack, np.median(ms), min(ms), max(ms), n / np.median(ms) / 1e3, st.nodesVisited / n,
                                                                      st.trisTested / n, "-"))
    outs = {0: torch.empty(n, dtype=torch.int32, device="cuda"), 1: torch.empty((n, 8), dtype=torch.int32, device="cuda")}
    for move in [float(x) for x in args.moves.split(",")]:
        q = np.zeros((n, 8), np.float32)
        q[:, 0:3] = org; q[:, 3] = r; q[:, 4:7] = dirs * (move * ext)
        dev = torch.from_numpy(q).cuda()
        torch.cuda.synchronize()
        for kind, kname in ((1, "closest"), (0, "any")):
            def sweep_call(tree):
                def f():
                    os.environ["RAYLIB_QUERY_TREE"] = tree
                    return lib.RaylibAMD_SweepSpheresDevice(ses.scene, kind, C.c_void_p(dev.data_ptr()), n, C.c_void_p(outs[kind].data_ptr()), None)
                return f
            got = measure({t[0]: sweep_call(t[0]) for t in trees})
            o = outs[kind].cpu().numpy()
            hit = float((o[:, 1] >= 0).mean()) if kind == 1 else float((o != 0).mean())
            for tree, tname, stack in trees:
                ms, st = got[tree]
                say("%-10s %-8g %-6s %5d %9.3f %9.3f %9.3f %10.1f %8.2f %8.2f %6.3f" % ("sweep " + kname[:3], move, tname, stack, np.median(ms), min(ms), max(ms), n / np.median(ms) / 1e3,
                                                                                 st.nodesVisited / n, st.trisTested / n, hit))
    os.environ.pop("RAYLIB_QUERY_TREE", None)
    ses.close()
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(out_lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
