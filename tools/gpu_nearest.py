#!/usr/bin/env python3
"""Standalone nearest-point query rates (RaylibAMD_NearestPointsDevice on device-resident points, the library's stream, HIP-event time of the kernel) for each
kind and tree.

usage: python tools/gpu_nearest.py [--scenes cornell,room] [--width 1920] [--height 1080] [--runs 5] [--timeout 600] [--lib PATH] [--json PATH]
Two point sets per scene: surface-near points -- the hit points of the camera rays of a width x height pinhole view, offset by 1e-3 along the normal (what a
contact or snapping query asks) -- and as many uniform points in the scene's bounds (what a distance-field bake asks); maxDist +inf.  After one warm-up call,
the median of --runs calls.  Each scene is measured in a child process under its own time limit; one table row per (scene, points, tree, kind).  --lib: another
build of the library (an A/B of a kernel setting).
--all: RaylibAMD_NearestPointsAllDevice instead (the K nearest triangles and the count in range), on the same point sets and trees: maxHits 1, 4 and 16, without
the count (maxDist +inf) and with it (maxDist = the median 8th-neighbour distance of a 4096-point subsample, computed by the host oracle); the median, the least
and the greatest of --runs kernel times, node and triangle records per point, the median count, and beside each row RaylibAMD_NearestPointsDevice(CLOSEST) on
the same points in the same process.  Every row carries the library's build id.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("RAYLIB_QUIET", "1")

KINDS = {0: "within", 1: "closest"}


def all_rows(args, lib, ses, np, torch, set_name, pts):
    """--all: RaylibAMD_NearestPointsAllDevice on one point set, for each tree, maxHits 1, 4 and 16, without the count (maxDist +inf, as CLOSEST) and with it
    (maxDist = the median 8th-neighbour distance of a 4096-point subsample, which the host oracle computes); beside each, CLOSEST on the same points."""
    from raylib_amd import binding
    n = len(pts)
    sub = pts[np.random.RandomState(2).permutation(n)[:4096]]
    eighth = binding.nearest_points_all(lib, ses.scene, np.ascontiguousarray(sub), 8, host=True)["dist2"][:, 7]
    radius = float(np.median(np.sqrt(eighth.astype(np.float64))))
    ranged = np.array(pts, np.float32); ranged[:, 3] = radius
    dev = {False: torch.from_numpy(np.ascontiguousarray(pts)).cuda(), True: torch.from_numpy(ranged).cuda()}
    closest = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    hits = torch.empty((n * 16, 4), dtype=torch.int32, device="cuda")
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def timed(call):
        ks = []
        for _ in range(args.runs + 1):   # the first is the warm-up
            assert call() == 1
            st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
            ks.append(st.kernelMs)
        return float(np.median(ks[1:])), float(min(ks[1:])), float(max(ks[1:])), st

    rows = []
    for tree in ("2", "4"):
        os.environ["RAYLIB_QUERY_TREE"] = tree
        rc, plan = binding.plan_nearest_all(lib, ses.scene, 1)
        if str(plan["treeWidth"]) != tree:
            continue   # the scene has no such tree
        for count in (False, True):
            p = C.c_void_p(dev[count].data_ptr())
            c_ms, c_lo, c_hi, _ = timed(lambda: lib.RaylibAMD_NearestPointsDevice(ses.scene, 1, p, n, C.c_void_p(closest.data_ptr()), None))
            for max_hits in (1, 4, 16):
                ms, lo, hi, st = timed(lambda: lib.RaylibAMD_NearestPointsAllDevice(ses.scene, p, n, max_hits, C.c_void_p(hits.data_ptr()),
                                                                                      C.c_void_p(counts.data_ptr()) if count else None, None))
                rows.append(dict(scene=args.scene, points=set_name, n=n, tree={"2": "bvh2", "4": "grid4"}[tree], stack=plan["stack"], max_hits=max_hits, count=count,
                                 max_dist=radius if count else "inf", ms=ms, ms_min=lo, ms_max=hi, gpoints=n / ms / 1e6, nodes_per_point=st.nodesVisited / n,
                                 tris_per_point=st.trisTested / n, median_count=float(np.median(counts.cpu().numpy().view(np.uint32))) if count else None,
                                 closest_ms=c_ms, closest_ms_min=c_lo, closest_ms_max=c_hi, timing="kernel", build=lib.RaylibAMD_BuildId().decode()))
    os.environ.pop("RAYLIB_QUERY_TREE", None)
    return rows


def child(args):
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
    from gpu_ray_query import camera_rays
    lib = binding.load(args.lib) if args.lib else binding.load()
    assert lib.Raylib_Initialize() == 1
    d = tempfile.mkdtemp()
    if args.scene == "cornell":
        obj, _ = scenes.cornell(os.path.join(d, "cornell.obj"))
        cam = ((0, 1, 4), (0, 1, -1), 45.0)
    else:   # the tessellated room of the bench (298 k triangles), seen from inside
        obj, _ = scenes.cornell(os.path.join(d, "room.obj"), tess=91, displace_fraction=0.2)
        cam = ((0, 1, 0.9), (0, 1, -1), 60.0)
    ses = binding.SceneSession(lib, obj, cam[0], cam[1], cam[2], 1.0)
    tris, _ = ses.export_flat()
    surf = binding.trace_rays(lib, ses.scene, camera_rays(np, args.width, args.height, *cam), binding.QUERY_SURFACE)
    h = surf["hit"] == 1
    near = np.concatenate([surf["p"][h] + np.float32(1e-3) * surf["n"][h], np.full((int(h.sum()), 1), np.inf, np.float32)], 1).astype(np.float32)
    lo = np.minimum(np.minimum(tris["v0"].min(0), tris["v1"].min(0)), tris["v2"].min(0))
    hi = np.maximum(np.maximum(tris["v0"].max(0), tris["v1"].max(0)), tris["v2"].max(0))
    uni = np.concatenate([np.random.RandomState(1).uniform(lo, hi, (len(near), 3)), np.full((len(near), 1), np.inf)], 1).astype(np.float32)
    rows = []
    if args.all:
        for set_name, pts in (("surface", near), ("uniform", uni)):
            rows += all_rows(args, lib, ses, np, torch, set_name, pts)
        ses.close()
        print("ROWS " + json.dumps(rows))
        return
    for set_name, pts in (("surface", near), ("uniform", uni)):
        n = len(pts)
        dev = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
        outs = {0: torch.empty(n, dtype=torch.int32, device="cuda"), 1: torch.empty((n, 4), dtype=torch.int32, device="cuda")}
        torch.cuda.synchronize()
        for tree in ("2", "4"):
            os.environ["RAYLIB_QUERY_TREE"] = tree
            rc, plan = binding.plan_nearest(lib, ses.scene, 1)
            if str(plan["treeWidth"]) != tree:
                continue   # the scene has no such tree
            for kind in (0, 1):
                ks, ws = [], []
                for _ in range(args.runs + 1):
                    assert lib.RaylibAMD_NearestPointsDevice(ses.scene, kind, C.c_void_p(dev.data_ptr()), n, C.c_void_p(outs[kind].data_ptr()), None) == 1
                    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
                    ks.append(st.kernelMs); ws.append(st.wallMs)
                k_ms, w_ms = float(np.median(ks[1:])), float(np.median(ws[1:]))
                rows.append(dict(scene=args.scene, points=set_name, n=n, tree={"2": "bvh2", "4": "grid4"}[tree], kind=KINDS[kind], stack=plan["stack"], ms=k_ms, wall_ms=w_ms,
                                 gpoints=n / k_ms / 1e6, nodes_per_point=st.nodesVisited / n, tris_per_point=st.trisTested / n, timing="kernel"))
        os.environ.pop("RAYLIB_QUERY_TREE", None)
    ses.close()
    print("ROWS " + json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,room")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--lib")
    ap.add_argument("--json")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scene")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for name in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--scene", name, "--width", str(args.width), "--height", str(args.height), "--runs", str(args.runs)]
        if args.all:
            cmd += ["--all"]
        if args.lib:
            cmd += ["--lib", args.lib]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("%s: over the %d s limit; stopping" % (name, args.timeout)); break
        if r.returncode != 0:
            print("%s: exit status %d; stopping\n%s" % (name, r.returncode, r.stderr[-3000:])); break
        rows += json.loads([l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
    if args.all:
        print("%-8s %-8s %9s %-6s %4s %-5s %9s %9s %9s %10s %8s %8s %7s | %9s %9s %9s" % ("scene", "points", "n", "tree", "K", "count", "ms", "min", "max", "Gpoints/s", "nodes", "tris",
                                                                                       "median", "closest", "min", "max"))
        for w in rows:
            print("%-8s %-8s %9d %-6s %4d %-5s %9.3f %9.3f %9.3f %10.3f %8.2f %8.2f %7s | %9.3f %9.3f %9.3f" % (
                w["scene"], w["points"], w["n"], w["tree"], w["max_hits"], "yes" if w["count"] else "no", w["ms"], w["ms_min"], w["ms_max"], w["gpoints"], w["nodes_per_point"],
                w["tris_per_point"], "-" if w["median_count"] is None else "%g" % w["median_count"], w["closest_ms"], w["closest_ms_min"], w["closest_ms_max"]))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(rows, f, indent=1)
        return 0
    print("%-8s %-8s %9s %-6s %-8s %9s %10s %8s %8s" % ("scene", "points", "n", "tree", "kind", "ms", "Gpoints/s", "nodes", "tris"))
    for w in rows:
        print("%-8s %-8s %9d %-6s %-8s %9.3f %10.3f %8.2f %8.2f" % (w["scene"], w["points"], w["n"], w["tree"], w["kind"], w["ms"], w["gpoints"], w["nodes_per_point"],
                                                                 w["tris_per_point"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
