#!/usr/bin/env python3
"""Ordered multi-hit query rates (RaylibAMD_TraceRaysAllDevice on device-resident rays, the library's stream, HIP-event time of the kernel) against what a caller
does without it: peeling, maxHits successive CLOSEST launches (RaylibAMD_TraceRaysDevice) with tMin = nextup(t_k), their summed kernel times.  k_query is the
parent commit's code (profiles/multi_hit_isa_equivalence.log), so the peel is measured on the parent's kernels.

usage: python tools/gpu_multi_hit.py [--scenes cornell,room] [--width 1920] [--height 1080] [--runs 5] [--hits 1,4,16] [--timeout 600] [--json PATH]
Two ray sets per scene, as tools/gpu_ray_query.py: a pinhole view's camera rays, and one cosine-distributed ray from each surface point those hit.  Per
(scene, rays, tree, maxHits, count): the median of `runs` kernel times after a warm-up, the peel's median of `runs` sums, their ratio, and node records and
triangles per ray of both.  Between the peel's launches the next tMin is written on the device by torch (not timed; a ray that has run out gets tMin = +inf and
costs the root's test).  maxHits == 1 against CLOSEST itself is the price of the list.  Each scene is measured in a child process under its own time limit."""
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


def child(args):
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
    from gpu_ray_query import camera_rays, bounce_rays
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1
    d = tempfile.mkdtemp()
    if args.scene == "cornell":
        obj, _ = scenes.cornell(os.path.join(d, "cornell.obj"))
        cam = ((0, 1, 4), (0, 1, -1), 45.0)
    else:   # the tessellated room of the bench (298 k triangles), seen from inside
        obj, _ = scenes.cornell(os.path.join(d, "room.obj"), tess=91, displace_fraction=0.2)
        cam = ((0, 1, 0.9), (0, 1, -1), 60.0)
    ses = binding.SceneSession(lib, obj, cam[0], cam[1], cam[2], 1.0)
    hits_list = [int(k) for k in args.hits.split(",")]
    rows = []
    cam_rays = camera_rays(np, args.width, args.height, *cam)
    surf = binding.trace_rays(lib, ses.scene, cam_rays, binding.QUERY_SURFACE)
    sets = {"camera": cam_rays, "bounce": bounce_rays(np, surf)}
    stats = binding.Stats()
    for set_name, rays in sets.items():
        n = len(rays)
        dev = torch.from_numpy(rays).cuda()
        work = dev.clone()
        closest = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        out = torch.empty((n, max(hits_list), 4), dtype=torch.int32, device="cuda")
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        inf_bits = torch.tensor(0x7f800000, dtype=torch.int32, device="cuda")
        ray_p = lambda t: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(binding.Ray))
        hit_p = C.cast(C.c_void_p(out.data_ptr()), C.POINTER(binding.HitT))
        cnt_p = C.cast(C.c_void_p(cnt.data_ptr()), C.POINTER(C.c_uint32))

        def closest_launch(r):
            torch.cuda.synchronize()
            assert lib.RaylibAMD_TraceRaysDevice(ses.scene, binding.QUERY_CLOSEST, ray_p(r), n, 0.0, C.c_void_p(closest.data_ptr()), None, None) == 1
            lib.RaylibAMD_GetLastStats(C.byref(stats))
            return stats.kernelMs, stats.nodesVisited, stats.trisTested

        def peel(layers):
            work.copy_(dev)
            ms = nodes = tris = 0
            for _ in range(layers):
                k, a, b = closest_launch(work)
                ms += k; nodes += a; tris += b
                # tMin = nextup(t) where the layer hit (t > 0: the next float is the next integer), +inf where the ray has run out
                nxt = torch.where(closest[:, 1] >= 0, closest[:, 0] + 1, inf_bits)
                work.view(torch.int32)[:, 3] = nxt
            return ms, nodes, tris

        for tree in ("2", "8"):
            os.environ["RAYLIB_QUERY_TREE"] = tree
            rc, plan = binding.plan_ray_query_all(lib, ses.scene, 4)
            if str(plan["treeWidth"]) != tree:
                continue   # the scene has no such tree
            name = {"2": "bvh2", "8": "wide8"}[tree]
            for k in hits_list:
                peels = [peel(k) for _ in range(args.runs + 1)][1:]
                peel_ms = float(np.median([p[0] for p in peels]))
                for count in (0, 1):
                    ks = []
                    for _ in range(args.runs + 1):
                        torch.cuda.synchronize()
                        assert lib.RaylibAMD_TraceRaysAllDevice(ses.scene, ray_p(dev), n, 0.0, k, hit_p, cnt_p if count else None, None) == 1
                        lib.RaylibAMD_GetLastStats(C.byref(stats))
                        ks.append(stats.kernelMs)
                    ms = float(np.median(ks[1:]))
                    rows.append(dict(scene=args.scene, rays=set_name, n=n, tree=name, maxHits=k, count=count, ms=ms, spread_ms=float(max(ks[1:]) - min(ks[1:])), mrays=n / ms / 1e3,
                                     nodes_per_ray=stats.nodesVisited / n, tris_per_ray=stats.trisTested / n, peel_ms=peel_ms, ratio=ms / peel_ms,
                                     peel_nodes_per_ray=peels[-1][1] / n, peel_tris_per_ray=peels[-1][2] / n, runs=args.runs))
        os.environ.pop("RAYLIB_QUERY_TREE", None)
    ses.close()
    print("ROWS " + json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,room")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--hits", default="1,4,16")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scene")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for name in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--scene", name, "--width", str(args.width), "--height", str(args.height), "--runs", str(args.runs),
               "--hits", args.hits]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("%s: over the %d s limit; stopping" % (name, args.timeout)); break
        if r.returncode != 0:
            print("%s: exit status %d; stopping\n%s" % (name, r.returncode, r.stderr[-3000:])); break
        rows += json.loads([l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
    print("%-8s %-7s %9s %-6s %4s %5s %9s %9s %6s %8s %8s %9s %9s" % ("scene", "rays", "n", "tree", "hits", "count", "ms", "peel ms", "ratio", "nodes", "tris", "peel nod.", "peel tris"))
    for w in rows:
        print("%-8s %-7s %9d %-6s %4d %5d %9.3f %9.3f %6.2f %8.2f %8.2f %9.2f %9.2f" % (w["scene"], w["rays"], w["n"], w["tree"], w["maxHits"], w["count"], w["ms"], w["peel_ms"],
                                                                                     w["ratio"], w["nodes_per_ray"], w["tris_per_ray"], w["peel_nodes_per_ray"], w["peel_tris_per_ray"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if rows else 1


if __name__ == "__main__":
    sys.exit(main())
