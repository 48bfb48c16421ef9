#!/usr/bin/env python3
"""Standalone oriented-box query times (RaylibAMD_OverlapBoxesDevice on device-resident queries, the library's stream, HIP-event time of the kernel) on the
298 k-triangle room, for each box size, orientation, kind and tree.

usage: python tools/gpu_boxes.py [--sizes 0.005:1048576,0.05:1048576,0.5:16384] [--runs 5] [--max-hits 16] [--timeout 900] [--lib PATH] [--json PATH]
--sizes: half extent as a fraction of the scene's extent, and how many boxes of that size a call holds.  The boxes sit about uniform points of the scene's
bounds; every half extent of a box is the size times a factor from 0.5 to 1 per axis.  Each set is measured axis-aligned and under random rotations, as ANY,
LIST (--max-hits) and MARK, on both trees (RAYLIB_QUERY_TREE), which take turns call by call.  After one warm-up call: the median, least and greatest kernel
time of --runs calls, node records and triangle records per query, the share of queries that meet a triangle.  (MARK's time includes the clear of its mask.)
For scale, RaylibAMD_OverlapTrianglesDevice ANY / LIST on the same scene with two query triangles per axis-aligned box, which span the rectangle through two
of its opposite edges: what a caller without box queries could ask -- it misses everything strictly inside the box.  The measurement runs in a child process
under --timeout."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
os.environ.setdefault("RAYLIB_QUIET", "1")

KINDS = {0: "any", 1: "list", 2: "mark"}


def child(args):
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
    lib = binding.load(args.lib) if args.lib else binding.load()
    assert lib.Raylib_Initialize() == 1
    d = tempfile.mkdtemp()
    obj, _ = scenes.cornell(os.path.join(d, "room.obj"), tess=91, displace_fraction=0.2)   # the tessellated room of the bench (298 k triangles)
    ses = binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    tris, _ = ses.export_flat()
    P = np.concatenate([tris["v0"], tris["v1"], tris["v2"]]).astype(np.float64)
    lo, hi = P.min(0), P.max(0)
    extent = float((hi - lo).max())
    m = len(tris)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    plans = {}
    for tree in ("2", "4"):
        os.environ["RAYLIB_QUERY_TREE"] = tree
        rc, plan = binding.plan_overlap_boxes(lib, ses.scene, 1)
        if str(plan["treeWidth"]) == tree:
            plans[tree] = plan
    rows = []

    def measure(calls, n, label):
        """calls: {kind name: (function of no arguments, the tensor that says which queries met)}; the trees take turns run by run."""
        for kind, (call, met_of) in calls.items():
            ks, last = {t: [] for t in plans}, {}
            for _ in range(args.runs + 1):
                for tree in plans:
                    os.environ["RAYLIB_QUERY_TREE"] = tree
                    assert call() == 1
                    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
                    ks[tree].append(st.kernelMs); last[tree] = (st.nodesVisited, st.trisTested)
            met = met_of()
            for tree in plans:
                kk = ks[tree][1:]
                rows.append(dict(label, n=n, tree={"2": "bvh2", "4": "grid4"}[tree], stack=plans[tree]["stack"], kind=kind, ms=float(np.median(kk)), ms_min=float(min(kk)),
                                 ms_max=float(max(kk)), nodes_per_query=last[tree][0] / n, tris_per_query=last[tree][1] / n, share_meeting=met))
                print("ROW " + json.dumps(rows[-1]), flush=True)

    for spec in args.sizes.split(","):
        size, n = float(spec.split(":")[0]), int(spec.split(":")[1])
        rng = np.random.RandomState(1)
        centre = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
        half = (size * extent * rng.uniform(0.5, 1.0, (n, 3))).astype(np.float32)
        R = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0].astype(np.float32)
        for orient, axes in (("aligned", None), ("rotated", R)):
            q = binding.box_queries(centre, half, axes)
            dev = torch.from_numpy(q.view(np.float32).reshape(n, 16)).cuda()
            hit = torch.empty(n, dtype=torch.int32, device="cuda")
            lst = torch.empty((n, args.max_hits), dtype=torch.int32, device="cuda")
            cnt = torch.empty(n, dtype=torch.int32, device="cuda")
            mask = torch.empty((m + 31) // 32, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            f = lib.RaylibAMD_OverlapBoxesDevice
            calls = {"any": (lambda: f(ses.scene, 0, ptr(dev), n, 0, ptr(hit), None, None), lambda: float((hit != 0).float().mean())),
                     "list": (lambda: f(ses.scene, 1, ptr(dev), n, args.max_hits, ptr(lst), ptr(cnt), None), lambda: float((cnt > 0).float().mean())),
                     "mark": (lambda: f(ses.scene, 2, ptr(dev), n, 0, ptr(mask), None, None), lambda: float("nan"))}
            measure(calls, n, dict(query="box", size=size, orient=orient))
        # for scale: two triangles per axis-aligned box, the rectangle through two opposite edges
        c, h = centre.astype(np.float64), half.astype(np.float64)
        A, B, Cc, D = c + h * (-1, -1, -1), c + h * (1, -1, -1), c + h * (1, 1, 1), c + h * (-1, 1, 1)
        Q = np.concatenate([np.stack([A, B, Cc], 1), np.stack([A, Cc, D], 1)]).astype(np.float32)
        tq = binding.overlap_queries(Q[:, 0], Q[:, 1], Q[:, 2])
        n2 = len(tq)
        dev = torch.from_numpy(tq.view(np.float32).reshape(n2, 12)).cuda()
        hit = torch.empty(n2, dtype=torch.int32, device="cuda")
        lst = torch.empty((n2, args.max_hits), dtype=torch.int32, device="cuda")
        cnt = torch.empty(n2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = lib.RaylibAMD_OverlapTrianglesDevice
        calls = {"any": (lambda: g(ses.scene, 0, 0, ptr(dev), n2, 0, ptr(hit), None, None), lambda: float((hit != 0).float().mean())),
                 "list": (lambda: g(ses.scene, 1, 0, ptr(dev), n2, args.max_hits, ptr(lst), ptr(cnt), None), lambda: float((cnt > 0).float().mean()))}
        measure(calls, n2, dict(query="2 tris", size=size, orient="aligned"))
    os.environ.pop("RAYLIB_QUERY_TREE", None)
    ses.close()
    print("DONE %d triangles, extent %.3f" % (m, extent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="0.005:1048576,0.05:1048576,0.5:16384")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-hits", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--lib")
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--sizes", args.sizes, "--runs", str(args.runs), "--max-hits", str(args.max_hits)]
    if args.lib:
        cmd += ["--lib", args.lib]
    out, status = "", ""
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        out = r.stdout
        if r.returncode != 0:
            status = "exit status %d\n%s" % (r.returncode, r.stderr[-3000:])
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        status = "over the %d s limit: the rows so far" % args.timeout
    rows = [json.loads(l[4:]) for l in out.splitlines() if l.startswith("ROW ")]
    print("# 298 k-triangle room; kernel ms: median [least .. greatest] of %d calls after a warm-up; nodes, tris: records per query; the trees take turns call by call" % args.runs)
    print("%-7s %6s %-8s %8s %-6s %5s %-5s %9s  %-19s %9s %10s %8s" % ("query", "size", "orient", "n", "tree", "stack", "kind", "ms", "[least .. greatest]", "nodes", "tris", "meeting"))
    for w in rows:
        print("%-7s %6.3f %-8s %8d %-6s %5d %-5s %9.3f  [%8.3f .. %8.3f] %8.2f %10.2f %8.3f" % (w["query"], w["size"], w["orient"], w["n"], w["tree"], w["stack"], w["kind"], w["ms"],
                                                                                           w["ms_min"], w["ms_max"], w["nodes_per_query"], w["tris_per_query"], w["share_meeting"]))
    if status:
        print(status)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if rows and not status else 1


if __name__ == "__main__":
    sys.exit(main())
