#!/usr/bin/env python3
"""Standalone triangle-overlap query rates (RaylibAMD_OverlapTrianglesDevice on device-resident queries, the library's stream, HIP-event time of the kernel) for
each kind and tree.

usage: python tools/gpu_overlap.py [--scenes cornell,room] [--runs 5] [--max-hits 4] [--min-queries 1048576] [--timeout 600] [--lib PATH] [--json PATH] [--contacts]
Two query sets per scene: the scene's own triangles with RAYLIB_AMD_OVERLAP_SKIP_SHARED -- the self-intersection pass; a scene of fewer than --min-queries
triangles has them repeated -- and as many random triangles of the
median triangle's size about uniform points of the scene's bounds, without the flag.  After one warm-up call, the median of --runs calls, the two trees taking turns call by call.  Each scene is
measured in a child process under its own time limit; one table row per (scene, query set, tree, kind): queries per second, node records and triangle records
per query, and the share of queries that meet a triangle.  --lib: another build of the library.
--contacts: RaylibAMD_OverlapContactsDevice beside LIST (ANY is left out) on the same scenes and queries, the two calls taking turns run by run as the trees do;
the table gains a column, the call's time over LIST's.  LIST's own time, against the commit before the contacts, is the yardstick: the contacts instances are
kernels of their own and must leave it alone.
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
os.environ.setdefault("RAYLIB_QUIET", "1")

KINDS = {0: "any", 1: "list", 2: "contacts"}   # 2: RaylibAMD_OverlapContactsDevice (--contacts)


def child(args):
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
    lib = binding.load(args.lib) if args.lib else binding.load()
    assert lib.Raylib_Initialize() == 1
    d = tempfile.mkdtemp()
    if args.scene == "cornell":
        obj, _ = scenes.cornell(os.path.join(d, "cornell.obj"))
    else:   # the tessellated room of the bench (298 k triangles)
        obj, _ = scenes.cornell(os.path.join(d, "room.obj"), tess=91, displace_fraction=0.2)
    ses = binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    tris, _ = ses.export_flat()
    T = np.stack([tris["v0"], tris["v1"], tris["v2"]], 1).astype(np.float32)
    lo, hi = T.reshape(-1, 3).min(0), T.reshape(-1, 3).max(0)
    size = float(np.median((T.max(1) - T.min(1)).max(1)))
    T = np.tile(T, (-(-args.min_queries // len(T)), 1, 1))   # a small scene's triangles again and again, until a launch fills the device
    n = len(T)
    rng = np.random.RandomState(1)
    rand = (rng.uniform(lo, hi, (n, 3))[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 3)) * size).astype(np.float32)
    rows = []
    for set_name, Q, flags in (("self", T, binding.OVERLAP_SKIP_SHARED), ("random", rand, 0)):
        q = binding.overlap_queries(Q[:, 0], Q[:, 1], Q[:, 2])
        dev = torch.from_numpy(q.view(np.float32).reshape(n, 12)).cuda()
        outs = {0: torch.empty(n, dtype=torch.int32, device="cuda"), 1: torch.empty((n, args.max_hits), dtype=torch.int32, device="cuda")}
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        if args.contacts:
            outs[2] = outs[1]
            rec = torch.empty((n, args.max_hits, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        plans = {}
        for tree in ("2", "4"):
            os.environ["RAYLIB_QUERY_TREE"] = tree
            rc, plan = binding.plan_overlap(lib, ses.scene, 1)
            if str(plan["treeWidth"]) == tree:   # (else the scene has no such tree)
                plans[tree] = plan
        def call(kind):
            if kind == 2:
                return lib.RaylibAMD_OverlapContactsDevice(ses.scene, flags, C.c_void_p(dev.data_ptr()), n, args.max_hits, C.c_void_p(outs[2].data_ptr()), C.c_void_p(rec.data_ptr()),
                                                           C.c_void_p(cnt.data_ptr()), None)
            return lib.RaylibAMD_OverlapTrianglesDevice(ses.scene, kind, flags, C.c_void_p(dev.data_ptr()), n, args.max_hits, C.c_void_p(outs[kind].data_ptr()),
                                                        C.c_void_p(cnt.data_ptr()) if kind == 1 else None, None)

        # --contacts: LIST and the contacts call take turns too (one group); else each kind is measured by itself
        for group in (((1, 2),) if args.contacts else ((0,), (1,))):
            # the trees take turns, run by run, so that whatever else the machine does meets both alike
            ks, ws, last = {(t, k): [] for t in plans for k in group}, {(t, k): [] for t in plans for k in group}, {}
            for _ in range(args.runs + 1):
                for tree in plans:
                    os.environ["RAYLIB_QUERY_TREE"] = tree
                    for kind in group:
                        assert call(kind) == 1
                        st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
                        ks[(tree, kind)].append(st.kernelMs); ws[(tree, kind)].append(st.wallMs); last[(tree, kind)] = (st.nodesVisited, st.trisTested)
            met = float((outs[0] != 0).float().mean()) if group == (0,) else float((cnt > 0).float().mean())
            for (tree, kind) in ks:
                plan = plans[tree]
                kk, ww, ll = ks[(tree, kind)], ws[(tree, kind)], last[(tree, kind)]
                k_ms, w_ms = float(np.median(kk[1:])), float(np.median(ww[1:]))
                rows.append(dict(scene=args.scene, queries=set_name, n=n, tree={"2": "bvh2", "4": "grid4"}[tree], kind=KINDS[kind], max_hits=args.max_hits if kind >= 1 else 0,
                                 stack=plan["stack"], ms=k_ms, ms_min=float(min(kk[1:])), ms_max=float(max(kk[1:])), wall_ms=w_ms, mqueries=n / k_ms / 1e3,
                                 nodes_per_query=ll[0] / n, tris_per_query=ll[1] / n, share_meeting=met, timing="kernel"))
        os.environ.pop("RAYLIB_QUERY_TREE", None)
    ses.close()
    print("ROWS " + json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,room")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-hits", type=int, default=4)
    ap.add_argument("--min-queries", type=int, default=1 << 20)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--lib")
    ap.add_argument("--json")
    ap.add_argument("--contacts", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scene")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for name in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--scene", name, "--runs", str(args.runs), "--max-hits", str(args.max_hits), "--min-queries", str(args.min_queries)]
        if args.lib:
            cmd += ["--lib", args.lib]
        if args.contacts:
            cmd += ["--contacts"]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("%s: over the %d s limit; stopping" % (name, args.timeout)); break
        if r.returncode != 0:
            print("%s: exit status %d; stopping\n%s" % (name, r.returncode, r.stderr[-3000:])); break
        rows += json.loads([l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
    list_ms = {(w["scene"], w["queries"], w["tree"]): w["ms"] for w in rows if w["kind"] == "list"}
    print("%-8s %-8s %9s %-6s %-8s %9s %11s %8s %8s %8s%s" % ("scene", "queries", "n", "tree", "kind", "ms", "Mqueries/s", "nodes", "tris", "meeting", "  x list" if args.contacts else ""))
    for w in rows:
        print("%-8s %-8s %9d %-6s %-8s %9.3f %11.1f %8.2f %8.2f %8.3f%s" % (w["scene"], w["queries"], w["n"], w["tree"], w["kind"], w["ms"], w["mqueries"], w["nodes_per_query"],
                                                                         w["tris_per_query"], w["share_meeting"],
                                                                         "  %6.3f" % (w["ms"] / list_ms[(w["scene"], w["queries"], w["tree"])]) if args.contacts else ""))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if rows else 1


if __name__ == "__main__":
    sys.exit(main())
