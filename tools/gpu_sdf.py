#!/usr/bin/env python3
"""Distance-field bake times (RaylibAMD_BakeDistanceFieldDevice) against what a caller composes from the query entries.

usage: python tools/gpu_sdf.py [--scenes torus,room] [--dim 128] [--runs 5] [--timeout 900] [--lib PATH] [--json PATH]
Per scene, in one child process, warm, the two sides alternating in every round, the median (and the least and the greatest) of --runs rounds:
  (a) RaylibAMD_BakeDistanceFieldDevice on a dim^3 grid over 1.3 x the scene's bounds, device tensors out, the library's stream: SIGN_X and SIGN_MAJORITY with
      maxDist +inf on the torus (tests/sdf_cases.py, 800 triangles); UNSIGNED with a band of 4 voxels on the 298 k-triangle room of the bench.
  (b) the composition: RaylibAMD_NearestPointsDevice CLOSEST on the materialised centres (16 bytes a point in, 16 out), and for a signed field
      RaylibAMD_TraceRaysAllDevice with maxHits 1 and the count on one +x ray per voxel (32 bytes a ray in, 16 + 4 out), then torch: sqrt, the band's fill and
      the parity.  The points and rays are built once, outside the timed window (a caller pays for that too: `materialise_ms`, timed once).
Both sides are timed by the host clock around calls that end in a device synchronise (`ms`); (a) also carries the HIP-event time of its kernels (`kernel_ms`)
and the records visited per voxel.  `ratio` = (b) / (a) on `ms`.  The magnitudes of (a) and (b) are compared bit for bit (`same_magnitudes`).  Every row
carries the library's build id."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("RAYLIB_QUIET", "1")

FLT_MAX = 3.4028234663852886e38


def child(args):
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
    import sdf_cases as sc
    lib = binding.load(args.lib) if args.lib else binding.load()
    assert lib.Raylib_Initialize() == 1
    d = tempfile.mkdtemp()
    if args.scene == "torus":
        obj = sc.write_mesh(os.path.join(d, "torus.obj"), "torus")
        modes, band_voxels = [("sign_x", sc.SIGN_X), ("majority", sc.MAJORITY)], None
    else:   # the tessellated room of the bench (298 k triangles)
        obj, _ = scenes.cornell(os.path.join(d, "room.obj"), tess=91, displace_fraction=0.2)
        modes, band_voxels = [("unsigned", sc.UNSIGNED)], 4.0
    ses = sc.session(lib, obj)
    tris, _ = ses.export_flat()
    lo = np.minimum(np.minimum(tris["v0"].min(0), tris["v1"].min(0)), tris["v2"].min(0)).astype(np.float64)
    hi = np.maximum(np.maximum(tris["v0"].max(0), tris["v1"].max(0)), tris["v2"].max(0)).astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.3
    dims = (args.dim, args.dim, args.dim)
    spacing = (2 * half / args.dim).astype(np.float32)
    origin = (mid - half + np.asarray(sc.IRRATIONAL) * spacing).astype(np.float32)
    max_dist = float("inf") if band_voxels is None else band_voxels * float(spacing.max())
    n = args.dim ** 3
    sync = torch.cuda.synchronize

    # ---- (b)'s inputs, materialised once ----
    t0 = time.perf_counter()
    cen = torch.from_numpy(sc.centres(origin, spacing, dims).reshape(-1, 3)).cuda()
    pts = torch.cat([cen, torch.full((n, 1), max_dist, dtype=torch.float32, device="cuda")], 1).contiguous()
    rays = None
    if band_voxels is None:
        rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        rays[:, 0:3] = cen; rays[:, 4] = 1.0; rays[:, 7] = FLT_MAX
    sync()
    materialise_ms = (time.perf_counter() - t0) * 1e3
    near = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    hits = torch.empty((n, 4), dtype=torch.int32, device="cuda") if rays is not None else None
    counts = torch.empty(n, dtype=torch.int32, device="cuda") if rays is not None else None
    dist = torch.empty(n, dtype=torch.float32, device="cuda")
    sync()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def bake(sign):
        p = binding.distance_field_params(origin, spacing, dims, max_dist, sign)
        t = time.perf_counter()
        assert lib.RaylibAMD_BakeDistanceFieldDevice(ses.scene, C.byref(p), ptr(dist), None, None) == 1   # (synchronous: the library's stream)
        ms = (time.perf_counter() - t) * 1e3
        st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
        return ms, st

    def composed(signed):
        sync()
        t = time.perf_counter()
        assert lib.RaylibAMD_NearestPointsDevice(ses.scene, 1, ptr(pts), n, ptr(near), None) == 1
        if signed:
            assert lib.RaylibAMD_TraceRaysAllDevice(ses.scene, C.cast(ptr(rays), C.POINTER(binding.Ray)), n, 0.0, 1, C.cast(ptr(hits), C.POINTER(binding.HitT)),
                                                    C.cast(ptr(counts), C.POINTER(C.c_uint32)), None) == 1
        m = torch.where(near[:, 1] >= 0, torch.sqrt(near[:, 0].view(torch.float32)), torch.full_like(dist, max_dist))
        out = torch.where((counts & 1) == 1, -m, m) if signed else m
        sync()
        return (time.perf_counter() - t) * 1e3, out

    rows = []
    for mode, sign in modes:
        a, ak, b = [], [], []
        st = None
        for r in range(args.runs + 1):   # the first round is the warm-up
            ms, st = bake(sign)
            a.append(ms); ak.append(st.kernelMs)
            ms, out = composed(sign != sc.UNSIGNED)
            b.append(ms)
        bake(sign)
        same = bool(torch.equal(dist.abs().view(torch.int32), out.abs().view(torch.int32)))
        med = lambda v: float(np.median(v[1:]))
        rc, pn, pr = binding.plan_distance_field(lib, ses.scene, origin, spacing, dims, max_dist, sign)
        rows.append(dict(scene=args.scene, triangles=int(len(tris)), dims=list(dims), mode=mode, max_dist=("inf" if band_voxels is None else max_dist),
                         ms=med(a), ms_min=float(min(a[1:])), ms_max=float(max(a[1:])), kernel_ms=med(ak), kernel_ms_min=float(min(ak[1:])), kernel_ms_max=float(max(ak[1:])),
                         mvoxels_per_s=n / med(a) / 1e3, row_rays=int(st.rays - n), nodes_per_voxel=st.nodesVisited / n, tris_per_voxel=st.trisTested / n,
                         dist_tree=pn["treeWidth"], rows_tree=pr["treeWidth"] if sign != sc.UNSIGNED else None,
                         composed_ms=med(b), composed_ms_min=float(min(b[1:])), composed_ms_max=float(max(b[1:])), materialise_ms=materialise_ms,
                         ratio=med(b) / med(a), same_magnitudes=same, runs=args.runs, build=lib.RaylibAMD_BuildId().decode()))
    ses.close()
    print("ROWS " + json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="torus,room")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--lib")
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scene")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for name in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--scene", name, "--dim", str(args.dim), "--runs", str(args.runs)]
        if args.lib:
            cmd += ["--lib", args.lib]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("%s: over the %d s limit; stopping" % (name, args.timeout)); return 1
        if r.returncode != 0:
            print("%s: exit status %d; stopping\n%s" % (name, r.returncode, r.stderr[-3000:])); return 1
        rows += json.loads([l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
    print("%-6s %-9s %9s %9s %9s %9s %10s %8s %8s | %9s %9s %9s %7s %5s" % ("scene", "mode", "ms", "min", "max", "kernel", "Mvoxels/s", "nodes", "tris", "composed", "min", "max",
                                                                        "ratio", "same"))
    for w in rows:
        print("%-6s %-9s %9.3f %9.3f %9.3f %9.3f %10.1f %8.2f %8.2f | %9.3f %9.3f %9.3f %7.2f %5s" % (
            w["scene"], w["mode"], w["ms"], w["ms_min"], w["ms_max"], w["kernel_ms"], w["mvoxels_per_s"], w["nodes_per_voxel"], w["tris_per_voxel"], w["composed_ms"],
            w["composed_ms_min"], w["composed_ms_max"], w["ratio"], "yes" if w["same_magnitudes"] else "NO"))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
