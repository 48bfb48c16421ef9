#!/usr/bin/env python3
"""Standalone ray-query rates (RaylibAMD_TraceRaysDevice on device-resident rays, the library's stream, HIP-event time of the kernel) for each query kind
and tree, against RaylibAMD_ClosestHit (the test hook: host rays, its own allocations and copies; wall time).

usage: python tools/gpu_ray_query.py [--scenes cornell,room] [--width 1920] [--height 1080] [--runs 5] [--timeout 600] [--lib PATH] [--json PATH]
       python tools/gpu_ray_query.py --overhead --lib PATH [--runs 5]
Two ray sets per scene: the camera rays of a width x height pinhole view (coherent), and one cosine-distributed ray leaving each surface point those camera
rays hit (incoherent, as a diffuse bounce).  Each scene is measured in a child process under its own time limit; one table row per (scene, rays, tree, kind).
--lib: another build of the library.  --overhead: the host path of a synchronous call, the tree's library against --lib's in one process (overhead()).
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

KINDS = {0: "any", 1: "closest", 2: "surface"}
FLT_MAX = 3.4028235e38


def camera_rays(np, w, h, origin, look_at, fov):
    o = np.asarray(origin, np.float64); f = np.asarray(look_at, np.float64) - o; f /= np.linalg.norm(f)
    r = np.cross(f, (0.0, 1.0, 0.0)); r /= np.linalg.norm(r); u = np.cross(r, f)
    k = np.tan(np.radians(fov) / 2)
    ys, xs = np.mgrid[0:h, 0:w]
    px = (2 * (xs + 0.5) / w - 1) * k * w / h; py = (1 - 2 * (ys + 0.5) / h) * k
    d = f[None, None] + px[..., None] * r + py[..., None] * u
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.zeros((w * h, 8), np.float32)
    rays[:, 0:3] = o; rays[:, 3] = 1e-4; rays[:, 4:7] = d.reshape(-1, 3); rays[:, 7] = FLT_MAX
    return rays


def bounce_rays(np, surf, seed=1):
    """a cosine-distributed direction about the surface normal (facing the incoming ray) from every hit point"""
    rng = np.random.RandomState(seed)
    h = surf["hit"] == 1
    p = surf["p"][h].astype(np.float64); n = surf["n"][h].astype(np.float64)
    u1, u2 = rng.uniform(size=len(p)), rng.uniform(size=len(p))
    a = np.where(np.abs(n[:, 0:1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = np.cross(a, n); t /= np.linalg.norm(t, axis=1, keepdims=True); b = np.cross(n, t)
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    d = t * (r * np.cos(phi))[:, None] + b * (r * np.sin(phi))[:, None] + n * np.sqrt(1 - u1)[:, None]
    rays = np.zeros((len(p), 8), np.float32)
    rays[:, 0:3] = p; rays[:, 3] = 1e-3; rays[:, 4:7] = d; rays[:, 7] = FLT_MAX
    return rays


def overhead(args):
    """--overhead: what a synchronous call costs beside its kernel -- wallMs - kernelMs of its stats, in microseconds -- for CLOSEST queries of 1 ray and of
    width x height camera rays on the Cornell box, and for a CLOSEST nearest-point call on the rays' origins: the tree's library and --lib's (another build, e.g.
    the parent commit's) take turns call by call in this one process, --runs calls each after 3 warm-up calls.  Per build the median, the least and the greatest;
    the tree's median is then placed against the other build's spread."""
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
    d = tempfile.mkdtemp()
    obj, _ = scenes.cornell(os.path.join(d, "cornell.obj"))
    cam = ((0, 1, 4), (0, 1, -1), 45.0)
    builds = {}
    for name, path in (("tree", None), ("other", args.lib)):
        lib = binding.load(path) if path else binding.load()
        assert lib.Raylib_Initialize() == 1
        builds[name] = (lib, binding.SceneSession(lib, obj, cam[0], cam[1], cam[2], 1.0))
    all_rays = torch.from_numpy(camera_rays(np, args.width, args.height, *cam)).cuda()
    print("%-8s %-6s %9s %-17s %10s %10s %10s" % ("call", "build", "n", "id", "median us", "least", "greatest"))
    for n in (1, len(all_rays)):
        rays = all_rays[:n].contiguous()
        points = rays[:, :4].contiguous(); points[:, 3] = float("inf")
        out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        calls = {"rays": lambda lib, ses: lib.RaylibAMD_TraceRaysDevice(ses.scene, 1, C.c_void_p(rays.data_ptr()), n, 0.0, C.c_void_p(out.data_ptr()), None, None),
                 "nearest": lambda lib, ses: lib.RaylibAMD_NearestPointsDevice(ses.scene, 1, C.c_void_p(points.data_ptr()), n, C.c_void_p(out.data_ptr()), None)}
        for what, call in calls.items():
            us = {name: [] for name in builds}
            for k in range(args.runs + 3):
                for name, (lib, ses) in builds.items():
                    assert call(lib, ses) == 1
                    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
                    if k >= 3:
                        us[name].append((st.wallMs - st.kernelMs) * 1e3)
            for name, (lib, _) in builds.items():
                print("%-8s %-6s %9d %-17s %10.1f %10.1f %10.1f" % (what, name, n, lib.RaylibAMD_BuildId().decode(), np.median(us[name]), min(us[name]), max(us[name])))
            inside = min(us["other"]) <= np.median(us["tree"]) <= max(us["other"])
            print("%-8s n %d: the tree's median is %s the other build's spread" % (what, n, "within" if inside else "below" if np.median(us["tree"]) < min(us["other"]) else "ABOVE"))
    for _, ses in builds.values():
        ses.close()


def child(args):
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
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
    rows = []
    cam_rays = camera_rays(np, args.width, args.height, *cam)
    surf = binding.trace_rays(lib, ses.scene, cam_rays, binding.QUERY_SURFACE)
    sets = {"camera": cam_rays, "bounce": bounce_rays(np, surf)}
    for set_name, rays in sets.items():
        n = len(rays)
        dev = torch.from_numpy(rays).cuda()
        outs = {0: torch.empty(n, dtype=torch.int32, device="cuda"), 1: torch.empty((n, 4), dtype=torch.int32, device="cuda"),
                2: torch.empty((n, 11), dtype=torch.int32, device="cuda")}
        torch.cuda.synchronize()
        # the hook: host rays (6 floats), tMin 1e-4, hipMalloc / copies / hipFree per call -- wall time
        r6 = np.ascontiguousarray(np.concatenate([rays[:, 0:3], rays[:, 4:7]], axis=1))
        hook_out = np.zeros(n, dtype=np.dtype([("w", "i4", 11)]))
        import time
        ms = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            assert lib.RaylibAMD_ClosestHit(ses.scene, r6.ctypes.data_as(C.POINTER(C.c_float)), n, 1e-4, hook_out.ctypes.data) == 1
            ms.append((time.perf_counter() - t0) * 1e3)
        hook_ms = float(np.median(ms))
        rows.append(dict(scene=args.scene, rays=set_name, n=n, tree="bvh2", kind="hook", ms=hook_ms, mrays=n / hook_ms / 1e3, timing="wall"))
        for tree in ("2", "4", "8"):
            os.environ["RAYLIB_QUERY_TREE"] = tree
            rc, plan = binding.plan_ray_query(lib, ses.scene, 1)
            if str(plan["treeWidth"]) != tree:
                continue   # the scene has no such tree
            for kind in (0, 1, 2):
                ptr = C.cast(C.c_void_p(dev.data_ptr()), C.POINTER(binding.Ray))
                ks, ws = [], []
                for _ in range(args.runs + 1):
                    assert lib.RaylibAMD_TraceRaysDevice(ses.scene, kind, ptr, n, 0.0, C.c_void_p(outs[kind].data_ptr()), None, None) == 1
                    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
                    ks.append(st.kernelMs); ws.append(st.wallMs)
                k_ms, w_ms = float(np.median(ks[1:])), float(np.median(ws[1:]))
                rows.append(dict(scene=args.scene, rays=set_name, n=n, tree={"2": "bvh2", "4": "grid4", "8": "wide8"}[tree], kind=KINDS[kind], ms=k_ms, wall_ms=w_ms,
                                 mrays=n / k_ms / 1e3, nodes_per_ray=st.nodesVisited / n, tris_per_ray=st.trisTested / n, timing="kernel"))
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
    ap.add_argument("--json")
    ap.add_argument("--lib")
    ap.add_argument("--overhead", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scene")
    args = ap.parse_args()
    if args.overhead:
        if not args.lib:
            ap.error("--overhead compares the tree's library with --lib's")
        return overhead(args)
    if args.child:
        return child(args)
    rows = []
    for name in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--scene", name, "--width", str(args.width), "--height", str(args.height), "--runs", str(args.runs)]
        if args.lib:
            cmd += ["--lib", args.lib]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("%s: over the %d s limit; stopping" % (name, args.timeout)); break
        if r.returncode != 0:
            print("%s: exit status %d; stopping\n%s" % (name, r.returncode, r.stderr[-3000:])); break
        rows += json.loads([l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
    print("%-8s %-7s %9s %-6s %-8s %9s %10s %8s %8s" % ("scene", "rays", "n", "tree", "kind", "ms", "Mrays/s", "nodes", "tris"))
    for w in rows:
        print("%-8s %-7s %9d %-6s %-8s %9.3f %10.1f %8.2f %8.2f" % (w["scene"], w["rays"], w["n"], w["tree"], w["kind"], w["ms"], w["mrays"],
                                                                 w.get("nodes_per_ray", float("nan")), w.get("tris_per_ray", float("nan"))))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
