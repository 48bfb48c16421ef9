#!/usr/bin/env python3
"""RaylibAMD_GatherDevice measured: HIP-event kernel times (RaylibAMDStats.kernelMs: the trace launches and their resolves; traceKernelMs: the trace launches),
interleaved with the call it is compared with, RUNS times each after a warm-up pair; median (min .. max) and the build id.

  parity   the surface points a W x H frame of camera rays meets, SAMPLES samples each, GATHER_IRRADIANCE -- against RaylibAMD_TraceRadianceDevice on the same
           n x SAMPLES rays materialised in advance (sample-major, the directions RaylibAMD_GatherDirectionsHost gives, a stream of its own per ray; upload not
           timed).  k_radiance is the parent commit's code (tools/isa_equivalence.py), so its time here is the parent's.  The walks and the shading are
           statistically the same work -- the bounces' random numbers differ -- and both calls' ray counters are reported beside the times.
  small    64 points x 16384 samples and 1 point x 65536 samples on the Cornell box (no sun: every trip of a lane is one closest-hit query, so the lanes per
           trip are rays / waveTrips): wave trips, lanes per trip, the resolve's time (kernelMs - traceKernelMs), and RaylibAMD_TraceRadianceDevice on the
           same rays materialised.
  "resolve" is kernelMs - traceKernelMs throughout: the resolve kernels plus the clear of the ray counter in front of each trace launch and the gaps between
  the call's kernels -- the resolve's time where it is large, an upper bound on it where it is tens of microseconds.
  bytes    the ray records a 1024 x 1024 lightmap at 256 samples would need, from the record sizes (arithmetic, not a measurement).

usage: python tools/gpu_gather.py [--cases parity:cornell,parity:interior,small] [--width 1920] [--height 1080] [--samples 8] [--runs 5] [--timeout 600] [--json PATH]
cornell: the 36-triangle Cornell box; interior: the 298 k-triangle room from inside (bench.py's breakfast_interior view).  Each case is measured in a child
process under its own time limit.
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


def _session(lib, name, aspect):
    from raylib_amd import binding, scenes
    d = tempfile.mkdtemp()
    if name == "cornell":
        obj, _ = scenes.cornell(os.path.join(d, "cornell.obj"))
        return binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, aspect)
    cam = scenes.CONFIG_CAMERAS["breakfast_interior"]
    obj, _ = scenes.cornell(os.path.join(d, "room.obj"), tess=91, displace_fraction=0.2)
    return binding.SceneSession(lib, obj, cam["origin"], cam["look_at"], cam["fov"], aspect, sun=cam["sun"], sun_dir=cam["sun_dir"])


def _surface_points(lib, ses, W, H):
    """(n, 8) float32 gather points where the frame's sample-0 camera rays meet the scene: the hit's position and normal, the ray's time, the index as stream"""
    import numpy as np
    from raylib_amd import binding
    n = W * H
    ys, xs = np.mgrid[0:H, 0:W]
    uv = np.ascontiguousarray(np.stack([xs.ravel().astype(np.float32) / np.float32(W), ys.ravel().astype(np.float32) / np.float32(H)], 1), np.float32)
    cr = np.zeros((n, 7), np.float32)
    assert lib.RaylibAMD_EvalCameraRays(ses.camera, uv.ctypes.data_as(C.POINTER(C.c_float)), n, lib.RaylibAMD_GetSeed(), cr.ctypes.data_as(C.POINTER(C.c_float))) == 1
    q = np.zeros((n, 8), np.float32)
    q[:, 0:3] = cr[:, 0:3]; q[:, 3] = 1e-4; q[:, 4:7] = cr[:, 3:6]; q[:, 7] = np.finfo(np.float32).max
    hits = binding.trace_rays(lib, ses.scene, q, binding.QUERY_SURFACE)
    ok = hits["hit"] != 0
    pts = np.zeros((int(ok.sum()), 8), np.float32)
    pts[:, 0:3] = hits["p"][ok]; pts[:, 3] = cr[ok, 6]; pts[:, 4:7] = hits["n"][ok]
    pts[:, 7] = np.arange(len(pts), dtype=np.uint32).view(np.float32)
    return pts


def _materialised_rays(lib, pts, kind, samples):
    """the n x samples path rays of the gather's directions, sample-major, each on a stream of its own"""
    import numpy as np
    from raylib_amd import binding
    n = len(pts)
    rays = np.zeros((samples, n, 8), np.float32)
    for s in range(samples):
        rays[s] = pts
        rays[s, :, 4:7] = binding.gather_directions_host(lib, pts, kind, lib.RaylibAMD_GetSeed(), s)
        rays[s, :, 7] = ((np.arange(n, dtype=np.uint64) + np.uint64(s) * np.uint64(n)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
    return rays.reshape(-1, 8)


def _stats(lib):
    from raylib_amd import binding
    st = binding.Stats()
    lib.RaylibAMD_GetLastStats(C.byref(st))
    return st


def _compare(lib, ses, pts, kind, samples, runs):
    """the gather of pts x samples beside the radiance call on its materialised rays, interleaved; a row of numbers"""
    import numpy as np
    import torch
    from raylib_amd import binding
    n = len(pts)
    rays = _materialised_rays(lib, pts, kind, samples)
    dpts, drays = torch.from_numpy(pts).cuda(), torch.from_numpy(rays).cuda()
    gout = torch.empty((n, 4 if kind == binding.GATHER_IRRADIANCE else 27), dtype=torch.float32, device="cuda")
    rout = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tlo, thi = float(pts[:, 3].min()), float(pts[:, 3].max())
    gprm = binding.GatherParams(kind, 5, 1e-4, 0, samples, 0, tlo, thi)
    rprm = binding.RadianceParams(5, 1e-4, 0, 1, 2, tlo, thi)
    fp = lambda t: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_float))
    g_ms, g_trace, r_ms = [], [], []
    gst = rst = None
    for k in range(runs + 1):   # (the first pair warms both up and is dropped)
        assert lib.RaylibAMD_GatherDevice(ses.scene, C.byref(gprm), C.cast(C.c_void_p(dpts.data_ptr()), C.POINTER(binding.GatherPoint)), n, fp(gout), None) == 1
        gst = _stats(lib)
        assert lib.RaylibAMD_TraceRadianceDevice(ses.scene, C.byref(rprm), C.cast(C.c_void_p(drays.data_ptr()), C.POINTER(binding.PathRay)), len(rays), fp(rout), None) == 1
        rst = _stats(lib)
        if k:
            g_ms.append(gst.kernelMs); g_trace.append(gst.traceKernelMs); r_ms.append(rst.kernelMs)
    med = lambda v: float(np.median(v))
    finite = bool(np.isfinite(gout.cpu().numpy()).all())
    return dict(points=n, samples=samples, kind=int(kind), paths=n * samples, build=lib.RaylibAMD_BuildId().decode(), tree=gst.treeWidth,
                gather_ms=g_ms, gather_trace_ms=g_trace, gather_resolve_ms=[a - b for a, b in zip(g_ms, g_trace)], radiance_ms=r_ms,
                gather_median=med(g_ms), gather_trace_median=med(g_trace), gather_resolve_median=med([a - b for a, b in zip(g_ms, g_trace)]), radiance_median=med(r_ms),
                ratio=med(g_ms) / med(r_ms), launches=gst.traceLaunches,
                gather_rays=gst.rays, radiance_rays=rst.rays, gather_samples=gst.cameraSamples, radiance_samples=rst.cameraSamples,
                gather_trips=gst.waveTrips, radiance_trips=rst.waveTrips, gather_lanes_per_trip=gst.rays / max(1, gst.waveTrips),
                radiance_lanes_per_trip=rst.rays / max(1, rst.waveTrips), ray_bytes_not_materialised=n * samples * 32, point_bytes=n * 32, finite=finite)


def child(args):
    import torch  # noqa: F401  (before the library is loaded, so that both run on one HIP runtime: INTEGRATION.md section 3e)
    from raylib_amd import binding
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1
    lib.RaylibAMD_SetSeed(1)
    rows = []
    if args.case.startswith("parity:"):
        scene = args.case.split(":")[1]
        ses = _session(lib, scene, args.width / args.height)
        pts = _surface_points(lib, ses, args.width, args.height)
        rows.append(dict(_compare(lib, ses, pts, binding.GATHER_IRRADIANCE, args.samples, args.runs), case=args.case, scene=scene, width=args.width, height=args.height))
    else:
        ses = _session(lib, "cornell", 1.0)
        pts = _surface_points(lib, ses, 64, 64)
        pick = pts[:: max(1, len(pts) // 64)][:64].copy()
        for kind in (binding.GATHER_IRRADIANCE, binding.GATHER_SH9):
            rows.append(dict(_compare(lib, ses, pick, kind, 16384, args.runs), case="small:64x16384", scene="cornell"))
            rows.append(dict(_compare(lib, ses, pick[:1].copy(), kind, 65536, args.runs), case="small:1x65536", scene="cornell"))
    ses.close()
    for r in rows:
        print("ROW " + json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="parity:cornell,parity:interior,small")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--case")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for name in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--case", name, "--width", str(args.width), "--height", str(args.height),
               "--samples", str(args.samples), "--runs", str(args.runs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("%s: over the %d s limit; stopping" % (name, args.timeout)); break
        if r.returncode != 0:
            print("%s: exit status %d; stopping\n%s" % (name, r.returncode, r.stderr[-3000:])); break
        rows += [json.loads(l[4:]) for l in r.stdout.splitlines() if l.startswith("ROW ")]
    spread = lambda v: "%.3f (%.3f .. %.3f)" % (sorted(v)[len(v) // 2], min(v), max(v))
    for w in rows:
        print("%s, %s, build %s: %d points x %d samples, kind %d, tree %d, %d launch(es)" % (w["case"], w["scene"], w["build"], w["points"], w["samples"], w["kind"], w["tree"], w["launches"]))
        print("    gather %s ms = trace %s + resolve %s | radiance on the materialised rays %s ms | ratio %.3f" % (
            spread(w["gather_ms"]), spread(w["gather_trace_ms"]), spread(w["gather_resolve_ms"]), spread(w["radiance_ms"]), w["ratio"]))
        print("    gather: %d rays, %d wave trips, %.1f lanes per trip | radiance: %d rays, %d wave trips, %.1f lanes per trip | %d ray bytes not materialised (%d point bytes)" % (
            w["gather_rays"], w["gather_trips"], w["gather_lanes_per_trip"], w["radiance_rays"], w["radiance_trips"], w["radiance_lanes_per_trip"],
            w["ray_bytes_not_materialised"], w["point_bytes"]))
    lm = dict(points=1024 * 1024, samples=256)
    lm.update(ray_records=lm["points"] * lm["samples"], ray_bytes=lm["points"] * lm["samples"] * 32, point_bytes=lm["points"] * 32)
    print("bytes (arithmetic from the 32-byte records): a 1024 x 1024 lightmap at 256 samples is %d ray records = %.1f GiB of rays for %.0f MiB of points" % (
        lm["ray_records"], lm["ray_bytes"] / 2.0 ** 30, lm["point_bytes"] / 2.0 ** 20))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(rows=rows, lightmap_bytes=lm), f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
