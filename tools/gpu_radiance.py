#!/usr/bin/env python3
"""RaylibAMD_TraceRadianceDevice beside Raylib_Render: a frame's own sample-0 camera rays (RaylibAMD_EvalCameraRays on the pixels' streams) traced as caller
rays, against the render of the same frame at spp = 1 on the same device, interleaved, RUNS times each; median and spread of the HIP-event kernel times.
The two must also agree bit for bit (tests/test_gpu_radiance.py checks that on small frames; here it is counted).

usage: python tools/gpu_radiance.py [--scenes cornell,interior] [--width 1920] [--height 1080] [--runs 5] [--timeout 600] [--json PATH]
cornell: the 36-triangle Cornell box; interior: the 298 k-triangle room from inside (bench.py's breakfast_interior view).  Each scene is measured in a child
process under its own time limit.  RAYLIB_QUERY_TREE=2|4 chooses the radiance kernel's tree as usual.
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


def child(args):
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1
    lib.RaylibAMD_SetSeed(1)
    d = tempfile.mkdtemp()
    W, H = args.width, args.height
    if args.scene == "cornell":
        obj, _ = scenes.cornell(os.path.join(d, "cornell.obj"))
        ses = binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, W / H)
    else:
        cam = scenes.CONFIG_CAMERAS["breakfast_interior"]
        obj, _ = scenes.cornell(os.path.join(d, "room.obj"), tess=91, displace_fraction=0.2)
        ses = binding.SceneSession(lib, obj, cam["origin"], cam["look_at"], cam["fov"], W / H, sun=cam["sun"], sun_dir=cam["sun_dir"])
    n = W * H
    ys, xs = np.mgrid[0:H, 0:W]
    uv = np.ascontiguousarray(np.stack([xs.ravel().astype(np.float32) / np.float32(W), ys.ravel().astype(np.float32) / np.float32(H)], 1), np.float32)
    cr = np.zeros((n, 7), np.float32)
    assert lib.RaylibAMD_EvalCameraRays(ses.camera, uv.ctypes.data_as(C.POINTER(C.c_float)), n, lib.RaylibAMD_GetSeed(), cr.ctypes.data_as(C.POINTER(C.c_float))) == 1
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = cr[:, 0:3]; rays[:, 3] = cr[:, 6]; rays[:, 4:7] = cr[:, 3:6]; rays[:, 7] = np.arange(n, dtype=np.uint32).view(np.float32)
    dev = torch.from_numpy(rays).cuda()
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    prm = binding.RadianceParams(5, 1e-4, 0, 1, 3, float(rays[:, 3].min()), float(rays[:, 3].max()))
    rp, op = C.cast(C.c_void_p(dev.data_ptr()), C.POINTER(binding.PathRay)), C.cast(C.c_void_p(out.data_ptr()), C.POINTER(C.c_float))
    _, plan = binding.plan_radiance(lib, ses.scene)
    rad, ren, ren_trace = [], [], []
    rst = qst = None
    for k in range(args.runs + 1):   # (the first pair warms both up and is dropped)
        img = ses.render(W, H, 1)
        rst = ses.stats()
        assert lib.RaylibAMD_TraceRadianceDevice(ses.scene, C.byref(prm), rp, n, op, None) == 1
        qst = ses.stats()
        if k:
            ren.append(rst.kernelMs); ren_trace.append(rst.traceKernelMs); rad.append(qst.kernelMs)
    got = out.cpu().numpy()
    differ = int((got.view(np.uint32) != img.reshape(-1, 4).view(np.uint32)).any(-1).sum())
    row = dict(scene=args.scene, width=W, height=H, rays=n, build=lib.RaylibAMD_BuildId().decode(), radiance_tree=plan["treeWidth"], radiance_stack=plan["stack"],
               radiance_ms=rad, render_ms=ren, render_trace_ms=ren_trace,
               radiance_median=float(np.median(rad)), render_median=float(np.median(ren)), render_trace_median=float(np.median(ren_trace)),
               ratio=float(np.median(rad) / np.median(ren)),
               render_tree=rst.treeWidth, render_paths_per_wave=rst.pathsPerWave, render_culled_samples=rst.culledSamples,
               radiance_rays=qst.rays, radiance_nodes_per_ray=qst.nodesVisited / max(1, qst.rays), radiance_tris_per_ray=qst.trisTested / max(1, qst.rays),
               radiance_trips=qst.waveTrips, render_rays=rst.rays, render_nodes_per_ray=rst.nodesVisited / max(1, rst.rays), pixels_differing=differ)
    ses.close()
    print("ROW " + json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,interior")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scene")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for name in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--scene", name, "--width", str(args.width), "--height", str(args.height), "--runs", str(args.runs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("%s: over the %d s limit; stopping" % (name, args.timeout)); break
        if r.returncode != 0:
            print("%s: exit status %d; stopping\n%s" % (name, r.returncode, r.stderr[-3000:])); break
        rows.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("ROW ")][-1][4:]))
    for w in rows:
        spread = lambda v: "%.3f (%.3f .. %.3f)" % (sorted(v)[len(v) // 2], min(v), max(v))
        print("%s %dx%d, build %s: radiance (tree %d) %s ms | render %s ms (megakernel %s; tree %d, %d paths per wave, %d samples culled) | ratio %.2f | %d pixels differ" % (
            w["scene"], w["width"], w["height"], w["build"], w["radiance_tree"], spread(w["radiance_ms"]), spread(w["render_ms"]), spread(w["render_trace_ms"]),
            w["render_tree"], w["render_paths_per_wave"], w["render_culled_samples"], w["ratio"], w["pixels_differing"]))
        print("    radiance: %d rays, %.2f node records and %.2f triangles per ray, %d wave trips | render: %d rays executed, %.2f node records per ray" % (
            w["radiance_rays"], w["radiance_nodes_per_ray"], w["radiance_tris_per_ray"], w["radiance_trips"], w["render_rays"], w["render_nodes_per_ray"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
