#!/usr/bin/env python3
"""What the primary-hit G-buffer costs beside the calls it replaces (include/raylib_amd.h statements G1 to G6), in one process on one build.

usage: python tools/gpu_gbuffer.py [--width 1920] [--height 1080] [--runs 5] [--tess 91] [--lib PATH] [--log PATH]
The scene is the bench's 298 116-triangle room (raylib_amd/scenes.py cornell, tess 91, a fifth of the triangles displaced) from the bench's interior camera.
After one warm-up each, --runs rounds in which the four sequences alternate:
  (a) RaylibAMD_RenderGuides into two images (albedo + micro normal): one launch
  (b) the two Raylib_Render AOV calls it replaces
  (c) all seven planes through RaylibAMD_RenderGBufferDevice on the library's stream
  (d) the five Raylib_Render AOV calls + RaylibAMD_TraceRaysDevice(SURFACE, with primitives) on uploaded camera rays (the upload is not timed)
Per sequence the median, least and greatest of: the host clock around the calls, each of which ends in a synchronise, and the sum of the calls' HIP-event
kernel times from RaylibAMD_GetLastStats; then rays, node records and triangle tests per pixel of each, and the tree walked.  The planes of (a) and (c) are
checked against (b) and (d) bit for bit before anything is timed.  --log: the raw runs as JSON lines, with the library's build id.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
os.environ.setdefault("RAYLIB_QUIET", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tess", type=int, default=91)
    ap.add_argument("--lib")
    ap.add_argument("--log")
    args = ap.parse_args()
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
    lib = binding.load(args.lib) if args.lib else binding.load()
    assert lib.Raylib_Initialize() == 1, "no HIP device"
    lib.RaylibAMD_SetSeed(1)
    w, h, tmin = args.width, args.height, 1e-4
    cam = scenes.CONFIG_CAMERAS["breakfast_interior"]
    obj, ntri = scenes.cornell(os.path.join(tempfile.mkdtemp(), "room.obj"), tess=args.tess, displace_fraction=0.2)
    ses = binding.SceneSession(lib, obj, cam["origin"], cam["look_at"], cam["fov"], w / h, sun=cam["sun"], sun_dir=cam["sun_dir"])
    build = lib.RaylibAMD_BuildId().decode()
    modes = {"albedo": binding.RENDERMODE_ALBEDO, "surfaceNormal": binding.RENDERMODE_SURFACE_NORMAL, "microNormal": binding.RENDERMODE_MICROSURFACE_NORMAL,
             "texcoord": binding.RENDERMODE_TEXCOORD, "emission": binding.RENDERMODE_EMISSION}
    images = {k: lib.Raylib_CreateImage(w, h) for k in modes}
    guides = {k: lib.Raylib_CreateImage(w, h) for k in ("albedo", "microNormal")}
    planes = {k: torch.empty((h, w, 11 if k == "surface" else 4), dtype=torch.int32 if k in ("hit", "surface") else torch.float32, device="cuda") for k in binding.GBUFFER_PLANES}
    P = binding.GBufferPlanes(**{k: v.data_ptr() for k, v in planes.items()})
    st1 = ses.settings(w, h, 1, 5, tmin)
    # (d)'s rays: what RaylibAMD_EvalCameraRays gives for the frame's pixels, on the device before the clock starts
    ys, xs = np.mgrid[0:h, 0:w]
    uv = np.stack([np.float32(xs.ravel()) / np.float32(w), np.float32(ys.ravel()) / np.float32(h)], 1).astype(np.float32)
    cr = np.zeros((w * h, 7), np.float32)
    assert lib.RaylibAMD_EvalCameraRays(ses.camera, uv.ctypes.data_as(C.POINTER(C.c_float)), w * h, 1, cr.ctypes.data_as(C.POINTER(C.c_float))) == 1
    rays = np.zeros((w * h, 8), np.float32)
    rays[:, 0:3] = cr[:, 0:3]; rays[:, 3] = tmin; rays[:, 4:7] = cr[:, 3:6]; rays[:, 7] = np.finfo(np.float32).max
    d_rays = torch.from_numpy(rays).cuda()
    d_surf = torch.empty((w * h, 11), dtype=torch.int32, device="cuda")
    d_prim = torch.empty(w * h, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def stats():
        s = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(s))
        return s

    def render(mode, img):
        st = ses.settings(w, h, 1, 5, tmin, mode)
        lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, img)
        return stats()

    def seq_a():
        assert lib.RaylibAMD_RenderGuides(C.byref(st1), ses.scene, ses.camera, guides["albedo"], guides["microNormal"]) == 1
        return [stats()]

    def seq_b():
        return [render(modes[k], images[k]) for k in ("albedo", "microNormal")]

    def seq_c():
        assert lib.RaylibAMD_RenderGBufferDevice(C.byref(st1), ses.scene, ses.camera, C.byref(P), None) == 1
        return [stats()]

    def seq_d():
        out = [render(modes[k], images[k]) for k in modes]
        assert lib.RaylibAMD_TraceRaysDevice(ses.scene, binding.QUERY_SURFACE, C.c_void_p(d_rays.data_ptr()), w * h, 0.0, C.c_void_p(d_surf.data_ptr()), C.c_void_p(d_prim.data_ptr()), None) == 1
        return out + [stats()]

    seqs = {"a": seq_a, "b": seq_b, "c": seq_c, "d": seq_d}
    for f in seqs.values():      # the warm-up: uploads, trees, tables, code objects, buffers
        f()

    def dump(img):
        out = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, out.ctypes.data_as(C.POINTER(C.c_float)))
        return out
    for k in modes:
        assert planes[k].cpu().numpy().tobytes() == dump(images[k]).tobytes(), "plane %s differs from its AOV render" % k
    for k in guides:
        assert dump(guides[k]).tobytes() == dump(images[k]).tobytes(), "guide %s differs from its AOV render" % k
    assert planes["surface"].cpu().numpy().tobytes() == d_surf.cpu().numpy().tobytes(), "the surface plane differs from the SURFACE query"
    assert np.array_equal(planes["hit"].cpu().numpy()[..., 1].reshape(-1), d_prim.cpu().numpy()), "the hit plane's primitives differ from the SURFACE query's"

    raw = []
    for r in range(args.runs):
        for name, f in seqs.items():
            t0 = time.perf_counter()
            ss = f()
            wall = (time.perf_counter() - t0) * 1e3
            raw.append(dict(run=r, seq=name, wall_ms=wall, kernel_ms=sum(s.kernelMs for s in ss), calls=len(ss), rays=sum(s.rays for s in ss),
                            nodes=sum(s.nodesVisited for s in ss), tris=sum(s.trisTested for s in ss), tree_width=[s.treeWidth for s in ss], node_bytes=[s.nodeBytes for s in ss]))
    what = {"a": "RenderGuides (albedo + micro normal)", "b": "2 AOV Raylib_Render", "c": "7 planes, RenderGBufferDevice", "d": "5 AOV Raylib_Render + TraceRays(SURFACE)"}
    print("room of %d triangles from inside, %d x %d, build %s, median of %d (least .. greatest), the sequences alternating" % (ntri, w, h, build, args.runs))
    print("%-3s %-42s %5s %27s %27s %9s %9s %9s  %s" % ("", "sequence", "calls", "wall ms", "kernel ms", "rays/px", "nodes/px", "tris/px", "trees"))
    for name in seqs:
        rows = [x for x in raw if x["seq"] == name]
        col = lambda k: "%8.3f (%7.3f .. %7.3f)" % (float(np.median([x[k] for x in rows])), min(x[k] for x in rows), max(x[k] for x in rows))
        x = rows[-1]
        print("(%s) %-42s %5d %27s %27s %9.3f %9.2f %9.2f  %s" % (name, what[name], x["calls"], col("wall_ms"), col("kernel_ms"), x["rays"] / (w * h), x["nodes"] / (w * h),
                                                                 x["tris"] / (w * h), x["tree_width"]))
    if args.log:
        with open(args.log, "w") as f:
            f.write(json.dumps(dict(scene="cornell tess %d, displace 0.2" % args.tess, triangles=ntri, camera="breakfast_interior", width=w, height=h, build=build, runs=args.runs)) + "\n")
            for x in raw:
                f.write(json.dumps(x) + "\n")
    for img in list(images.values()) + list(guides.values()):
        lib.Raylib_DestroyImage(img)
    ses.close()


if __name__ == "__main__":
    sys.exit(main())
