#!/usr/bin/env python3
"""What the motion launch and the temporal accumulation cost (include/raylib_amd.h statements T1 to T8), in one process on one build.

usage: python tools/gpu_temporal.py [--width 1920] [--height 1080] [--runs 15] [--tess 91] [--lib PATH] [--log PATH]
The scene is the bench's 298 116-triangle room (raylib_amd/scenes.py cornell, tess 91, a fifth of the triangles displaced) from the bench's interior camera; the
previous camera stands a little aside, and a third of the triangles are given previous positions a little aside.
After one warm-up each, --runs rounds in which these alternate, every one on the library's stream and timed by the HIP-event pair around its kernel
(RaylibAMD_GetLastStats kernelMs), the copies by a torch event pair around the one copy:
  (a1) RaylibAMD_RenderMotionDevice, hit + motion              the fused launch
  (a2) RaylibAMD_RenderGBufferDevice, hit alone                the baseline: the parent's kernel
  (a3) a device-to-device copy of 32 bytes per pixel           a2 + a3 is the floor of any two-pass design (a second pass reads the hit plane and writes the motion plane)
  (b1) RaylibAMD_TemporalAccumulateDevice                      k_temporal; its compulsory traffic is 104 bytes per pixel: 48 read, 36 of history read once, 20 written
  (b2) a device-to-device copy that moves the same 104 bytes per pixel (52 read, 52 written)
The planes of (a1) are checked against (a2) and against RaylibAMD_MotionHost, and (b1) against RaylibAMD_TemporalAccumulateHost, bit for bit before anything is
timed.  --log: the raw runs as JSON lines, with the library's build id.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
os.environ.setdefault("RAYLIB_QUIET", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=15)
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
    n = w * h
    cam = scenes.CONFIG_CAMERAS["breakfast_interior"]
    obj, ntri = scenes.cornell(os.path.join(tempfile.mkdtemp(), "room.obj"), tess=args.tess, displace_fraction=0.2)
    ses = binding.SceneSession(lib, obj, cam["origin"], cam["look_at"], cam["fov"], w / h, sun=cam["sun"], sun_dir=cam["sun_dir"])
    build = lib.RaylibAMD_BuildId().decode()
    o = np.asarray(cam["origin"], np.float64)
    prev = binding.create_camera(lib, o + (0.02, 0.01, 0.0), cam["look_at"], cam["fov"], w / h)
    tris = ses.export_flat()[0]
    first, count = ntri // 3, ntri // 3
    pos = np.concatenate([tris["v0"], tris["v1"], tris["v2"]], 1).astype(np.float32)[first:first + count]
    pp_host = np.ascontiguousarray(pos - np.tile(np.asarray((0.01, 0.0, 0.005), np.float32), 3))
    pp = torch.from_numpy(pp_host).cuda()
    i32 = lambda: torch.empty((h, w, 4), dtype=torch.int32, device="cuda")
    hit, motion, hit0, hist_hit = i32(), i32(), i32(), i32()
    rng = np.random.RandomState(1)
    colour = torch.from_numpy(rng.uniform(0, 2, (h, w, 4)).astype(np.float32)).cuda()
    hist_colour = torch.from_numpy(rng.uniform(0, 2, (h, w, 4)).astype(np.float32)).cuda()
    hist_len = torch.full((h, w), 3.0, dtype=torch.float32, device="cuda")
    out_c = torch.empty((h, w, 4), dtype=torch.float32, device="cuda"); out_l = torch.empty((h, w), dtype=torch.float32, device="cuda")
    src32, dst32 = torch.empty(n * 8, dtype=torch.float32, device="cuda"), torch.empty(n * 8, dtype=torch.float32, device="cuda")
    src52, dst52 = torch.empty(n * 13, dtype=torch.float32, device="cuda"), torch.empty(n * 13, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = binding.RendererSettings(w, h, 1, 1, tmin, 0)
    prm = binding.MotionParams(prev, first, count, pp.data_ptr())
    mp = binding.MotionPlanes(hit=hit.data_ptr(), motion=motion.data_ptr())
    gp = binding.GBufferPlanes(hit=hit0.data_ptr())
    tp = binding.TemporalParams(0.02, 32.0)
    frame = binding.TemporalFrame(hist_colour.data_ptr(), hist_hit.data_ptr(), hist_len.data_ptr())

    def kernel_ms():
        s = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(s))
        return s.kernelMs

    def a1():
        assert lib.RaylibAMD_RenderMotionDevice(C.byref(st), ses.scene, ses.camera, C.byref(prm), C.byref(mp), None) == 1
        return kernel_ms()

    def a2():
        assert lib.RaylibAMD_RenderGBufferDevice(C.byref(st), ses.scene, ses.camera, C.byref(gp), None) == 1
        return kernel_ms()

    def copy(dst, src):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def b1():
        assert lib.RaylibAMD_TemporalAccumulateDevice(w, h, C.byref(tp), colour.data_ptr(), hit.data_ptr(), motion.data_ptr(), C.byref(frame), out_c.data_ptr(), out_l.data_ptr(), None) == 1
        return kernel_ms()

    # the previous frame's hit plane: the walk through the previous camera (the triangles stand where they are: most taps find their surface)
    assert lib.RaylibAMD_RenderGBufferDevice(C.byref(st), ses.scene, prev, C.byref(binding.GBufferPlanes(hit=hist_hit.data_ptr())), None) == 1
    seqs = {"a1": a1, "a2": a2, "a3": lambda: copy(dst32, src32), "b1": b1, "b2": lambda: copy(dst52, src52)}
    for f in seqs.values():      # the warm-up: uploads, trees, tables, code objects, buffers
        f()
    # what is timed is right
    hit_np = hit.cpu().numpy()
    assert hit_np.tobytes() == hit0.cpu().numpy().tobytes(), "the motion launch's hit plane differs from the G-buffer's"
    ys, xs = np.mgrid[0:h, 0:w]
    uv = np.stack([np.float32(xs.ravel()) / np.float32(w), np.float32(ys.ravel()) / np.float32(h)], 1).astype(np.float32)
    cr = np.zeros((n, 7), np.float32)
    assert lib.RaylibAMD_EvalCameraRays(ses.camera, uv.ctypes.data_as(C.POINTER(C.c_float)), n, 1, cr.ctypes.data_as(C.POINTER(C.c_float))) == 1
    hit_rec = hit_np.view(binding.HITT_DTYPE).reshape(h, w)
    want_m = binding.motion_host(lib, ses.scene, ses.camera, w, h, cr, hit_rec, prev, first, pp_host)
    assert motion.cpu().numpy().tobytes() == want_m.tobytes(), "the motion plane differs from RaylibAMD_MotionHost"
    want = binding.temporal_accumulate(lib, colour.cpu().numpy(), hit_rec, want_m, (hist_colour.cpu().numpy(), hist_hit.cpu().numpy().view(binding.HITT_DTYPE).reshape(h, w),
                                       hist_len.cpu().numpy()), 0.02, 32.0, host=True)
    assert out_c.cpu().numpy().tobytes() == want[0].tobytes() and out_l.cpu().numpy().tobytes() == want[1].tobytes(), "the accumulation differs from its host oracle"
    found = float((want[1] > 1).mean())

    raw = []
    for r in range(args.runs):
        for name, f in seqs.items():
            raw.append(dict(run=r, seq=name, ms=f()))
    med = {k: float(np.median([x["ms"] for x in raw if x["seq"] == k])) for k in seqs}
    rng_ = {k: (min(x["ms"] for x in raw if x["seq"] == k), max(x["ms"] for x in raw if x["seq"] == k)) for k in seqs}
    what = {"a1": "RenderMotionDevice, hit + motion (fused)", "a2": "RenderGBufferDevice, hit alone (the parent's kernel)", "a3": "device-to-device copy, 32 B per pixel",
            "b1": "TemporalAccumulateDevice (k_temporal)", "b2": "device-to-device copy moving 104 B per pixel (52 read, 52 written)"}
    print("room of %d triangles from inside, %d x %d, build %s, median of %d (least .. greatest) kernel / copy ms, the sequences alternating" % (ntri, w, h, build, args.runs))
    for k in seqs:
        print("(%s) %-66s %8.4f (%8.4f .. %8.4f)" % (k, what[k], med[k], rng_[k][0], rng_[k][1]))
    floor = med["a2"] + med["a3"]
    print("(a) the fused launch %.4f ms against the two-pass floor a2 + a3 = %.4f ms: %s by %.4f ms; the motion plane costs %.4f ms over the hit plane alone"
          % (med["a1"], floor, "under" if med["a1"] < floor else "NOT under", abs(floor - med["a1"]), med["a1"] - med["a2"]))
    gbs = lambda ms: 104.0 * n / (ms * 1e-3) / 1e9
    print("(b) k_temporal moves its compulsory 104 B per pixel (%.1f MB) at %.1f GB/s; the copy of the same traffic runs at %.1f GB/s; %.1f %% of the pixels found their history"
          % (104.0 * n / 1e6, gbs(med["b1"]), gbs(med["b2"]), 100.0 * found))
    if args.log:
        with open(args.log, "w") as f:
            f.write(json.dumps(dict(scene="cornell tess %d, displace 0.2" % args.tess, triangles=ntri, camera="breakfast_interior", width=w, height=h, build=build, runs=args.runs)) + "\n")
            for x in raw:
                f.write(json.dumps(x) + "\n")
    lib.Raylib_DestroyCamera(prev)
    ses.close()


if __name__ == "__main__":
    sys.exit(main())
