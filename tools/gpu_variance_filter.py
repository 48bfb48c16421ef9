#!/usr/bin/env python3
"""What the accumulation with moments and the variance-guided filter cost (include/raylib_amd.h statements S1 to S7), in one process on one build, beside
RaylibAMD_Denoise on the same frame; and what the filter does to a Cornell frame's error.

usage: python tools/gpu_variance_filter.py [--width 1920] [--height 1080] [--runs 11] [--tess 91] [--lib PATH] [--log PATH]
       python tools/gpu_variance_filter.py --overhead --lib PATH [--runs 11] [--log PATH]
The scene is the bench's 298 116-triangle room (raylib_amd/scenes.py cornell, tess 91, a fifth of the triangles displaced) from the bench's interior camera.  Its
planes: the G-buffer's hit and surface, two 1-spp frames accumulated with moments under identity motion (so every length is 2, below the default historyLength:
every pixel takes the 7 x 7 spatial variance, the dearer branch of S5), and the denoiser's albedo and micro-normal images.
After a warm-up, --runs rounds in which these alternate:
  (m)   RaylibAMD_TemporalAccumulateMomentsDevice             k_temporal_moments, HIP-event pair around the kernel (RaylibAMD_GetLastStats kernelMs)
  (t)   RaylibAMD_TemporalAccumulateDevice                    k_temporal, the same way: what the moments add
  (fK)  RaylibAMD_FilterVarianceDevice at K = 1 .. 6          the event pair around all 2 + K launches; f(K) - f(K - 1) is the iteration at step 2^(K-1), f1 less
                                                              that of a step-1 iteration is not separable here: f1 holds pack, variance and the step-1 iteration
  (dK)  RaylibAMD_Denoise at K = 1 .. 6 on the same frame     it has no event pair of its own: wall clock around the synchronous call, images resident on the
                                                              device; d(K) - d(K - 1) is k_dn_iter at step 2^(K-1), and the call's fixed cost cancels in it
The filter's outputs are checked against RaylibAMD_FilterVarianceHost bit for bit on a 256 x 144 frame of the same scene before anything is timed (the host oracle
at 1920 x 1080 takes minutes).  Then the quality figures of tests/test_gpu_variance.py (tests/variance_cases.quality) on the Cornell box.
--log: everything printed, and the raw runs as JSON lines, with the library's build id.
--overhead: the host path of a synchronous plane call, the tree's library against --lib's in one process (overhead()).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("RAYLIB_QUIET", "1")


def overhead(args):
    """--overhead: what a synchronous plane call costs beside its kernels -- wallMs - kernelMs of its stats, in microseconds: the staging of the input planes,
    the copies back, the host's own work -- for the host entries of the accumulation with moments (with a history) and of the filter at K = 5, on frames of
    1 x 1 and of width x height pixels (tests/variance_cases.no_bleed_planes: no scene is needed).  The tree's library and --lib's (another build, e.g. the parent
    commit's) take turns call by call in this one process, --runs calls each after 3 warm-up calls.  Per build the median, the least and the greatest; the
    tree's median is then placed against the other build's spread."""
    import numpy as np
    from raylib_amd import binding
    import variance_cases as vc
    builds = {"tree": binding.load(), "other": binding.load(args.lib)}
    for lib in builds.values():
        assert lib.Raylib_Initialize() == 1, "no HIP device"
    lines = []

    def say(s):
        print(s); lines.append(s)
    say("%-10s %-6s %11s %-17s %10s %10s %10s" % ("call", "build", "frame", "id", "median us", "least", "greatest"))
    for w, h in ((1, 1), (args.width, args.height)):
        colour, moments, length, hit, surface, _ = vc.no_bleed_planes(w, h)
        motion = vc.identity_motion(hit)
        calls = {"moments": lambda lib: binding.temporal_accumulate_moments(lib, colour, hit, motion, (colour, hit, length, moments)),
                 "filter K=5": lambda lib: binding.filter_variance(lib, colour, moments, length, hit, surface, params=dict(iterations=5))}
        for what, call in calls.items():
            us = {name: [] for name in builds}
            for k in range(args.runs + 3):
                for name, lib in builds.items():
                    call(lib)
                    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
                    if k >= 3:
                        us[name].append((st.wallMs - st.kernelMs) * 1e3)
            for name, lib in builds.items():
                say("%-10s %-6s %11s %-17s %10.1f %10.1f %10.1f" % (what, name, "%d x %d" % (w, h), lib.RaylibAMD_BuildId().decode(), np.median(us[name]), min(us[name]), max(us[name])))
            mid = np.median(us["tree"])
            say("%-10s %d x %d: the tree's median is %s the other build's spread" % (what, w, h, "within" if min(us["other"]) <= mid <= max(us["other"]) else "below" if mid < min(us["other"]) else "ABOVE"))
    if args.log:
        with open(args.log, "w") as fh_:
            fh_.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--tess", type=int, default=91)
    ap.add_argument("--lib")
    ap.add_argument("--log")
    ap.add_argument("--overhead", action="store_true")
    args = ap.parse_args()
    if args.overhead:
        if not args.lib:
            ap.error("--overhead compares the tree's library with --lib's")
        return overhead(args)
    import numpy as np
    import torch
    from raylib_amd import binding, scenes
    import variance_cases as vc
    lib = binding.load(args.lib) if args.lib else binding.load()
    assert lib.Raylib_Initialize() == 1, "no HIP device"
    lib.RaylibAMD_SetSeed(1)
    lines = []

    def say(s):
        print(s); lines.append(s)
    w, h, tmin = args.width, args.height, 1e-4
    n = w * h
    cam = scenes.CONFIG_CAMERAS["breakfast_interior"]
    tmp = tempfile.mkdtemp()
    obj, ntri = scenes.cornell(os.path.join(tmp, "room.obj"), tess=args.tess, displace_fraction=0.2)
    ses = binding.SceneSession(lib, obj, cam["origin"], cam["look_at"], cam["fov"], w / h, sun=cam["sun"], sun_dir=cam["sun_dir"])
    build = lib.RaylibAMD_BuildId().decode()

    def frame(lib_, ses_, seed, fw, fh, spp):
        lib_.RaylibAMD_SetSeed(seed)
        try:
            return np.ascontiguousarray(ses_.render_cells(fw, fh, spp, 0, 1)).reshape(fh, fw, 4)
        finally:
            lib_.RaylibAMD_SetSeed(1)

    # what is timed is right: a small frame of the same scene against the oracle
    sw, sh = 256, 144
    gb = ses.gbuffer(sw, sh, tmin, ("hit", "surface"))
    mo = vc.identity_motion(gb["hit"])
    a0 = binding.temporal_accumulate_moments(lib, frame(lib, ses, 2, sw, sh, 1), gb["hit"], mo, None)
    a1 = binding.temporal_accumulate_moments(lib, frame(lib, ses, 3, sw, sh, 1), gb["hit"], mo, (a0[0], gb["hit"], a0[1], a0[2]))
    want = binding.temporal_accumulate_moments(lib, frame(lib, ses, 3, sw, sh, 1), gb["hit"], mo, (a0[0], gb["hit"], a0[1], a0[2]), host=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a1, want)), "the accumulation differs from its host oracle"
    got = binding.filter_variance(lib, a1[0], a1[2], a1[1], gb["hit"], gb["surface"])
    want = binding.filter_variance(lib, a1[0], a1[2], a1[1], gb["hit"], gb["surface"], host=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)), "the filter differs from its host oracle"

    # the timed frame's planes, on the device
    g = ses.gbuffer_device(w, h, tmin, ("hit", "surface"))
    hit_np = g["hit"].cpu().numpy().view(binding.HITT_DTYPE).reshape(h, w)
    motion = torch.from_numpy(vc.identity_motion(hit_np).view(np.int32).reshape(h, w, 4)).cuda()
    c0, c1 = (torch.from_numpy(frame(lib, ses, s, w, h, 1)).cuda() for s in (2, 3))
    torch.cuda.synchronize()
    first = binding.temporal_accumulate_moments_device(lib, c0, g["hit"], motion, None)
    hist = (first[0], g["hit"], first[1], first[2])
    acc = binding.temporal_accumulate_moments_device(lib, c1, g["hit"], motion, hist)
    out_c = torch.empty((h, w, 4), dtype=torch.float32, device="cuda"); out_v = torch.empty((h, w), dtype=torch.float32, device="cuda")
    images = []
    st1 = binding.RendererSettings(w, h, 1, 5, tmin, binding.RENDERMODE_DEFAULT)
    main_img = lib.Raylib_CreateImage(w, h); images.append(main_img)
    lib.Raylib_Render(C.byref(st1), ses.scene, ses.camera, main_img)
    albedo, normal, den_out = (lib.Raylib_CreateImage(w, h) for _ in range(3)); images += [albedo, normal, den_out]
    assert binding.render_guides(lib, ses.scene, ses.camera, w, h, albedo, normal, tmin) == 1

    def kernel_ms():
        s = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(s))
        return s.kernelMs

    def m():
        binding.temporal_accumulate_moments_device(lib, c1, g["hit"], motion, hist, out=acc)
        return kernel_ms()

    def t():
        binding.temporal_accumulate_device(lib, c1, g["hit"], motion, hist[:3], out=acc[:2])
        return kernel_ms()

    def f(k):
        def run():
            binding.filter_variance_device(lib, acc[0], acc[2], acc[1], g["hit"], g["surface"], params=dict(iterations=k), out=(out_c, out_v))
            return kernel_ms()
        return run

    def d(k):
        p = binding.DenoiseParams(k, 0.6, 0.35, 0.25)

        def run():
            t0 = time.perf_counter()
            assert lib.RaylibAMD_Denoise(main_img, 1, albedo, normal, den_out, C.byref(p)) == 1
            return (time.perf_counter() - t0) * 1e3
        return run
    seqs = {"m": m, "t": t}
    seqs.update({"f%d" % k: f(k) for k in range(1, 7)})
    seqs.update({"d%d" % k: d(k) for k in range(1, 7)})
    for fn in seqs.values():      # the warm-up: code objects, scratch, staging
        fn(); fn()
    raw = []
    for r in range(args.runs):
        for name, fn in seqs.items():
            raw.append(dict(run=r, seq=name, ms=fn()))
    med = {k: float(np.median([x["ms"] for x in raw if x["seq"] == k])) for k in seqs}
    lo = {k: min(x["ms"] for x in raw if x["seq"] == k) for k in seqs}
    hi = {k: max(x["ms"] for x in raw if x["seq"] == k) for k in seqs}
    say("room of %d triangles from inside, %d x %d, build %s, median of %d (least .. greatest) ms, the sequences alternating" % (ntri, w, h, build, args.runs))
    say("(m)  TemporalAccumulateMomentsDevice, kernel   %8.4f (%8.4f .. %8.4f)   128 B per pixel compulsory (48 read, 44 of history read once, 28 written): %.1f GB/s"
        % (med["m"], lo["m"], hi["m"], 128.0 * n / (med["m"] * 1e-3) / 1e9))
    say("(t)  TemporalAccumulateDevice, kernel          %8.4f (%8.4f .. %8.4f)   104 B per pixel: %.1f GB/s" % (med["t"], lo["t"], hi["t"], 104.0 * n / (med["t"] * 1e-3) / 1e9))
    for k in range(1, 7):
        step = med["f%d" % k] - (med["f%d" % (k - 1)] if k > 1 else 0.0)
        dstep = med["d%d" % k] - (med["d%d" % (k - 1)] if k > 1 else 0.0)
        say("(f%d) FilterVarianceDevice K = %d, kernels       %8.4f (%8.4f .. %8.4f)   over K - 1: %8.4f  |  (d%d) Denoise K = %d, wall %8.4f (%8.4f .. %8.4f)   over K - 1: %8.4f"
            % (k, k, med["f%d" % k], lo["f%d" % k], hi["f%d" % k], step, k, k, med["d%d" % k], lo["d%d" % k], hi["d%d" % k], dstep))
    # compulsory traffic of the filter's launches, per pixel: pack reads 16 + 16 + 44 and writes 32 + 16; variance reads 32 + 8 + 4 and writes 4 (its window comes
    # from cache); an iteration reads 32 + 16 and writes 16 (the last: 16 + 4).  k_dn_iter reads 3 x 16 and writes 16.
    pack, var, it, last = 124.0, 48.0, 64.0, 68.0
    for k in (1, 5):
        total = (pack + var + (k - 1) * it + last) * n
        say("compulsory traffic of a K = %d filter call: %.1f MB, which the measured %.4f ms moves at %.1f GB/s" % (k, total / 1e6, med["f%d" % k], total / (med["f%d" % k] * 1e-3) / 1e9))
    say("compulsory traffic of one middle iteration: %.1f MB (k_vf_iter) against %.1f MB (k_dn_iter)" % (it * n / 1e6, 64.0 * n / 1e6))
    # the quality figures of the test
    cornell = binding.SceneSession(lib, scenes.cornell(os.path.join(tmp, "cornell.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    mse_acc, mse_fil = vc.quality(lib, cornell, frame)
    say("Cornell 64 x 40, 8 x 1 spp (seeds 10 .. 17) accumulated under identity motion, against 1024 spp: mse accumulated %.6g, filtered with the defaults %.6g" % (mse_acc, mse_fil))
    cornell.close()
    if args.log:
        with open(args.log, "w") as fh_:
            for s in lines:
                fh_.write(s + "\n")
            fh_.write(json.dumps(dict(scene="cornell tess %d, displace 0.2" % args.tess, triangles=ntri, camera="breakfast_interior", width=w, height=h, build=build, runs=args.runs)) + "\n")
            for x in raw:
                fh_.write(json.dumps(x) + "\n")
    for img in images:
        lib.Raylib_DestroyImage(img)
    ses.close()


if __name__ == "__main__":
    sys.exit(main())
