#!/usr/bin/env python3
"""The lightmap atlas filter measured (RaylibAMD_BakeLightmapFiltered, RaylibAMD_FilterLightmap; include/raylib_amd.h statement F): the HIP-event time of the
filter stage as the library logs it for a synchronous call under RAYLIB_LIGHTMAP_LOG=1, the median of RUNS calls after a warm-up, for K = 1 .. ITERATIONS on a raw
bake of each kind -- iteration i's time is median(K = i + 1) - median(K = i) --, beside the compulsory traffic of an iteration (one read and one write of the
covered texels' values and one read of their guides) at the 6.3 TB/s a streaming kernel reaches on the MI355X; and the unfiltered bake's stage times, the
medians of as many runs, to set against the ones recorded before the filter existed (profiles/r19_lightmap.log).

usage: python tools/gpu_lightmap_filter.py [--size 1024] [--iterations 5] [--samples 16] [--tess 91] [--runs 11] [--out PATH]
The scene is raylib_amd.scenes.textured (298 116 triangles at its default size), the atlas the tests' "grid" chart layout.
"""
import argparse
import ctypes as C
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["RAYLIB_LIGHTMAP_LOG"] = "1"
os.environ.pop("RAYLIB_QUIET", None)
HBM_STREAM = 6.3e12   # bytes per second


class Captured:
    """What the library logs (C stdout) while the block runs, as .text; it is passed on to the real stdout afterwards."""
    def __init__(self, lib):
        self.lib, self.text = lib, ""

    def __enter__(self):
        sys.stdout.flush(); self.lib.Raylib_FlushLogThread()
        self.saved, self.tmp = os.dup(1), tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 1)
        return self

    def __exit__(self, *exc):
        self.lib.Raylib_FlushLogThread()
        os.dup2(self.saved, 1); os.close(self.saved)
        self.tmp.seek(0); self.text = self.tmp.read().decode(errors="replace"); self.tmp.close()
        return False


STAGES = [("setup + scan + cover", r"setup \+ scan \+ cover ([0-9.]+) ms"), ("points + compaction", r"points \+ compaction ([0-9.]+) ms"), ("gather", r"gather ([0-9.]+) ms"),
          ("atlas taken", r"atlas taken ([0-9.]+) ms"), ("filter", r"filter \(\d+ iterations\) ([0-9.]+) ms"), ("scatter + dilate", r"scatter \+ dilate ([0-9.]+) ms"),
          ("whole", r"whole ([0-9.]+) ms")]


def stage_medians(text, skip=1):
    """name -> the median over the logged calls but the first `skip` (the warm-up), for every stage the lines name."""
    out = {}
    for name, pat in STAGES:
        v = [float(x) for x in re.findall(pat, text)][skip:]
        if v:
            out[name] = (statistics.median(v), len(v))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--tess", type=int, default=91)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from raylib_amd import binding, scenes
    import lightmap_cases as lc
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1, "no HIP device"
    lib.RaylibAMD_SetSeed(1)
    lib.RaylibAMD_BuildId.restype = C.c_char_p
    d = tempfile.mkdtemp()
    obj, n_tris = scenes.textured(os.path.join(d, "textured.obj"), tess=a.tess)
    cam = scenes.CONFIG_CAMERAS["breakfast"]
    ses = binding.SceneSession(lib, obj, cam["origin"], cam["look_at"], cam["fov"], 1.0, sun=cam["sun"], sun_dir=cam["sun_dir"])
    uv = lc.grid_uv(n_tris)
    w = h = a.size
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    # sigmaPosition: two texel footprints in world units -- twice the median distance between the points of texels that are neighbours in a row
    pts, tex, count = binding.lightmap_points(lib, ses.scene, w, h, uv)
    pair = (tex[1:] == tex[:-1] + 1) & (tex[1:] % w != 0)
    foot = float(np.median(np.linalg.norm(pts[1:][pair][:, :3] - pts[:-1][pair][:, :3], axis=1)))
    sigmas = (0.5, 0.3, 2.0 * foot)
    say("build %s: scenes.textured tess %d (%d triangles), %d x %d grid atlas, %d points = %.1f %% of the atlas, %d samples, maxPathLength 5; medians of %d runs after a warm-up"
        % (lib.RaylibAMD_BuildId().decode(), a.tess, n_tris, w, h, count, 100.0 * count / (w * h), a.samples, a.runs))
    say("sigmaColor %.2f sigmaNormal %.2f sigmaPosition %.5f (texel footprint %.5f world units)" % (sigmas + (foot,)))
    # the unfiltered bake, as before the filter existed
    with Captured(lib) as cap:
        for _ in range(a.runs + 1):
            binding.bake_lightmap(lib, ses.scene, w, h, uv, binding.GATHER_IRRADIANCE, dilate=2, sample_count=a.samples)
    say("RaylibAMD_BakeLightmap, IRRADIANCE, dilate 2: " + ", ".join("%s %.3f ms" % (k, v[0]) for k, v in stage_medians(cap.text).items()))
    for kind, name in ((binding.GATHER_IRRADIANCE, "IRRADIANCE"), (binding.GATHER_SH9, "SH9")):
        c = 4 if kind == binding.GATHER_IRRADIANCE else 27
        with Captured(lib) as cap:
            for _ in range(a.runs + 1):
                binding.bake_lightmap(lib, ses.scene, w, h, uv, kind, dilate=2, sample_count=a.samples, filter=(a.iterations,) + sigmas)
        say("RaylibAMD_BakeLightmapFiltered, %s, K = %d, dilate 2: " % (name, a.iterations) + ", ".join("%s %.3f ms" % (k, v[0]) for k, v in stage_medians(cap.text).items()))
        raw, _ = binding.bake_lightmap(lib, ses.scene, w, h, uv, kind, dilate=0, sample_count=a.samples)
        total = [0.0]
        for k in range(1, a.iterations + 1):
            with Captured(lib) as cap:
                for _ in range(a.runs + 1):
                    binding.filter_lightmap(lib, ses.scene, w, h, raw, (k,) + sigmas, uv, kind, dilate=0)
            total.append(stage_medians(cap.text)["filter"][0])
        traffic = count * (2 * c * 4 + 32)
        floor_ms = traffic / HBM_STREAM * 1e3
        say("RaylibAMD_FilterLightmap, %s: compulsory traffic of an iteration %d points x (2 x %d + 32) bytes = %.1f MB = %.4f ms at 6.3 TB/s" % (name, count, 4 * c, traffic / 1e6, floor_ms))
        for k in range(1, a.iterations + 1):
            it = total[k] - total[k - 1]
            say("  iteration %d (step %2d): %.4f ms = %.1f x the traffic's time      (filter stage with K = %d: %.4f ms)" % (k - 1, 1 << (k - 1), it, it / floor_ms, k, total[k]))
        say("  K = %d in total: %.4f ms = %.1f x the traffic's time of %d iterations" % (a.iterations, total[-1], total[-1] / (floor_ms * a.iterations), a.iterations))
    ses.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
