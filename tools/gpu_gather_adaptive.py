#!/usr/bin/env python3
"""The adaptive bake measured against the plain one (RaylibAMD_BakeLightmapAdaptive, RaylibAMD_BakeLightmap; include/raylib_amd.h statements A1 to A5): the
HIP-event time of the whole synchronous call (RaylibAMD_GetLastStats kernelMs) and its cameraSamples, RUNS runs of every item, alternated, after a warm-up.

  a   RaylibAMD_BakeLightmap at CAP samples: the baseline
  b   the adaptive bake at threshold 0 in passes of PASS samples: the same samples plus a resolve, a compaction and a read-back per pass; b / a is the passes' overhead
  b1  the adaptive bake at threshold 0 with passSamples = CAP: one pass, the moments on top of the sums
  c   the adaptive bake at the two thresholds that trace about one half and one quarter of a's samples (found by bisection on cameraSamples)

and the two criteria on them: b1's median must not exceed a's slowest run by more than a's own spread; a run that traces at most half of a's samples must have a
median below a's fastest run.  One process; every GPU step runs under a time limit of its own, after which the process ends with status 124.

usage: python tools/gpu_gather_adaptive.py [--size 256] [--cap 256] [--pass-samples 16] [--tess 91] [--runs 5] [--out PATH]
The scene is raylib_amd.scenes.textured (298 116 triangles at its default size), the atlas the tests' "grid" chart layout, as tools/gpu_lightmap_filter.py.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("RAYLIB_QUIET", "1")


class Limit:
    """The block under a time limit: a timer thread ends the process (status 124) when the block has not returned by then -- also out of a call that hangs."""
    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self.expired)
        self.t.daemon = True
        self.what, self.seconds = what, seconds

    def expired(self):
        sys.stderr.write("time limit of %d s reached in: %s\n" % (self.seconds, self.what))
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.t.start()
        return self

    def __exit__(self, *exc):
        self.t.cancel()
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--pass-samples", type=int, default=16)
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--tess", type=int, default=91)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from raylib_amd import binding, scenes
    import lightmap_cases as lc
    lib = binding.load()
    with Limit(120, "initialising the device"):
        assert lib.Raylib_Initialize() == 1, "no HIP device"
    lib.RaylibAMD_SetSeed(1)
    lib.RaylibAMD_BuildId.restype = C.c_char_p
    d = tempfile.mkdtemp()
    obj, n_tris = scenes.textured(os.path.join(d, "textured.obj"), tess=a.tess)
    cam = scenes.CONFIG_CAMERAS["breakfast"]
    ses = binding.SceneSession(lib, obj, cam["origin"], cam["look_at"], cam["fov"], 1.0, sun=cam["sun"], sun_dir=cam["sun_dir"])
    uv = lc.grid_uv(n_tris)
    w = h = a.size
    K = binding.GATHER_IRRADIANCE
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def stats():
        st = binding.Stats()
        lib.RaylibAMD_GetLastStats(C.byref(st))
        return st

    def plain():
        with Limit(120, "RaylibAMD_BakeLightmap"):
            binding.bake_lightmap(lib, ses.scene, w, h, uv, K, sample_count=a.cap)
        st = stats()
        return st.kernelMs, int(st.cameraSamples), int(st.traceLaunches), int(st.pixels)

    def adaptive(threshold, pass_samples):
        with Limit(120, "RaylibAMD_BakeLightmapAdaptive, threshold %g" % threshold):
            binding.bake_lightmap_adaptive(lib, ses.scene, w, h, threshold, a.min_samples, pass_samples, uv, K, sample_count=a.cap)
        st = stats()
        return st.kernelMs, int(st.cameraSamples), int(st.traceLaunches), int(st.pixels)

    _, full, _, count = plain()                       # the warm-up: the scene's upload, the scratch
    adaptive(0.0, a.pass_samples)

    def threshold_for(share):
        """the threshold that traces the most samples still within share x the plain bake's, by bisection (the samples traced grow as the threshold falls)"""
        lo, hi = 0.0, 0.5                             # y lies in [0, 1): no error exceeds 1 / 2
        best = None
        for _ in range(16):
            mid = (lo + hi) / 2
            got = adaptive(mid, a.pass_samples)[1]
            if got <= share * full and (best is None or got > best[1]):
                best = (mid, got)                     # the most samples that are still at most the share
            if got > share * full:
                lo = mid
            else:
                hi = mid
        return best[0] if best else hi
    t_half, t_quarter = threshold_for(0.5), threshold_for(0.25)
    items = [("a", "RaylibAMD_BakeLightmap", plain),
             ("b", "adaptive, threshold 0, passes of %d" % a.pass_samples, lambda: adaptive(0.0, a.pass_samples)),
             ("b1", "adaptive, threshold 0, one pass of %d" % a.cap, lambda: adaptive(0.0, a.cap)),
             ("c1", "adaptive, threshold %.6g, passes of %d" % (t_half, a.pass_samples), lambda: adaptive(t_half, a.pass_samples)),
             ("c2", "adaptive, threshold %.6g, passes of %d" % (t_quarter, a.pass_samples), lambda: adaptive(t_quarter, a.pass_samples))]
    runs = {k: [] for k, _, _ in items}
    for _ in range(a.runs):                           # alternated: a b b1 c1 c2, a b b1 c1 c2, ...
        for k, _, fn in items:
            runs[k].append(fn())
    say("build %s: scenes.textured tess %d (%d triangles), %d x %d grid atlas, %d points = %.1f %% of the atlas, IRRADIANCE, cap %d, minSamples %d, maxPathLength 5; "
        "%d runs of every item, alternated, after a warm-up; times are the whole call's HIP-event time (kernelMs)"
        % (lib.RaylibAMD_BuildId().decode(), a.tess, n_tris, w, h, count, 100.0 * count / (w * h), a.cap, a.min_samples, a.runs))
    med = {}
    for k, name, _ in items:
        ms = [r[0] for r in runs[k]]
        med[k] = statistics.median(ms)
        say("%-2s %-48s samples %10d = %5.1f %% of a's, %4d trace launches | ms: %s | fastest %.3f median %.3f slowest %.3f"
            % (k, name, runs[k][0][1], 100.0 * runs[k][0][1] / full, runs[k][0][2], " ".join("%.3f" % v for v in ms), min(ms), med[k], max(ms)))
    a_ms = [r[0] for r in runs["a"]]
    a_fast, a_slow = min(a_ms), max(a_ms)
    say("b / a = %.4f: the overhead of %d passes (resolves with moments, compactions, read-backs of the live count) on the same samples" % (med["b"] / med["a"], runs["b"][0][2]))
    bound = a_slow + (a_slow - a_fast)
    say("criterion b1: median %.3f ms <= a's slowest %.3f + a's spread %.3f = %.3f ms: %s" % (med["b1"], a_slow, a_slow - a_fast, bound, "met" if med["b1"] <= bound else "NOT met"))
    for k in ("c1", "c2"):
        share = runs[k][0][1] / full
        verdict = ("met" if med[k] < a_fast else "NOT met") if share <= 0.5 else "does not apply (more than half of the samples)"
        say("criterion %s: %.1f %% of the samples in %.1f %% of a's median time; median %.3f ms < a's fastest %.3f ms: %s"
            % (k, 100.0 * share, 100.0 * med[k] / med["a"], med[k], a_fast, verdict))
    ses.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
