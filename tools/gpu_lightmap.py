#!/usr/bin/env python3
"""RaylibAMD_BakeLightmap measured: the HIP-event times of its stages (setup + scan + cover, points + compaction, gather, scatter + dilate: the library logs
them for a synchronous bake under RAYLIB_LIGHTMAP_LOG=1), RUNS bakes after a warm-up, with the build id; and how the (triangle, texel) pairs are spread: the
pairs in all, the triangles that have any, the largest rectangle, the share of the pairs that pass the coverage test -- from the NumPy restatement of the
setup stage (tests/lightmap_cases.py).  k_lm_cover deals one pair to a lane, so the lanes' loads are equal by construction; what varies is how many pairs
there are per covered texel.

usage: python tools/gpu_lightmap.py [--size 1024] [--samples 16] [--dilate 2] [--tess 91] [--runs 3] [--out PATH]
The scene is raylib_amd.scenes.textured (298 116 triangles at its default size), the atlas the tests' "grid" chart layout, the kind IRRADIANCE.
"""
import argparse
import ctypes as C
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "software-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["RAYLIB_LIGHTMAP_LOG"] = "1"
os.environ.pop("RAYLIB_QUIET", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--tess", type=int, default=91)
    ap.add_argument("--runs", type=int, default=3)
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
    lines = ["build %s: scenes.textured tess %d (%d triangles), %d x %d grid atlas, IRRADIANCE, %d samples, maxPathLength 5, dilate %d"
             % (lib.RaylibAMD_BuildId().decode(), a.tess, n_tris, a.size, a.size, a.samples, a.dilate)]
    # the pairs' spread, from the restated setup stage
    X, Y, A2, keep = lc.snap(uv, a.size, a.size)
    x0 = np.maximum(0, -((128 - X.min(1)) // 256)); x1 = np.minimum(a.size - 1, (X.max(1) - 128) // 256)
    y0 = np.maximum(0, -((128 - Y.min(1)) // 256)); y1 = np.minimum(a.size - 1, (Y.max(1) - 128) // 256)
    cells = np.where(keep, np.maximum(0, x1 - x0 + 1) * np.maximum(0, y1 - y0 + 1), 0)
    _, _, count = binding.lightmap_points(lib, ses.scene, a.size, a.size, uv, capacity=0)
    lines.append("pairs %d over %d of %d triangles (max %d, mean %.2f per triangle that has any), one pair per lane: %d waves of 64; %d points = %.1f %% of the pairs, "
                 "%.1f %% of the atlas" % (cells.sum(), (cells > 0).sum(), n_tris, cells.max(), cells.sum() / max(1, (cells > 0).sum()), -(-int(cells.sum()) // 64),
                                           count, 100.0 * count / max(1, cells.sum()), 100.0 * count / (a.size * a.size)))
    print("\n".join(lines), flush=True)
    for run in range(a.runs + 1):
        binding.bake_lightmap(lib, ses.scene, a.size, a.size, uv, binding.GATHER_IRRADIANCE, dilate=a.dilate, sample_count=a.samples)
        st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
        line = "%s: kernelMs %.3f traceKernelMs %.3f wallMs %.3f pixels %d rays %d" % ("warm-up" if run == 0 else "run %d" % run, st.kernelMs, st.traceKernelMs, st.wallMs,
                                                                                     st.pixels, st.rays)
        print(line, flush=True)
        lines.append(line)
    ses.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
