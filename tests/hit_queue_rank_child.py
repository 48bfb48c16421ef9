"""Child process of tests/test_gpu_hit_queue.py: the library reads RAYLIB_NUM_GPUS / RAYLIB_GPU_MAP once, when it initialises, so a rank layout needs its own
process.  One Raylib_Render of an OBJ scene from the Cornell camera; stores the frame, which megakernel ran and the render's counters.
usage: python hit_queue_rank_child.py <out.npz> <file.obj> <width> <height> <spp>"""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402,F401  (sets sys.path)

COUNTERS = ("rays", "nodesVisited", "trisTested", "shadedHits", "texFetches", "cameraSamples", "culledSamples", "pixels", "litPaths", "litFoldedInPlace")

if __name__ == "__main__":
    from raylib_amd import binding
    out, obj, w, h, spp = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1
    lib.RaylibAMD_SetSeed(1)
    ses = binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, w / h)
    img = ses.render(w, h, spp)
    s = ses.stats()
    np.savez(out, img=img, ranks=s.ranks, lazy=lib.RaylibAMD_LastTraceLazy(), hitQueue=lib.RaylibAMD_LastHitQueue(),
             counters=np.asarray([getattr(s, k) for k in COUNTERS], np.int64))
    ses.close()
