"""Child process of tests/test_gpu_sdf.py::test_behind_a_multi_rank_frame_in_flight (modelled on tests/nearest_rank_child.py): the library reads
RAYLIB_NUM_GPUS / RAYLIB_GPU_MAP once, when it initialises, so a rank layout needs its own process.  Raylib_Render of the Cornell scene at 1920 x 1080, 2
samples -- with several ranks the frame is still in flight when the call returns -- then at once a distance-field bake of a torus through the host entry and
through the device entry on a stream of the caller's; then the oracle's answer and the frame's pixels.

usage: python sdf_rank_child.py <workdir> <out.npz>"""
import ctypes as C
import os
import sys

import numpy as np
import torch    # before the library is loaded

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import sdf_cases as sc  # noqa: E402
from raylib_amd import binding  # noqa: E402

FRAME = (1920, 1080, 2)
DIMS = (20, 17, 9)


def run(lib, workdir):
    d = os.path.join(str(workdir), "sdf_rank_%d" % os.getpid()); os.makedirs(d, exist_ok=True)
    ses = sc.session(lib, helpers.scenes.cornell(os.path.join(d, "cornell.obj"))[0])
    torus = sc.session(lib, sc.write_mesh(os.path.join(d, "torus.obj"), "torus"))
    try:
        origin, spacing = sc.grid_around(DIMS, shift=sc.IRRATIONAL)
        args = (origin, spacing, DIMS, float("inf"), sc.MAJORITY)
        w, h, spp = FRAME
        ses.render(64, 48, 1)                                   # the scene is on every rank's device
        ranks = np.int64(ses.stats().ranks)                     # (read behind the render's own frame: RaylibAMD_GetLastStats completes it)
        sc.bake(lib, torus, *args)                              # ... and the torus, its trees and tables on rank 0's
        torch.cuda.synchronize()
        st = ses.settings(w, h, spp)
        img = lib.Raylib_CreateImage(w, h)
        lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, img)      # nothing is read: in flight
        out = {}
        out["host_entry_dist"], out["host_entry_prim"] = sc.bake(lib, torus, *args, prim=True)
        stats = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(stats))
        nx, ny, nz = DIMS
        assert stats.rays == nx * ny * nz + ny * nz + nx * nz + nx * ny, "the synchronous bake reports its own numbers, not the frame's"
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            td, tp = sc.bake(lib, torus, *args, prim=True, device=True)
        s.synchronize()
        out["device_entry_dist"], out["device_entry_prim"] = td.cpu().numpy(), tp.cpu().numpy()
        frame = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, frame.ctypes.data_as(C.POINTER(C.c_float)))
        lib.Raylib_DestroyImage(img)
        out["frame"] = frame
        out["oracle_dist"], out["oracle_prim"] = sc.bake(lib, torus, *args, prim=True, host=True)
        out["ranks"] = ranks
        return out
    finally:
        ses.close(); torus.close()


def main():
    workdir, path = sys.argv[1], sys.argv[2]
    os.environ.setdefault("RAYLIB_QUIET", "1")
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1, "no HIP device"
    lib.RaylibAMD_SetSeed(1)
    np.savez(path, **run(lib, workdir))


if __name__ == "__main__":
    main()
