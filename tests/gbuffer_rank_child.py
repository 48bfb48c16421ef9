"""Child process of tests/test_gpu_gbuffer_ranks.py (modelled on tests/sdf_rank_child.py): the library reads RAYLIB_NUM_GPUS / RAYLIB_GPU_MAP once, when it
initialises, so a rank layout needs its own process.  Raylib_Render of the Cornell scene at 1920 x 1080, 2 samples -- with several ranks the frame is still in
flight when the call returns -- then at once the G-buffer of a tessellated room through the host entry and through the device entry on a stream of the
caller's; then the stats, and the frame's pixels.

usage: python gbuffer_rank_child.py <workdir> <out.npz>"""
import ctypes as C
import os
import sys

import numpy as np
import torch    # before the library is loaded

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
from raylib_amd import binding  # noqa: E402

FRAME = (1920, 1080, 2)
W, H, TMIN = 37, 21, 1e-4


def run(lib, workdir):
    d = os.path.join(str(workdir), "gbuffer_rank_%d" % os.getpid()); os.makedirs(d, exist_ok=True)
    ses = binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "cornell.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1920 / 1080)
    room = binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "room.obj"), tess=4)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    try:
        w, h, spp = FRAME
        ses.render(64, 48, 1)                                   # the scene is on every rank's device
        ranks = np.int64(ses.stats().ranks)                     # (read behind the render's own frame: RaylibAMD_GetLastStats completes it)
        room.gbuffer(8, 8, TMIN)                                # ... and the room, its tree and its table on rank 0's
        torch.cuda.synchronize()
        st = ses.settings(w, h, spp)
        img = lib.Raylib_CreateImage(w, h)
        lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, img)      # nothing is read: in flight
        out = {}
        for k, v in room.gbuffer(W, H, TMIN).items():
            out["host_entry_" + k] = v.view(np.uint8)
        stats = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(stats))
        out["stats"] = np.array([stats.ranks, stats.cameraSamples, stats.pixels, stats.rays, stats.nodesVisited, stats.trisTested, stats.shadedHits, stats.treeWidth], np.int64)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dev = room.gbuffer_device(W, H, TMIN)
        s.synchronize()
        for k, v in dev.items():
            out["device_entry_" + k] = v.cpu().numpy().view(np.uint8)
        frame = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, frame.ctypes.data_as(C.POINTER(C.c_float)))
        lib.Raylib_DestroyImage(img)
        out["frame"] = frame
        out["ranks"] = ranks
        return out
    finally:
        ses.close(); room.close()


def main():
    workdir, path = sys.argv[1], sys.argv[2]
    os.environ.setdefault("RAYLIB_QUIET", "1")
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1, "no HIP device"
    lib.RaylibAMD_SetSeed(1)
    np.savez(path, **run(lib, workdir))


if __name__ == "__main__":
    main()
