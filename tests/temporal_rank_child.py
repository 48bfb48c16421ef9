"""Child process of tests/test_gpu_temporal_ranks.py (modelled on tests/gbuffer_rank_child.py): the library reads RAYLIB_NUM_GPUS / RAYLIB_GPU_MAP once, when
it initialises, so a rank layout needs its own process.  Raylib_Render of the Cornell scene at 1920 x 1080, 2 samples -- with several ranks the frame is still
in flight when the call returns -- then at once the motion launch and the accumulation of a tessellated room, through the host entries and through the device
entries on a stream of the caller's; then the stats, and the frame's pixels.

usage: python temporal_rank_child.py <workdir> <out.npz>"""
import ctypes as C
import os
import sys

import numpy as np
import torch    # before the library is loaded

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import temporal_cases as tc  # noqa: E402
from raylib_amd import binding  # noqa: E402

FRAME = (1920, 1080, 2)
W, H, TMIN = tc.W, tc.H, 1e-4


def run(lib, workdir):
    d = os.path.join(str(workdir), "temporal_rank_%d" % os.getpid()); os.makedirs(d, exist_ok=True)
    ses = binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "cornell.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1920 / 1080)
    room = binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "room.obj"), tess=4)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    prev = binding.create_camera(lib, (0.2, 1.1, 3.9), (0, 1, -1), 45.0, 1.0)
    try:
        w, h, spp = FRAME
        first, pp = tc.partial_move(room.export_flat()[0])
        rng = np.random.RandomState(5)
        colour = rng.uniform(0, 2, (H, W, 4)).astype(np.float32); colour[..., 3] = 1
        hist_colour = rng.uniform(0, 2, (H, W, 4)).astype(np.float32); hist_colour[..., 3] = 1
        hist_len = rng.choice(np.asarray([0, 1, 3, 8], np.float32), (H, W)).astype(np.float32)
        ses.render(64, 48, 1)                                   # the scene is on every rank's device
        ranks = np.int64(ses.stats().ranks)                     # (read behind the render's own frame: RaylibAMD_GetLastStats completes it)
        room.motion(8, 8, planes=("hit",))                      # ... and the room, its tree and its table on rank 0's
        hist_hit = room.motion(W, H, planes=("hit",))["hit"]    # the history's hit plane: this frame's (nothing of the room moved for the walk)
        t_colour, t_pp, t_hcol, t_hhit, t_hlen = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (colour, pp, hist_colour, hist_hit.view(np.int32).reshape(H, W, 4), hist_len))
        torch.cuda.synchronize()
        st = ses.settings(w, h, spp)
        img = lib.Raylib_CreateImage(w, h)
        lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, img)      # nothing is read: in flight
        out = {}
        m = room.motion(W, H, prev, first, pp, TMIN)
        stats = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(stats))
        out["motion_stats"] = np.array([stats.ranks, stats.cameraSamples, stats.pixels, stats.rays, stats.nodesVisited, stats.trisTested, stats.treeWidth], np.int64)
        acc = room.temporal_accumulate(colour, m["hit"], m["motion"], (hist_colour, hist_hit, hist_len), 0.05, 16.0)
        stats = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(stats))
        out["accumulate_stats"] = np.array([stats.ranks, stats.pixels, stats.rays], np.int64)
        for k, v in (("hit", m["hit"]), ("motion", m["motion"]), ("colour", acc[0]), ("length", acc[1])):
            out["host_entry_" + k] = np.ascontiguousarray(v).view(np.uint8)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dm = room.motion_device(W, H, prev, first, t_pp, TMIN)
            da = room.temporal_accumulate_device(t_colour, dm["hit"], dm["motion"], (t_hcol, t_hhit, t_hlen), 0.05, 16.0)      # no host synchronisation between
        s.synchronize()
        for k, v in (("hit", dm["hit"]), ("motion", dm["motion"]), ("colour", da[0]), ("length", da[1])):
            out["device_entry_" + k] = v.cpu().numpy().view(np.uint8)
        frame = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, frame.ctypes.data_as(C.POINTER(C.c_float)))
        lib.Raylib_DestroyImage(img)
        out["frame"] = frame
        out["ranks"] = ranks
        return out
    finally:
        lib.Raylib_DestroyCamera(prev)
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
