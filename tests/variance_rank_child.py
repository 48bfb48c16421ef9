"""Child process of tests/test_gpu_variance_ranks.py (modelled on tests/temporal_rank_child.py): the library reads RAYLIB_NUM_GPUS / RAYLIB_GPU_MAP once, when it
initialises, so a rank layout needs its own process.  Raylib_Render of the Cornell scene at 1920 x 1080, 2 samples -- with several ranks the frame is still in
flight when the call returns -- then at once the accumulation with moments and the variance-guided filter on the crafted planes, through the host entries and
through the device entries on a stream of the caller's; then the stats, and the frame's pixels.

usage: python variance_rank_child.py <workdir> <out.npz>"""
import ctypes as C
import os
import sys

import numpy as np
import torch    # before the library is loaded

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import temporal_cases as tc  # noqa: E402
import variance_cases as vc  # noqa: E402
from raylib_amd import binding  # noqa: E402

FRAME = (1920, 1080, 2)
W, H = vc.W, vc.H
PARAMS = dict(iterations=4, history_length=2.5)
OUTPUTS = ("colour", "length", "moments", "filtered", "variance")


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.int32).reshape(a.shape + (a.dtype.itemsize // 4,))
    return torch.from_numpy(a).cuda()


def run(lib, workdir):
    d = os.path.join(str(workdir), "variance_rank_%d" % os.getpid()); os.makedirs(d, exist_ok=True)
    ses = binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "cornell.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1920 / 1080)
    try:
        w, h, spp = FRAME
        a = vc.moments_history()
        b = vc.crafted_filter()
        ses.render(64, 48, 1)                                   # the scene is on every rank's device
        ranks = np.int64(ses.stats().ranks)                     # (read behind the render's own frame: RaylibAMD_GetLastStats completes it)
        ta = [_dev(x) for x in (a[0], a[1], a[2]) + a[3]]
        tb = [_dev(x) for x in b]
        torch.cuda.synchronize()
        st = ses.settings(w, h, spp)
        img = lib.Raylib_CreateImage(w, h)
        lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, img)      # nothing is read: in flight
        out = {}
        acc = binding.temporal_accumulate_moments(lib, a[0], a[1], a[2], a[3], tc.TOL, tc.CAP)
        stats = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(stats))
        out["accumulate_stats"] = np.array([stats.ranks, stats.pixels, stats.rays], np.int64)
        fil = binding.filter_variance(lib, *b, params=PARAMS)
        stats = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(stats))
        out["filter_stats"] = np.array([stats.ranks, stats.pixels, stats.rays, stats.traceLaunches], np.int64)
        for k, v in zip(OUTPUTS, acc + fil):
            out["host_entry_" + k] = np.ascontiguousarray(v).view(np.uint8)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            da = binding.temporal_accumulate_moments_device(lib, ta[0], ta[1], ta[2], tuple(ta[3:]), tc.TOL, tc.CAP)
            df = binding.filter_variance_device(lib, *tb, params=PARAMS)                                       # no host synchronisation between
        s.synchronize()
        for k, v in zip(OUTPUTS, da + df):
            out["device_entry_" + k] = v.cpu().numpy().view(np.uint8)
        frame = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, frame.ctypes.data_as(C.POINTER(C.c_float)))
        lib.Raylib_DestroyImage(img)
        out["frame"] = frame
        out["ranks"] = ranks
        return out
    finally:
        ses.close()


def main():
    workdir, path = sys.argv[1], sys.argv[2]
    os.environ.setdefault("RAYLIB_QUIET", "1")
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1, "no HIP device"
    lib.RaylibAMD_SetSeed(1)
    np.savez(path, **run(lib, workdir))


if __name__ == "__main__":
    main()
