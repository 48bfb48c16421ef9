"""Child process of tests/test_gpu_ray_query_all.py::test_behind_a_multi_rank_frame_in_flight (modelled on tests/nearest_rank_child.py): the library reads
RAYLIB_NUM_GPUS / RAYLIB_GPU_MAP once, when it initialises, so a rank layout needs its own process.  Raylib_Render of the Cornell scene at 1920 x 1080, 2
samples -- with several ranks the frame is still in flight when the call returns -- then at once an ordered multi-hit query through the host entry and through
the device entry on a stream of the caller's; then the oracle's answers and the frame's pixels.

usage: python ray_query_all_rank_child.py <workdir> <out.npz>"""
import ctypes as C
import os
import sys

import numpy as np
import torch    # before the library is loaded

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import test_gpu_ray_query as base  # noqa: E402
from raylib_amd import binding  # noqa: E402

FRAME = (1920, 1080, 2)
MAX_HITS = 4


def run(lib, workdir):
    d = os.path.join(str(workdir), "ray_query_all_rank_%d" % os.getpid()); os.makedirs(d, exist_ok=True)
    ses = binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "cornell.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    try:
        rays = np.ascontiguousarray(base._random_rays(np.random.RandomState(61), 1000, (-0.9, 0.1, -0.9), (0.9, 1.9, 3.0)))
        dev = torch.from_numpy(rays).cuda()
        w, h, spp = FRAME
        ses.render(64, 48, 1)                                   # the scene is on every rank's device
        ranks = np.int64(ses.stats().ranks)                     # (read behind the render's own frame: RaylibAMD_GetLastStats completes it)
        binding.trace_rays_all(lib, ses.scene, rays[:64], MAX_HITS, count=True)   # ... and the query's tables on rank 0's
        torch.cuda.synchronize()
        st = ses.settings(w, h, spp)
        img = lib.Raylib_CreateImage(w, h)
        lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, img)      # nothing is read: in flight
        out = {}
        out["hits_host_entry"], out["counts_host_entry"] = binding.trace_rays_all(lib, ses.scene, rays, MAX_HITS, count=True)
        stats = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(stats))
        assert stats.rays == len(rays), "the synchronous query reports its own numbers, not the frame's"
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t, tc = binding.trace_rays_all(lib, ses.scene, dev, MAX_HITS, count=True)
        s.synchronize()
        out["hits_device_entry"] = t.cpu().numpy().view(binding.HITT_DTYPE).reshape(len(rays), MAX_HITS)
        out["counts_device_entry"] = tc.cpu().numpy().view(np.uint32)
        frame = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, frame.ctypes.data_as(C.POINTER(C.c_float)))
        lib.Raylib_DestroyImage(img)
        out["frame"] = frame
        out["hits_oracle"], out["counts_oracle"] = binding.trace_rays_all(lib, ses.scene, rays, MAX_HITS, count=True, host=True)
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
    out = run(lib, workdir)
    np.savez(path, **{k: (np.ascontiguousarray(v).view(np.uint32) if v.dtype == binding.HITT_DTYPE else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
