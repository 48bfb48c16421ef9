"""Child process of tests/test_gpu_sweep.py::test_behind_a_multi_rank_frame_in_flight (modelled on tests/overlap_rank_child.py and tests/nearest_rank_child.py):
the library reads RAYLIB_NUM_GPUS / RAYLIB_GPU_MAP once, when it initialises, so a rank layout needs its own process.  Raylib_Render of the Cornell scene at
1920 x 1080, 2 samples -- with several ranks the frame is still in flight when the call returns -- then at once a swept-sphere query through the host entry and
through the device entry on a stream of the caller's; then the oracle's answers and the frame's pixels.

usage: python sweep_rank_child.py <workdir> <out.npz>"""
import ctypes as C
import os
import sys

import numpy as np
import torch    # before the library is loaded

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import sweep_cases as sc  # noqa: E402
from raylib_amd import binding  # noqa: E402

FRAME = (1920, 1080, 2)


def run(lib, workdir):
    d = os.path.join(str(workdir), "sweep_rank_%d" % os.getpid()); os.makedirs(d, exist_ok=True)
    ses = sc.session(lib, helpers.scenes.cornell(os.path.join(d, "cornell.obj"))[0])
    try:
        tris, _ = ses.export_flat()
        q = np.ascontiguousarray(sc.query_set(np.random.RandomState(61), tris, 1000))
        dev = torch.from_numpy(q).cuda()
        w, h, spp = FRAME
        ses.render(64, 48, 1)                                   # the scene is on every rank's device
        ranks = np.int64(ses.stats().ranks)                     # (read behind the render's own frame: RaylibAMD_GetLastStats completes it)
        binding.sweep_spheres(lib, ses.scene, q[:64], sc.CLOSEST)   # ... and the query's tables on rank 0's
        torch.cuda.synchronize()
        st = ses.settings(w, h, spp)
        img = lib.Raylib_CreateImage(w, h)
        lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, img)      # nothing is read: in flight
        out = {"closest_host_entry": binding.sweep_spheres(lib, ses.scene, q, sc.CLOSEST)}
        stats = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(stats))
        assert stats.rays == len(q), "the synchronous query reports its own numbers, not the frame's"
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = binding.sweep_spheres(lib, ses.scene, dev, sc.CLOSEST)
        out["any_host_entry"] = binding.sweep_spheres(lib, ses.scene, q, sc.ANY)
        s.synchronize()
        out["closest_device_entry"] = t.cpu().numpy().view(binding.SWEEP_HIT_DTYPE).reshape(-1)
        frame = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, frame.ctypes.data_as(C.POINTER(C.c_float)))
        lib.Raylib_DestroyImage(img)
        out["frame"] = frame
        out["closest_oracle"] = binding.sweep_spheres(lib, ses.scene, q, sc.CLOSEST, host=True)
        out["any_oracle"] = binding.sweep_spheres(lib, ses.scene, q, sc.ANY, host=True)
        out["ranks"] = ranks
        return {k: (v.view(np.uint32) if getattr(v, "dtype", None) == binding.SWEEP_HIT_DTYPE else v) for k, v in out.items()}
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
