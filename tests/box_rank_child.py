"""Child process of tests/test_gpu_boxes.py::test_behind_a_multi_rank_frame_in_flight (modelled on tests/overlap_rank_child.py): the library reads
RAYLIB_NUM_GPUS / RAYLIB_GPU_MAP once, when it initialises, so a rank layout needs its own process.  Raylib_Render of the Cornell scene at 1920 x 1080, 2
samples -- with several ranks the frame is still in flight when the call returns -- then at once oriented-box queries through the host entry and through the
device entry on a stream of the caller's; then the oracle's answers and the frame's pixels.

usage: python box_rank_child.py <workdir> <out.npz>"""
import ctypes as C
import os
import sys

import numpy as np
import torch    # before the library is loaded

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import box_cases as bc  # noqa: E402
from raylib_amd import binding  # noqa: E402

FRAME = (1920, 1080, 2)
MAX_HITS = 4


def run(lib, workdir):
    d = os.path.join(str(workdir), "box_rank_%d" % os.getpid()); os.makedirs(d, exist_ok=True)
    ses = bc.session(lib, helpers.scenes.cornell(os.path.join(d, "cornell.obj"))[0])
    try:
        tris, _ = ses.export_flat()
        q = np.ascontiguousarray(bc.query_set(np.random.RandomState(61), tris, 1000))
        lead = np.ascontiguousarray(q[:bc.LEAD])
        dev = torch.from_numpy(q.view(np.float32).reshape(len(q), 16)).cuda()
        dev_lead = torch.from_numpy(lead.view(np.float32).reshape(len(lead), 16)).cuda()
        w, h, spp = FRAME
        ses.render(64, 48, 1)                                   # the scene is on every rank's device
        ranks = np.int64(ses.stats().ranks)                     # (read behind the render's own frame: RaylibAMD_GetLastStats completes it)
        binding.overlap_boxes(lib, ses.scene, q[:64], bc.LIST, MAX_HITS)   # ... and the query's tables on rank 0's
        torch.cuda.synchronize()
        st = ses.settings(w, h, spp)
        img = lib.Raylib_CreateImage(w, h)
        lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, img)      # nothing is read: in flight
        out = {}
        out["rows_host_entry"], out["counts_host_entry"] = binding.overlap_boxes(lib, ses.scene, q, bc.LIST, MAX_HITS)
        stats = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(stats))
        assert stats.rays == len(q), "the synchronous query reports its own numbers, not the frame's"
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t, tc = binding.overlap_boxes(lib, ses.scene, dev, bc.LIST, MAX_HITS)
            tm = binding.overlap_boxes(lib, ses.scene, dev_lead, bc.MARK)
        out["any_host_entry"] = binding.overlap_boxes(lib, ses.scene, q, bc.ANY)
        out["mark_host_entry"] = binding.overlap_boxes(lib, ses.scene, lead, bc.MARK)
        s.synchronize()
        out["rows_device_entry"] = t.cpu().numpy()
        out["counts_device_entry"] = tc.cpu().numpy().view(np.uint32)
        out["mark_device_entry"] = tm.cpu().numpy().view(np.uint32)
        frame = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, frame.ctypes.data_as(C.POINTER(C.c_float)))
        lib.Raylib_DestroyImage(img)
        out["frame"] = frame
        out["rows_oracle"], out["counts_oracle"] = binding.overlap_boxes(lib, ses.scene, q, bc.LIST, MAX_HITS, host=True)
        out["any_oracle"] = binding.overlap_boxes(lib, ses.scene, q, bc.ANY, host=True)
        out["mark_oracle"] = binding.overlap_boxes(lib, ses.scene, lead, bc.MARK, host=True)
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
