"""Child process of tests/test_gpu_gather_adaptive.py::test_behind_a_multi_rank_frame: under the rank layout of its environment, RaylibAMD_GatherAdaptive straight
behind a Raylib_Render whose frame is still in flight (tests/rank0_entries_child.py's large frame).

usage: gather_adaptive_child.py WORKDIR IN.npz OUT.npz     IN: points, threshold, kind, cap, pass_samples, min_samples"""
import ctypes as C
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the library is loaded, as in the parent)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
from raylib_amd import binding  # noqa: E402

FRAME = ("cornell", 1920, 1080, 2)


def dump(lib, img, w, h):
    out = np.zeros((h, w, 4), np.float32)
    lib.RaylibAMD_DumpImageRGBA(img, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def last_stats(lib):
    s = binding.Stats()
    lib.RaylibAMD_GetLastStats(C.byref(s))
    return s


def main(workdir, src, dst):
    os.environ.setdefault("RAYLIB_QUIET", "1")
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1
    lib.RaylibAMD_SetSeed(1)
    arg = np.load(src)
    name, w, h, spp = FRAME
    frame_ses = helpers.session_for_case(lib, name, workdir)
    ses = helpers.session_for_case(lib, "cutout_sky", workdir)
    frame = frame_ses.render(w, h, spp)                                  # rendered and read with nothing in between
    control_ranks = last_stats(lib).ranks
    # the scene's upload and trees, so that the call behind the frame is the passes alone
    binding.gather(lib, ses.scene, np.ascontiguousarray(arg["points"][:1]), int(arg["kind"]))
    img = lib.Raylib_CreateImage(w, h)
    st = frame_ses.settings(w, h, spp)
    lib.Raylib_Render(C.byref(st), frame_ses.scene, frame_ses.camera, img)     # in flight when this returns
    values, counts = binding.gather_adaptive(lib, ses.scene, arg["points"], int(arg["kind"]), float(arg["threshold"]), int(arg["min_samples"]), int(arg["pass_samples"]),
                                             sample_count=int(arg["cap"]))
    s = last_stats(lib)
    got = dump(lib, img, w, h)
    differing = int((~helpers.same(got, frame).all(-1)).sum())
    np.savez(dst, values=values, counts=counts, stats=np.asarray([s.ranks, s.cameraSamples], np.int64), control_ranks=np.int64(control_ranks),
             frame_pixels_differing=np.int64(differing))
    lib.Raylib_DestroyImage(img)
    ses.close()
    frame_ses.close()


if __name__ == "__main__":
    main(*sys.argv[1:4])
