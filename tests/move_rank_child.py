"""Child process of tests/test_gpu_move_ranks.py: a move straight behind a multi-rank Raylib_Render whose frame is still in flight.  The library reads the rank
layout once, when it initialises, so every layout needs its own process (tests/rank0_entries_child.py's pattern).

The Cornell scene and a copy of it with some vertices shifted (the oracle: loaded from the edited file under the same layout).  Per entry (host, device): the
large frame of the unmoved scene into image A -- nothing is read --, the move at once, a small frame of the moved scene, then A's pixels; then the move back.

usage: python move_rank_child.py <workdir> <out.npz>"""
import ctypes as C
import os
import sys

import numpy as np
import torch    # before the library is loaded

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import move_cases as mc  # noqa: E402
from raylib_amd import binding  # noqa: E402

FRAME = (1920, 1080, 2)      # rank0_entries_child.FRAME: still executing when Raylib_Render returns


def main():
    workdir, out_path = sys.argv[1], sys.argv[2]
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1
    lib.RaylibAMD_SetSeed(1)
    obj, _ = helpers.build_case("cornell", os.path.join(workdir, "move_ranks"))
    moved = mc.edit_obj(obj, os.path.join(os.path.dirname(obj), "moved.obj"), lambda k, p: p + np.asarray((0.11, 0.07, -0.13), np.float32) if 8 <= k < 20 else p)
    ses, fresh, origin = mc.case_session(lib, "cornell", obj), mc.case_session(lib, "cornell", moved), mc.case_session(lib, "cornell", obj)
    w, h, spp = FRAME
    out = {"frame": ses.render(w, h, spp), "want_moved": fresh.render(mc.W, mc.H, mc.SPP), "want_origin": ses.render(mc.W, mc.H, mc.SPP)}
    s = ses.stats()
    out["layout"] = np.asarray([s.ranks, s.devices], np.int64)
    st = ses.settings(w, h, spp)
    for device in (False, True):
        tag = "device" if device else "host"
        torch.cuda.synchronize()
        A = lib.Raylib_CreateImage(w, h)
        lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, A)          # the frame of the unmoved scene, in flight
        rc = mc.move_to(lib, ses, fresh, device)[0]                       # the move, at once
        out["rc_" + tag] = np.asarray(rc, np.int64)
        out["moved_" + tag] = ses.render(mc.W, mc.H, mc.SPP)
        got = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(A, got.ctypes.data_as(C.POINTER(C.c_float)))
        out["frame_" + tag] = got
        lib.Raylib_DestroyImage(A)
        out["trees_" + tag] = np.asarray(mc.check_trees(lib, ses.scene), np.int64)
        out["wide_" + tag] = np.asarray(mc.compare_trees(lib, ses.scene), np.int64)      # every copy's wide formats and records, as values
        if rc == 1:
            assert mc.move_to(lib, ses, origin, device)[0] == 1
        out["back_" + tag] = ses.render(mc.W, mc.H, mc.SPP)
    for x in (ses, fresh, origin):
        x.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
