"""RaylibAMD_SceneMoveTriangles straight behind a multi-rank Raylib_Render whose frame is in flight (tests/test_gpu_rank0_entries.py's rule for every rank-0
entry point): the move waits for the frame, which keeps the unmoved scene's pixels, and the next frame is the moved scene's -- on every device's copy of the scene (the two-device layout; RaylibAMD_SceneCheckTrees reads every copy).  One child process per rank layout
(tests/move_rank_child.py); the oracle is a scene loaded from the moved triangles in the same process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch    # before the library is loaded

import helpers

pytestmark = pytest.mark.gpu

LAYOUTS = [
    dict(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0"),
    dict(RAYLIB_NUM_GPUS="2", RAYLIB_GPU_MAP="0,0", RAYLIB_GATHER_SELF="1", RAYLIB_GATHER="peer"),
    # two PHYSICAL devices: run where the box has them, SKIPPED -- and not counted as covered -- where it has one
    dict(RAYLIB_NUM_GPUS="2", RAYLIB_GPU_MAP="0,1", RAYLIB_GATHER="rccl"),
]
LAYOUT_ENV = ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_DEVICE", "RAYLIB_POOL", "RAYLIB_LIB", "RAYLIB_LAZY_REFL")
CHILD_KILL_SECONDS = 300     # a kill limit; the child takes seconds


def same(a, b):
    return a.shape == b.shape and bool(helpers.same(a, b).all())


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda d: "-".join(d.values()).replace(",", ""))
def test_move_behind_a_frame_in_flight(gpu_lib, workdir, layout):
    physical = len(set(layout["RAYLIB_GPU_MAP"].split(",")))
    if torch.cuda.device_count() < physical:
        pytest.skip("needs %d physical devices, %d visible: NOT covered on this box" % (physical, torch.cuda.device_count()))
    out = os.path.join(str(workdir), "move_ranks_%s.npz" % layout["RAYLIB_GPU_MAP"].replace(",", ""))
    env = dict(os.environ)
    for k in LAYOUT_ENV:
        env.pop(k, None)
    env.update(layout)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "move_rank_child.py"), str(workdir), out], env=env, capture_output=True,
                       text=True, timeout=CHILD_KILL_SECONDS)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    A = np.load(out)
    assert tuple(A["layout"]) == (int(layout["RAYLIB_NUM_GPUS"]), physical)
    assert not same(A["want_moved"], A["want_origin"])
    for tag in ("host", "device"):
        assert same(A["frame_" + tag], A["frame"]), "the frame in flight lost pixels to the move (%s entry)" % tag
        assert int(A["rc_" + tag]) == 1 and tuple(A["trees_" + tag]) == (1, 0) and tuple(A["wide_" + tag]) == (1, 0)
        assert same(A["moved_" + tag], A["want_moved"]), tag
        assert same(A["back_" + tag], A["want_origin"]), tag
