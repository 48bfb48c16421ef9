"""The motion launch and the accumulation behind a multi-rank frame in flight (the pattern of tests/test_gpu_gbuffer_ranks.py): tests/temporal_rank_child.py in a
fresh process with three logical ranks enqueues a multi-rank Raylib_Render and calls the host and the device entries at once.  Both calls run on rank 0 and
give this process's one-rank bytes, the frame's pixels are unharmed, and the stats are the calls' own, with ranks = 1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch    # noqa: F401  before the library is loaded

import helpers
import temporal_rank_child as child
from raylib_amd import binding

pytestmark = pytest.mark.gpu

LAYOUT = dict(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0")
LAYOUT_ENV = ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_DEVICE", "RAYLIB_POOL", "RAYLIB_LIB", "RAYLIB_QUERY_TREE")
CHILD_KILL_SECONDS = 300     # a kill limit; the child takes seconds
PLANES = ("hit", "motion", "colour", "length")


def run_child(workdir):
    out = os.path.join(str(workdir), "temporal_rank_3.npz")
    env = dict(os.environ)
    for k in LAYOUT_ENV:
        env.pop(k, None)
    env.update(LAYOUT)
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(workdir), out], env=env, capture_output=True, text=True, timeout=CHILD_KILL_SECONDS)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return np.load(out)


def test_both_calls_behind_a_frame_in_flight(gpu_lib, workdir):
    saved = {k: os.environ.pop(k) for k in ("RAYLIB_QUERY_TREE",) if k in os.environ}
    try:
        one = child.run(gpu_lib, workdir)          # the same sequence on the one-rank library of this process, where nothing is ever in flight
    finally:
        os.environ.update(saved)
    n = child.W * child.H
    assert int(one["ranks"]) == 1
    m = one["host_entry_motion"].view(binding.MOTION_DTYPE)
    assert (m["status"] == binding.MOTION_SURFACE).sum() > n // 2 and (one["host_entry_length"].view(np.float32) > 1).any()
    assert one["motion_stats"][0] == 1 and one["motion_stats"][1] == one["motion_stats"][2] == one["motion_stats"][3] == n and one["motion_stats"][6] == 8, one["motion_stats"]
    assert one["accumulate_stats"].tolist() == [1, n, 0], one["accumulate_stats"]
    for k in PLANES:
        assert one["device_entry_" + k].tobytes() == one["host_entry_" + k].tobytes(), k
    got = run_child(workdir)
    assert int(got["ranks"]) == 3                  # control: the multi-rank path really ran
    for entry in ("host_entry_", "device_entry_"):
        for k in PLANES:
            assert got[entry + k].tobytes() == one["host_entry_" + k].tobytes(), entry + k
    assert np.array_equal(got["motion_stats"], one["motion_stats"]) and np.array_equal(got["accumulate_stats"], one["accumulate_stats"])
    assert bool(helpers.same(got["frame"], one["frame"]).all()), "the frame in flight behind the calls is not the one-rank frame"
