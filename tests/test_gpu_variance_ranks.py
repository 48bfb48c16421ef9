"""The accumulation with moments and the variance-guided filter behind a multi-rank frame in flight (the pattern of tests/test_gpu_gbuffer_ranks.py):
tests/variance_rank_child.py in a fresh process with three logical ranks enqueues a multi-rank Raylib_Render and calls the host and the device entries at once.
Both calls run on rank 0 and give the host oracles' bytes, the frame's pixels are unharmed, and the stats are the calls' own, with ranks = 1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch    # noqa: F401  before the library is loaded

import helpers
import temporal_cases as tc
import variance_cases as vc
import variance_rank_child as child
from raylib_amd import binding

pytestmark = pytest.mark.gpu

LAYOUT = dict(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0")
LAYOUT_ENV = ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_DEVICE", "RAYLIB_POOL", "RAYLIB_LIB", "RAYLIB_QUERY_TREE")
CHILD_KILL_SECONDS = 300     # a kill limit; the child takes seconds


def run_child(workdir):
    out = os.path.join(str(workdir), "variance_rank_3.npz")
    env = dict(os.environ)
    for k in LAYOUT_ENV:
        env.pop(k, None)
    env.update(LAYOUT)
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(workdir), out], env=env, capture_output=True, text=True, timeout=CHILD_KILL_SECONDS)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return np.load(out)


def test_both_calls_behind_a_frame_in_flight(gpu_lib, workdir):
    one = child.run(gpu_lib, workdir)          # the same sequence on the one-rank library of this process, where nothing is ever in flight
    n = child.W * child.H
    assert int(one["ranks"]) == 1
    a, b = vc.moments_history(), vc.crafted_filter()
    want = binding.temporal_accumulate_moments(gpu_lib, a[0], a[1], a[2], a[3], tc.TOL, tc.CAP, host=True) + binding.filter_variance(gpu_lib, *b, params=child.PARAMS, host=True)
    for k, v in zip(child.OUTPUTS, want):
        assert one["host_entry_" + k].tobytes() == np.ascontiguousarray(v).tobytes(), k
        assert one["device_entry_" + k].tobytes() == one["host_entry_" + k].tobytes(), k
    assert one["accumulate_stats"].tolist() == [1, n, 0], one["accumulate_stats"]
    assert one["filter_stats"].tolist() == [1, n, 0, 2 + child.PARAMS["iterations"]], one["filter_stats"]
    got = run_child(workdir)
    assert int(got["ranks"]) == 3                  # control: the multi-rank path really ran
    for entry in ("host_entry_", "device_entry_"):
        for k in child.OUTPUTS:
            assert got[entry + k].tobytes() == one["host_entry_" + k].tobytes(), entry + k
    assert np.array_equal(got["accumulate_stats"], one["accumulate_stats"]) and np.array_equal(got["filter_stats"], one["filter_stats"])
    assert bool(helpers.same(got["frame"], one["frame"]).all()), "the frame in flight behind the calls is not the one-rank frame"
