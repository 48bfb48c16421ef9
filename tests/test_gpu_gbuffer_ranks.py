"""The G-buffer entries behind a multi-rank frame in flight (the pattern of tests/test_gpu_rank0_entries.py): tests/gbuffer_rank_child.py in a fresh process per
rank layout enqueues a multi-rank Raylib_Render and calls the host and the device entry at once.  The planes equal this process's one-rank planes bit for bit,
the frame's pixels are unharmed, and the stats are the G-buffer call's, with ranks = 1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch    # before the library is loaded

import gbuffer_rank_child as child
import helpers
from raylib_amd import binding

pytestmark = pytest.mark.gpu

LAYOUTS = [
    dict(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0"),
    dict(RAYLIB_NUM_GPUS="2", RAYLIB_GPU_MAP="0,0", RAYLIB_GATHER_SELF="1", RAYLIB_GATHER="peer"),
    # two PHYSICAL devices: run where the box has them, SKIPPED -- and not counted as covered -- where it has one
    dict(RAYLIB_NUM_GPUS="2", RAYLIB_GPU_MAP="0,1", RAYLIB_GATHER="rccl"),
]
LAYOUT_ENV = ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_DEVICE", "RAYLIB_POOL", "RAYLIB_LIB", "RAYLIB_QUERY_TREE")
CHILD_KILL_SECONDS = 300     # a kill limit; a child takes seconds
# A child that faulted, aborted or hung: nothing more is started on the device by this module -- the remaining layouts fail at once.
TROUBLE = []


def _layout_id(d):
    return "-".join("%s%s" % (k.replace("RAYLIB_", "").lower(), v) for k, v in d.items())


def run_child(layout, workdir):
    if TROUBLE:
        pytest.fail("not started: an earlier child of this module %s" % TROUBLE[0])
    out = os.path.join(str(workdir), "gbuffer_rank_%s.npz" % "_".join(layout.values()).replace(",", ""))
    env = dict(os.environ)
    for k in LAYOUT_ENV:
        env.pop(k, None)
    env.update(layout)
    cmd = [sys.executable, os.path.abspath(child.__file__), str(workdir), out]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_KILL_SECONDS)
    except subprocess.TimeoutExpired as e:
        TROUBLE.append("under %s was killed after %d s" % (_layout_id(layout), CHILD_KILL_SECONDS))
        pytest.fail("the child %s: %s" % (TROUBLE[0], (e.stderr or b"")[-3000:]))
    if r.returncode < 0 or r.returncode in (134, 139):
        TROUBLE.append("under %s ended with return code %d" % (_layout_id(layout), r.returncode))
        pytest.fail("the child %s: %s" % (TROUBLE[0], r.stderr[-3000:]))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return np.load(out)


@pytest.fixture(scope="module")
def one_rank(gpu_lib, workdir):
    """The same sequence on the one-rank library of this process, where nothing is ever in flight."""
    saved = {k: os.environ.pop(k) for k in ("RAYLIB_QUERY_TREE",) if k in os.environ}
    try:
        return child.run(gpu_lib, workdir)
    finally:
        os.environ.update(saved)


def test_the_one_rank_run_is_a_reference(one_rank):
    R = one_rank
    assert int(R["ranks"]) == 1
    hit = R["host_entry_hit"].view(binding.HITT_DTYPE)
    assert (hit["prim"] >= 0).sum() > child.W * child.H // 2 and (R["host_entry_albedo"].view(np.float32) != 0).any()
    assert R["stats"][0] == 1 and R["stats"][1] == R["stats"][2] == child.W * child.H and R["stats"][3] >= child.W * child.H and R["stats"][7] == 8, R["stats"]
    for k in binding.GBUFFER_PLANES:
        assert R["device_entry_" + k].tobytes() == R["host_entry_" + k].tobytes(), k


@pytest.mark.parametrize("layout", LAYOUTS, ids=_layout_id)
def test_behind_a_frame_in_flight(layout, one_rank, workdir):
    need = 1 + max(int(x) for x in layout.get("RAYLIB_GPU_MAP", "0").split(","))
    if torch.cuda.device_count() < need:
        pytest.skip("needs %d physical devices, %d visible: NOT covered on this box" % (need, torch.cuda.device_count()))
    got = run_child(layout, workdir)
    assert int(got["ranks"]) == int(layout["RAYLIB_NUM_GPUS"])          # control: the multi-rank path really ran
    for entry in ("host_entry_", "device_entry_"):
        for k in binding.GBUFFER_PLANES:
            assert got[entry + k].tobytes() == one_rank["host_entry_" + k].tobytes(), entry + k
    assert np.array_equal(got["stats"], one_rank["stats"]) and got["stats"][0] == 1, (got["stats"], one_rank["stats"])
    assert bool(helpers.same(got["frame"], one_rank["frame"]).all()), "the frame in flight behind the G-buffer calls is not the one-rank frame"
