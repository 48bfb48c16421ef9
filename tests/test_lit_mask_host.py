"""The lit-sample mask without a device: the bit walk and the word indexing of the masked sum (csrc/rl_lit_mask.h LitMaskSum, the statement k_resolve_lit runs)
against the straight loop over every sample, and the switch that turns the mask off."""
import os
import subprocess

import helpers

ROOT = helpers.ROOT


def test_masked_sum_matches_the_straight_loop(tmp_path):
    """tools/lit_mask_host_check.cc compiled with g++ (no FMA contraction, as the library) and run: random masks and values, -0, infinities and NaNs among
    them, stale values in the samples the mask leaves out, two batches through one running sum.  Compared by bits."""
    exe = str(tmp_path / "lit_mask_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "software-raytracing_amd", "csrc"),
                           os.path.join(ROOT, "tools", "lit_mask_host_check.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "MASKED SUM BIT-EXACT" in out.stdout


def test_last_lit_mask_is_exported(lib):
    """Callable without a device; 0 until a lazy launch keeps a mask."""
    assert lib.RaylibAMD_LastLitMask() in (0, 1)
