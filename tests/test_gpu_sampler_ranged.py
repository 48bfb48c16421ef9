"""The lazy-reflectance instance's Beckmann sampler without the math guards its arguments cannot reach (csrc/rl_dev_shade.h "the ranged sampler",
RL_SAMPLER_RANGED in csrc/rl_render_lazy.hip).  Each ranged piece is a function of one float and is compared with the general form on all 2^32 bit patterns of
it, on the device (RaylibAMD_VerifySamplerRanged); frames that see the floor at a grazing angle must be the eager instance's -- which keeps the general
sampler -- bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_lazy_refl import _binding, render_both
from test_lazy_refl_host import box_with

pytestmark = pytest.mark.gpu

MODES = {0: "loop body (ErfInv(b), exp of minus its square)", 1: "prologue (tan, Erf(cot), fit, normalization of cosThetaI)",
         2: "the .9999 branch as a float compare", 3: "logf / expf / sqrtf _in_range_ over their domains"}


def _f32(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


@pytest.mark.parametrize("mode", sorted(MODES))
def test_sweep(gpu_lib, mode):
    """All 2^32 bit patterns, one launch per mode: 0 mismatches.  Mode 1 also reports the interval of cosThetaI on which the two prologues agree everywhere;
    the C_MIN the library was built with lies inside it, and the interval ends at the last float below the branch."""
    bad, first, outside = C.c_uint64(~0), C.c_uint64(0), C.c_uint64(0)
    iv = (C.c_uint32 * 3)(0, 0, 0)
    assert gpu_lib.RaylibAMD_VerifySamplerRanged(mode, C.byref(bad), C.byref(first), iv, C.byref(outside)) == 1
    print("sampler sweep mode %d, %s: %d mismatches%s" % (mode, MODES[mode], bad.value, "" if not bad.value else ", first at bits 0x%08x" % first.value))
    if mode == 1:
        lo, hi, cmin = iv[0], iv[1], iv[2]
        print("sampler sweep mode 1: the prologues agree on [0x%08x = %.9g, 0x%08x = %.9g]; C_MIN 0x%08x = %.9g; %d inputs outside [C_MIN, .9999] differ"
              % (lo, _f32(lo), hi, _f32(hi), cmin, _f32(cmin), outside.value))
        threshold = np.float32(.9999) if float(np.float32(.9999)) > .9999 else np.nextafter(np.float32(.9999), np.float32(2))
        assert hi == int(threshold.view(np.uint32)) - 1
        assert 0 < lo <= cmin <= hi, (lo, cmin, hi)     # (positive floats order as their bit patterns)
    assert bad.value == 0


def test_modes_outside_the_list_are_refused(gpu_lib):
    assert gpu_lib.RaylibAMD_VerifySamplerRanged(-1, None, None, None, None) == 0
    assert gpu_lib.RaylibAMD_VerifySamplerRanged(4, None, None, None, None) == 0


@pytest.mark.parametrize("name,pr", [("one", "Pr 1\nPm 1"), ("mid", "Pr 0.125\nPm 0.5"), ("low", "Pr 0.0009765625\nPm 0.75")])
def test_grazing_frame(gpu_lib, workdir, monkeypatch, name, pr):
    """The camera 2^-11 above the floor, looking along it: the lower half of the frame meets the floor at grazing angles.  The sampler stretches the outgoing
    direction by the roughness, so its cosThetaI runs from about 1e-3 (roughness 1) up into the .9999 branch (roughness 2^-10) over the three frames.  The
    lazy instance (ranged sampler) against the eager one (general sampler): the same bits, the same counters."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    d = os.path.join(str(workdir), "sampler_ranged_gpu"); os.makedirs(d, exist_ok=True)
    y = 2.0 ** -11
    w, h = 64, 32
    ses = _binding().SceneSession(gpu_lib, box_with(os.path.join(d, "graze_%s.obj" % name), pr=pr), (0, y, 0.96875), (0, y, -1), 45.0, w / h)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    st = render_both(ses, gpu_lib, monkeypatch, w=w, h=h, spp=8, max_path=3)      # (asserts RaylibAMD_LastTraceLazy() == 1 for the first render, 0 for the second)
    assert st.shadedHits > st.cameraSamples
    ses.close()
