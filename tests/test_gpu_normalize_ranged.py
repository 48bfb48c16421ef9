"""The lazy-reflectance unit's normalisations and single square roots without sqrtf's and 1 / x's range guards (csrc/rl_dev_core.h "normalize without the two range
guards", RL_NORMALIZE_RANGED in csrc/rl_render_lazy.hip).  The scalar chain, the guard-free acosf and the voted normalisation are swept on the device
(RaylibAMD_VerifyNormalizeRanged); frames that reach every site's edge -- short half vectors, a direction along the normal, zero and cancelling vertex normals --
must be bit-identical between the lazy hit-queue instance, the lazy ray-queue instance and the eager instance, which keeps every general form."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from helpers import scenes
from test_lazy_refl_host import box_with

pytestmark = pytest.mark.gpu

MODES = {0: "1 / sqrt(x), all 2^32 bit patterns", 1: "acosf on the ranged prologue's interval", 2: "normalize_voted_ on 64 edge and 2^24 generated vectors"}
NONE = (1 << 64) - 1
# (waveTrips is left out: it depends on which wave drew which batch and differs from run to run; the eager instance has no lit paths)
COUNTERS = ("rays", "nodesVisited", "trisTested", "shadedHits", "texFetches", "cameraSamples", "culledSamples", "culledCells", "listedCells", "pixels", "traceLaunches")
W, H, SPP = 64, 48, 4


def _binding():
    from raylib_amd import binding
    return binding


@pytest.mark.parametrize("mode", sorted(MODES))
def test_sweep(gpu_lib, mode):
    """One launch per mode: 0 mismatches on the domain.  Mode 0 also reports where the two chains first part outside the vote's domain -- a pattern the vote refuses;
    mode 2 must have run both sides of the vote."""
    bad, first, outside, count = C.c_uint64(NONE), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert gpu_lib.RaylibAMD_VerifyNormalizeRanged(mode, C.byref(bad), C.byref(first), C.byref(outside), C.byref(count)) == 1
    print("normalize sweep mode %d, %s: %d mismatches%s" % (mode, MODES[mode], bad.value, "" if not bad.value else ", first at 0x%08x" % first.value))
    if mode == 0:
        print("normalize sweep mode 0: outside [2^-101, FLT_MAX] the chains differ at %d patterns, the smallest 0x%08x" % (count.value, outside.value & 0xffffffff))
        if outside.value != NONE:
            assert not (0x0d000000 <= outside.value < 0x7f800000)
    if mode == 2:
        total = 64 + (1 << 24)
        print("normalize sweep mode 2: %d of %d vectors in waves that took the guard-free side" % (count.value, total))
        assert 0 < count.value < total
    assert bad.value == 0


def test_modes_outside_the_list_are_refused(gpu_lib):
    assert gpu_lib.RaylibAMD_VerifyNormalizeRanged(-1, None, None, None, None) == 0
    assert gpu_lib.RaylibAMD_VerifyNormalizeRanged(3, None, None, None, None) == 0


def render_three(ses, lib, monkeypatch, max_path, exact_bits=False):
    """The frame through the lazy hit-queue instance, the lazy ray-queue instance and the eager instance: the same bits, the same work counters."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    out = []
    for name, env, ran in (("hit queue", {"RAYLIB_HIT_QUEUE": "1"}, (1, 1)), ("ray queue", {"RAYLIB_HIT_QUEUE": "0"}, (1, 0)), ("eager", {"RAYLIB_LAZY_REFL": "0"}, (0, 0))):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        img = ses.render(W, H, SPP, max_path=max_path)
        assert (lib.RaylibAMD_LastTraceLazy(), lib.RaylibAMD_LastHitQueue()) == ran, name
        out.append((name, np.ascontiguousarray(img, np.float32), ses.stats()))
        for k in env:
            monkeypatch.delenv(k)
    (_, a, sa) = out[0]
    for name, b, sb in out[1:]:
        differ = (a.view(np.uint32) != b.view(np.uint32)) if exact_bits else ~helpers.same(a, b)
        assert not differ.any(), "%s: %d pixels differ from the hit-queue instance's" % (name, int(differ.any(-1).sum()))
        for k in COUNTERS:
            assert getattr(sa, k) == getattr(sb, k), (name, k, getattr(sa, k), getattr(sb, k))
    assert out[0][2].litPaths == out[1][2].litPaths
    return a, sa


@pytest.mark.parametrize("max_path", [1, 5])
def test_cornell(gpu_lib, workdir, monkeypatch, max_path):
    d = os.path.join(str(workdir), "normalize_ranged"); os.makedirs(d, exist_ok=True)
    ses = _binding().SceneSession(gpu_lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    _, st = render_three(ses, gpu_lib, monkeypatch, max_path)
    assert st.shadedHits >= st.cameraSamples // 2
    ses.close()


@pytest.mark.parametrize("name,pr", [("one", "Pr 1\nPm 1"), ("mid", "Pr 0.125\nPm 0.5"), ("low", "Pr 0.0009765625\nPm 0.75")])
def test_grazing_floor(gpu_lib, workdir, monkeypatch, name, pr):
    """tests/test_gpu_sampler_ranged.py's three floors: the camera 2^-11 above the floor, looking along it.  Wo.z is tiny there, the stretched direction and the
    recomputed half vector wo + wi are short."""
    d = os.path.join(str(workdir), "normalize_ranged"); os.makedirs(d, exist_ok=True)
    y = 2.0 ** -11
    ses = _binding().SceneSession(gpu_lib, box_with(os.path.join(d, "graze_%s.obj" % name), pr=pr), (0, y, 0.96875), (0, y, -1), 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    _, st = render_three(ses, gpu_lib, monkeypatch, 3)
    assert st.shadedHits > st.cameraSamples
    ses.close()


def test_down_the_normal(gpu_lib, workdir, monkeypatch):
    """The camera faces the back wall head-on, roughness 2^-10: the stretched direction (alpha x, alpha y, z) rounds to (., ., 1) over the middle of the frame, so
    1 - z z is an exact 0 in SinThetaL (the vote's general side) and the sampler takes its .9999 branch."""
    d = os.path.join(str(workdir), "normalize_ranged"); os.makedirs(d, exist_ok=True)
    ses = _binding().SceneSession(gpu_lib, box_with(os.path.join(d, "headon.obj"), pr="Pr 0.0009765625\nPm 0.75"), (0, 1, 0.9), (0, 1, -1), 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    _, st = render_three(ses, gpu_lib, monkeypatch, 3)
    assert st.shadedHits > st.cameraSamples
    ses.close()


def degenerate_normals_obj(path):
    """The all-microfacet box with the floor's vertex normals replaced: its first triangle's cancel along an edge (n, -n, n: the interpolated normal passes through
    zero and is arbitrarily short beside it), its second triangle's are zero (a NaN shading normal on every hit, as the reference computes it)."""
    obj = box_with(path)                                      # (writes the .mtl beside it; the .obj is written again below, a `vn` per corner)
    A = scenes.build_arrays(scenes.cornell_objects(scenes.WHITE, scenes.WHITE))
    tri, nrm, owner = A["tri"].astype(np.float64), A["normal"].astype(np.float64), A["owner"]
    floor = [k for k in range(len(tri)) if (tri[k, :, 1] == 0.0).all() and nrm[k, 1] > 0.5][:2]
    assert len(floor) == 2, "no floor triangles found"
    out, last = ["mtllib %s\n" % (os.path.splitext(os.path.basename(obj))[0] + ".mtl")], -1
    for k in range(len(tri)):
        if owner[k] != last:
            last = owner[k]
            out.append("o %s\nusemtl %s\n" % A["objects"][last])
        corner_normals = [nrm[k]] * 3
        if k == floor[0]:
            corner_normals = [nrm[k], -nrm[k], nrm[k]]
        if k == floor[1]:
            corner_normals = [np.zeros(3)] * 3
        for p in tri[k]:
            out.append("v %.9g %.9g %.9g\n" % tuple(p))
        for n in corner_normals:
            out.append("vn %.9g %.9g %.9g\n" % tuple(n))
        out.append("f %s\n" % " ".join("%d//%d" % (3 * k + c + 1, 3 * k + c + 1) for c in range(3)))
    with open(obj, "w") as f:
        f.write("".join(out))
    return obj


def test_degenerate_vertex_normals(gpu_lib, workdir, monkeypatch):
    """Zero and cancelling vertex normals: the surface frame's vote fails and the wave runs the three general normalisations, whose NaN normal the event carries
    as the reference does (a NaN pdf ends the path: the sample is the emission, no NaN reaches the frame).  Frames compared as uint32.  That the degenerate
    triangles were met shows in the frame differing from the same box with its own normals."""
    d = os.path.join(str(workdir), "normalize_ranged"); os.makedirs(d, exist_ok=True)
    ses = _binding().SceneSession(gpu_lib, degenerate_normals_obj(os.path.join(d, "degenerate.obj")), (0, 1, 4), (0, 1, -1), 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1        # (the predicate judges materials: the normals are the scene's to choose)
    img, st = render_three(ses, gpu_lib, monkeypatch, 5, exact_bits=True)
    ses.close()
    ses = _binding().SceneSession(gpu_lib, box_with(os.path.join(d, "regular.obj")), (0, 1, 4), (0, 1, -1), 45.0, W / H)
    monkeypatch.setenv("RAYLIB_POOL", "0")
    regular = np.ascontiguousarray(ses.render(W, H, SPP, max_path=5), np.float32)
    ses.close()
    assert (img.view(np.uint32) != regular.view(np.uint32)).any(), "no pixel saw the degenerate normals"
