"""Temporal reprojection where no device is needed (include/raylib_amd.h, statements T1 to T8): the two host oracles against NumPy restatements, the planner,
and every refusal that is made before the device is asked for.  A missing export fails these tests (the binding raises on load).

RaylibAMD_TemporalAccumulateHost is held to a float32 restatement of T7 byte for byte.  RaylibAMD_MotionHost is held to a float64 restatement of T2 to T4:
the status exactly wherever float64 is sure of lambda's sign, the floats within tests/temporal_cases.MARGIN (4) times the largest differences measured on the
CPU over these same scenes and cases and recorded in profiles/temporal_accuracy.json (tools/temporal_accuracy.py; measured on the 37 x 21 frame:
prevX 9.1e-6 and prevY 3.2e-6 pixels, prevT 1.7e-7 relative).

(A BVH deeper than 64 levels cannot be had from the builder: that refusal is not reachable from here, as in tests/test_gbuffer_host.py.)"""
import ctypes as C

import numpy as np
import pytest

import helpers
import temporal_cases as tc
from raylib_amd import binding

F = np.float32
W, H = tc.W, tc.H
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def scenes3(lib, workdir):
    s = tc.host_scenes(lib, workdir)
    yield s
    for v in s.values():
        v.close()


# ---- the accumulation oracle ----
def _same(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), "%s: outColour differs in %d pixels" % (what, (helpers.bits(got[0]) != helpers.bits(want[0])).any(-1).sum())
    assert got[1].tobytes() == want[1].tobytes(), "%s: outLength differs in %d pixels" % (what, (helpers.bits(got[1]) != helpers.bits(want[1])).sum())


def test_accumulate_host_on_crafted_planes(lib):
    colour, hit, motion, history = tc.crafted()
    census = {}
    want = tc.accumulate_f32(colour, hit, motion, history, tc.TOL, tc.CAP, census)
    missing = [k for k in tc.WANTED_BRANCHES if not census.get(k)]
    assert not missing, "the crafted planes do not reach: %s (reached: %s)" % (missing, census)
    got = binding.temporal_accumulate(lib, colour, hit, motion, history, tc.TOL, tc.CAP, host=True)
    _same(got, want, "crafted planes")
    assert (got[0][..., 3] == 1).all() and (got[1] >= 1).all() and (got[1] <= tc.CAP).all()
    # no history: the first frame
    first = binding.temporal_accumulate(lib, colour, hit, motion, None, tc.TOL, tc.CAP, host=True)
    _same(first, tc.accumulate_f32(colour, hit, motion, None, tc.TOL, tc.CAP), "no history")
    assert first[0].tobytes() == colour.tobytes() and (first[1] == 1).all()
    # a history of zero lengths is the first frame too
    zero = (history[0], history[1], np.zeros_like(history[2]))
    again = binding.temporal_accumulate(lib, colour, hit, motion, zero, tc.TOL, tc.CAP, host=True)
    assert again[0].tobytes() == colour.tobytes() and (again[1] == 1).all()


def test_accumulate_host_taps_off_each_edge_and_corner(lib):
    """Every pixel of the frame's border looks half a pixel outwards, the corners diagonally: the taps off the frame drop out and the rest are renormalised."""
    rng = np.random.RandomState(3)
    colour = rng.uniform(0, 2, (H, W, 4)).astype(F); colour[..., 3] = 1
    hist_colour = rng.uniform(0, 2, (H, W, 4)).astype(F); hist_colour[..., 3] = 1
    hit = np.zeros((H, W), binding.HITT_DTYPE); hit["t"] = 3; hit["prim"] = 5
    length = np.full((H, W), 2, F)
    ys, xs = np.mgrid[0:H, 0:W]
    motion = np.zeros((H, W), binding.MOTION_DTYPE)
    motion["prevX"] = xs + np.where(xs == 0, -0.5, np.where(xs == W - 1, 0.5, 0.25))
    motion["prevY"] = ys + np.where(ys == 0, -0.5, np.where(ys == H - 1, 0.5, 0.0))
    motion["prevT"] = 3; motion["status"] = binding.MOTION_SURFACE
    census = {}
    want = tc.accumulate_f32(colour, hit, motion, (hist_colour, hit, length), 0.01, 32, census)
    assert census["tap off the frame"] >= 2 * (W + H) and census.get("blend of 1 taps", 0) >= 4 and census.get("blend of 2 taps", 0) > 0
    _same(binding.temporal_accumulate(lib, colour, hit, motion, (hist_colour, hit, length), 0.01, 32, host=True), want, "edges")
    assert (want[1] == 3).all()


def test_accumulate_host_one_pixel_frame(lib):
    colour = np.asarray([[[1, 2, 3, 1]]], F)
    hit = np.zeros((1, 1), binding.HITT_DTYPE); hit[0, 0] = (2, 0, 0, 0)
    for px in (0.0, 0.5, -0.25, 1.0):
        motion = np.zeros((1, 1), binding.MOTION_DTYPE); motion[0, 0] = (px, 0, 2, binding.MOTION_SURFACE)
        history = (np.asarray([[[3, 2, 1, 1]]], F), hit, np.asarray([[4]], F))
        got = binding.temporal_accumulate(lib, colour, hit, motion, history, 0.01, 32, host=True)
        _same(got, tc.accumulate_f32(colour, hit, motion, history, 0.01, 32), "1 x 1 at %g" % px)
        assert got[1][0, 0] == (1 if px == 1.0 else 5)


def test_eight_frames_of_identity_motion_are_the_running_mean(lib):
    rng = np.random.RandomState(11)
    ys, xs = np.mgrid[0:H, 0:W]
    hit = np.zeros((H, W), binding.HITT_DTYPE); hit["t"] = 1.5; hit["prim"] = (xs + ys) % 3 - 1          # surfaces and sky
    motion = np.zeros((H, W), binding.MOTION_DTYPE)
    motion["prevX"], motion["prevY"] = xs, ys
    motion["prevT"] = np.where(hit["prim"] >= 0, 1.5, 0); motion["status"] = np.where(hit["prim"] >= 0, binding.MOTION_SURFACE, binding.MOTION_SKY)
    history, mean = None, None
    for k in range(1, 9):
        frame = rng.uniform(0, 8, (H, W, 4)).astype(F); frame[..., 3] = 1
        out_c, out_l = binding.temporal_accumulate(lib, frame, hit, motion, history, 0.0, 32, host=True)
        mean = frame[..., :3].copy() if mean is None else (mean + (frame[..., :3] - mean) / F(k)).astype(F)      # the incremental mean, in float32
        assert helpers.bits(out_c[..., :3]).tobytes() == helpers.bits(mean).tobytes(), "frame %d" % k
        assert (out_l == k).all() and (out_c[..., 3] == 1).all()
        history = (out_c, hit, out_l)


# ---- the motion oracle ----
def test_motion_host_against_float64(lib, scenes3):
    """Every scene and case of tests/temporal_cases.host_motion_cases; what is measured here is what tools/temporal_accuracy.py recorded."""
    bound = tc.margins()
    seen = set()
    for name, ses in scenes3.items():
        rays = tc.pinhole_rays(lib, ses.camera)
        hit = tc.brute_hits(ses.export_flat()[0], rays)
        assert (hit["prim"] >= 0).sum() > 50
        cases, handles = tc.host_motion_cases(lib, ses)
        try:
            for what, prev, first, pp in cases:
                got = binding.motion_host(lib, ses.scene, ses.camera, W, H, rays, hit, prev, first, pp)
                want = tc.motion_f64(tc.camera19(lib, prev or ses.camera), W, H, rays, hit, first, pp)
                diff, status_ok = tc.motion_differences(got, want)
                print("%s, %s: %s" % (name, what, diff))
                assert status_ok, (name, what)
                for k, v in diff.items():
                    assert v <= bound[k], "%s, %s: %s differs from float64 by %g, the margin is %g" % (name, what, k, v, bound[k])
                none = got["status"] == binding.MOTION_NONE
                assert not (helpers.bits(got["prevX"])[none].any() or helpers.bits(got["prevY"])[none].any() or helpers.bits(got["prevT"])[none].any()), "NONE is +0"
                seen |= set(got["status"].ravel().tolist())
                if what == "camera facing away":
                    assert none.all()
                if what == "same camera, nothing moved":          # a pinhole ray's own pixel, and the t it was found at
                    ys, xs = np.mgrid[0:H, 0:W]
                    on = got["status"] == binding.MOTION_SURFACE
                    assert on.sum() == (hit["prim"] >= 0).sum()
                    assert np.abs(got["prevX"] - xs).max() < 1e-3 and np.abs(got["prevY"] - ys).max() < 1e-3
                    assert np.abs(got["prevT"].ravel() - hit["t"])[on.ravel()].max() < 1e-4
                if what == "triangles moved":
                    k = hit["prim"].astype(np.int64) - first
                    inside = ((hit["prim"] >= 0) & (k >= 0) & (k < len(pp))).reshape(H, W)
                    same = binding.motion_host(lib, ses.scene, ses.camera, W, H, rays, hit)
                    assert inside.any() and (got[inside] != same[inside]).all() and got[~inside].tobytes() == same[~inside].tobytes()
        finally:
            for hnd in handles:
                lib.Raylib_DestroyCamera(hnd)
    assert seen == {binding.MOTION_NONE, binding.MOTION_SURFACE, binding.MOTION_SKY}


def test_motion_host_spheres_cubes_are_where_the_ray_found_them(lib, scenes3):
    """A record whose prim is a sphere's or a cube's takes the ray's point, whatever the range says."""
    ses = scenes3["cornell"]
    rays = tc.pinhole_rays(lib, ses.camera)
    hit = tc.brute_hits(ses.export_flat()[0], rays)
    first, pp = tc.partial_move(ses.export_flat()[0])
    other = hit.copy()
    on = other["prim"] >= 0
    other["prim"][on] = binding.PRIM_SPHERE | 1
    got = binding.motion_host(lib, ses.scene, ses.camera, W, H, rays, other, None, first, pp)
    want = binding.motion_host(lib, ses.scene, ses.camera, W, H, rays, hit)
    assert got.tobytes() == want.tobytes()


# ---- the planner and the refusals ----
@pytest.mark.parametrize("tree", [None, "2", "4", "8"])
def test_plan_is_the_gbuffers(lib, scenes3, monkeypatch, tree):
    if tree is None:
        monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    else:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
    for name, ses in scenes3.items():
        assert binding.plan_motion(lib, ses.scene) == binding.plan_gbuffer(lib, ses.scene), name
    raw = lib.Raylib_CreateScene()
    try:
        p = binding.QueryPlan()
        assert lib.RaylibAMD_PlanMotion(None, C.byref(p)) == 0 and lib.RaylibAMD_PlanMotion(ses.scene, None) == 0 and lib.RaylibAMD_PlanMotion(raw, C.byref(p)) == 0
    finally:
        lib.Raylib_DestroyScene(raw)


def test_motion_refusals_write_nothing(lib, scenes3):
    """T6, the refusals that need no device, through the host and the device entry and, where they apply, the oracle: 0, and the sentinel planes are untouched."""
    ses = scenes3["cornell"]
    n = lib.RaylibAMD_SceneNumTriangles(ses.scene)
    raw = lib.Raylib_CreateScene()
    gone = lib.Raylib_CreateCamera(); lib.Raylib_DestroyCamera(gone)
    ok = binding.RendererSettings(W, H, 1, 1, 1e-4, 0)
    bufs = {k: np.full(W * H * 16, SENTINEL, np.uint8) for k in ("hit", "motion")}
    planes = binding.MotionPlanes(**{k: v.ctypes.data for k, v in bufs.items()})
    pos = np.zeros((4, 9), F)
    bad = pos.copy(); bad[2, 5] = np.inf
    nan = pos.copy(); nan[0, 0] = np.nan
    prm = lambda cam=None, first=0, count=0, p=None: binding.MotionParams(cam, first, count, None if p is None else p.ctypes.data)
    good = prm()
    st = lambda w=W, h=H, tmin=1e-4: C.byref(binding.RendererSettings(w, h, 1, 1, tmin, 0))
    cases = {
        "null settings": (None, ses.scene, ses.camera, C.byref(good), C.byref(planes)),
        "null scene": (C.byref(ok), None, ses.camera, C.byref(good), C.byref(planes)),
        "null camera": (C.byref(ok), ses.scene, None, C.byref(good), C.byref(planes)),
        "null params": (C.byref(ok), ses.scene, ses.camera, None, C.byref(planes)),
        "null planes": (C.byref(ok), ses.scene, ses.camera, C.byref(good), None),
        "no plane asked for": (C.byref(ok), ses.scene, ses.camera, C.byref(good), C.byref(binding.MotionPlanes())),
        "W = 0": (st(w=0), ses.scene, ses.camera, C.byref(good), C.byref(planes)),
        "H = 0": (st(h=0), ses.scene, ses.camera, C.byref(good), C.byref(planes)),
        "W * H = 2^31": (st(1 << 16, 1 << 15), ses.scene, ses.camera, C.byref(good), C.byref(planes)),
        "rayTMin NaN": (st(tmin=float("nan")), ses.scene, ses.camera, C.byref(good), C.byref(planes)),
        "rayTMin inf": (st(tmin=float("inf")), ses.scene, ses.camera, C.byref(good), C.byref(planes)),
        "scene not finalized": (C.byref(ok), raw, ses.camera, C.byref(good), C.byref(planes)),
        "first < 0": (C.byref(ok), ses.scene, ses.camera, C.byref(prm(first=-1, count=4, p=pos)), C.byref(planes)),
        "count < 0": (C.byref(ok), ses.scene, ses.camera, C.byref(prm(first=0, count=-1, p=pos)), C.byref(planes)),
        "a range past the scene's triangles": (C.byref(ok), ses.scene, ses.camera, C.byref(prm(first=n - 3, count=4, p=pos)), C.byref(planes)),
        "first past the end with count 0": (C.byref(ok), ses.scene, ses.camera, C.byref(prm(first=n + 1, count=0)), C.byref(planes)),
        "first + count overflows": (C.byref(ok), ses.scene, ses.camera, C.byref(prm(first=2 ** 31 - 1, count=2 ** 31 - 1, p=pos)), C.byref(planes)),
        "count > 0 with null positions": (C.byref(ok), ses.scene, ses.camera, C.byref(prm(first=0, count=4)), C.byref(planes)),
        "an unknown previous camera": (C.byref(ok), ses.scene, ses.camera, C.byref(prm(cam=gone)), C.byref(planes)),
    }
    host_only = {
        "an infinite previous position": (C.byref(ok), ses.scene, ses.camera, C.byref(prm(first=1, count=4, p=bad)), C.byref(planes)),
        "a NaN previous position": (C.byref(ok), ses.scene, ses.camera, C.byref(prm(first=1, count=4, p=nan)), C.byref(planes)),
    }
    rays = tc.pinhole_rays(lib, ses.camera)
    hit = tc.brute_hits(ses.export_flat()[0], rays)
    out = np.full(W * H * 16, SENTINEL, np.uint8)
    try:
        for what, args in cases.items():
            assert lib.RaylibAMD_RenderMotion(*args) == 0, what
            assert lib.RaylibAMD_RenderMotionDevice(*args, None) == 0, what
        for what, args in host_only.items():
            assert lib.RaylibAMD_RenderMotion(*args) == 0, what
        # the oracle: its own arguments, and the params' refusals
        mh = lambda w, h, scene, cam, p, r, ht, o: lib.RaylibAMD_MotionHost(w, h, scene, cam, p, r, ht, o)
        r_, h_, o_ = rays.ctypes.data, hit.ctypes.data, out.ctypes.data
        oracle = {"null scene": (W, H, None, ses.camera, C.byref(good), r_, h_, o_), "null camera": (W, H, ses.scene, None, C.byref(good), r_, h_, o_),
                  "null params": (W, H, ses.scene, ses.camera, None, r_, h_, o_), "null rays": (W, H, ses.scene, ses.camera, C.byref(good), None, h_, o_),
                  "null hit": (W, H, ses.scene, ses.camera, C.byref(good), r_, None, o_), "null out": (W, H, ses.scene, ses.camera, C.byref(good), r_, h_, None),
                  "W = 0": (0, H, ses.scene, ses.camera, C.byref(good), r_, h_, o_), "W * H = 2^31": (1 << 16, 1 << 15, ses.scene, ses.camera, C.byref(good), r_, h_, o_),
                  "scene not finalized": (W, H, raw, ses.camera, C.byref(good), r_, h_, o_)}
        for what in ("first < 0", "count < 0", "a range past the scene's triangles", "first + count overflows", "count > 0 with null positions", "an unknown previous camera"):
            oracle[what] = (W, H, ses.scene, ses.camera, cases[what][3], r_, h_, o_)
        for what in host_only:
            oracle[what] = (W, H, ses.scene, ses.camera, host_only[what][3], r_, h_, o_)
        for what, args in oracle.items():
            assert mh(*args) == 0, what
        for k, v in bufs.items():
            assert (v == SENTINEL).all(), k
        assert (out == SENTINEL).all()
    finally:
        lib.Raylib_DestroyScene(raw)


def test_accumulate_refusals_write_nothing(lib):
    """T8, the refusals that need no device, through all three entries."""
    colour, hit, motion, history = tc.crafted()
    out_c, out_l = np.full((H, W, 4), 7, F), np.full((H, W), 7, F)
    frame = binding.TemporalFrame(*[a.ctypes.data for a in history])
    P = lambda tol=0.02, cap=32.0: C.byref(binding.TemporalParams(tol, cap))
    c_, h_, m_, oc, ol = colour.ctypes.data, hit.ctypes.data, motion.ctypes.data, out_c.ctypes.data, out_l.ctypes.data
    part = lambda **kw: C.byref(binding.TemporalFrame(**dict(dict(colour=history[0].ctypes.data, hit=history[1].ctypes.data, length=history[2].ctypes.data), **kw)))
    cases = {
        "null params": (W, H, None, c_, h_, m_, C.byref(frame), oc, ol),
        "null colour": (W, H, P(), None, h_, m_, C.byref(frame), oc, ol),
        "null hit": (W, H, P(), c_, None, m_, C.byref(frame), oc, ol),
        "null motion": (W, H, P(), c_, h_, None, C.byref(frame), oc, ol),
        "null outColour": (W, H, P(), c_, h_, m_, C.byref(frame), None, ol),
        "null outLength": (W, H, P(), c_, h_, m_, C.byref(frame), oc, None),
        "a history without colour": (W, H, P(), c_, h_, m_, part(colour=None), oc, ol),
        "a history without hit": (W, H, P(), c_, h_, m_, part(hit=None), oc, ol),
        "a history without length": (W, H, P(), c_, h_, m_, part(length=None), oc, ol),
        "W = 0": (0, H, P(), c_, h_, m_, C.byref(frame), oc, ol),
        "H = 0": (W, 0, P(), c_, h_, m_, C.byref(frame), oc, ol),
        "W * H = 2^31": (1 << 16, 1 << 15, P(), c_, h_, m_, C.byref(frame), oc, ol),
        "depthTolerance < 0": (W, H, P(tol=-0.01), c_, h_, m_, C.byref(frame), oc, ol),
        "depthTolerance NaN": (W, H, P(tol=float("nan")), c_, h_, m_, C.byref(frame), oc, ol),
        "depthTolerance inf": (W, H, P(tol=float("inf")), c_, h_, m_, C.byref(frame), oc, ol),
        "maxLength < 1": (W, H, P(cap=0.5), c_, h_, m_, C.byref(frame), oc, ol),
        "maxLength NaN": (W, H, P(cap=float("nan")), c_, h_, m_, C.byref(frame), oc, ol),
        "maxLength inf": (W, H, P(cap=float("inf")), c_, h_, m_, C.byref(frame), oc, ol),
        "outColour is the history's colour": (W, H, P(), c_, h_, m_, part(colour=oc), oc, ol),
        "outLength is the history's length": (W, H, P(), c_, h_, m_, part(length=ol), oc, ol),
    }
    for what, args in cases.items():
        assert lib.RaylibAMD_TemporalAccumulateHost(*args) == 0, what
        assert lib.RaylibAMD_TemporalAccumulate(*args) == 0, what
        assert lib.RaylibAMD_TemporalAccumulateDevice(*args, None) == 0, what
    assert (out_c == 7).all() and (out_l == 7).all()
    # in place on the pixel's own colour is no race: the oracle takes it
    mine = colour.copy()
    assert lib.RaylibAMD_TemporalAccumulateHost(W, H, P(tc.TOL, tc.CAP), mine.ctypes.data, h_, m_, C.byref(frame), mine.ctypes.data, ol) == 1
    assert mine.tobytes() == tc.accumulate_f32(colour, hit, motion, history, tc.TOL, tc.CAP)[0].tobytes()
