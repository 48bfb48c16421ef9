"""What the temporal-reprojection tests share (include/raylib_amd.h statements T1 to T8): tests/test_temporal_host.py (no device), tests/test_gpu_motion.py,
tests/test_gpu_temporal.py and tools/temporal_accuracy.py.

- the statements restated in NumPy: T2 to T4 in float64 (motion_f64), T7 in float32, operation by operation (accumulate_f32);
- pinhole camera rays from RaylibAMD_CameraExport and a brute-force hit plane over exported triangles, so that RaylibAMD_MotionHost has inputs without a device;
- the camera pairs and moves of the motion tests, and the crafted planes of the accumulation tests;
- the measurement behind profiles/temporal_accuracy.json (measure_accuracy) and its reader (margins)."""
import ctypes as C
import json
import os

import numpy as np

import helpers
from raylib_amd import binding

F = np.float32
W, H = 37, 21                       # partial cells on both edges (the G-buffer tests' frame)
ACCURACY_JSON = os.path.join(helpers.ROOT, "profiles", "temporal_accuracy.json")
MARGIN = 4.0                        # over the measured differences: for scenes a later test adds


# ---- cameras ----
def camera19(lib, camera):
    out = (C.c_float * 19)()
    lib.RaylibAMD_CameraExport(camera, out)
    return np.array(out[:], F)


def pinhole_rays(lib, camera, w=W, h=H):
    """(w * h, 7) float32 in RaylibAMD_EvalCameraRays' layout for a pinhole camera at time 0: origin, the float32 normalised direction through (x / w, y / h), 0.
    (MotionHost reads rays, it does not make them: any rays do, these are the frame's up to rounding.)"""
    c = camera19(lib, camera)
    o, tl, hv, vv = c[0:3], c[4:7], c[7:10], c[10:13]
    assert c[3] == 0.0, "a pinhole camera"
    ys, xs = np.mgrid[0:h, 0:w]
    s = (xs.ravel().astype(F) / F(w))[:, None]
    t = (ys.ravel().astype(F) / F(h))[:, None]
    d = (tl + s * hv + (F(1) - t) * vv - o).astype(F)
    d = (d / np.sqrt((d * d).sum(1, keepdims=True), dtype=F)).astype(F)
    return np.concatenate([np.tile(o, (w * h, 1)), d, np.zeros((w * h, 1), F)], 1).astype(F)


def device_rays(lib, camera, w=W, h=H, seed=1):
    """RaylibAMD_EvalCameraRays for the frame's pixels (needs the device): statement G1's rays."""
    import radiance_cases
    ys, xs = np.mgrid[0:h, 0:w]
    uv = np.stack([np.float32(xs.ravel()) / np.float32(w), np.float32(ys.ravel()) / np.float32(h)], 1).astype(F)
    return radiance_cases.camera_rays(lib, camera, uv, seed)


# ---- a hit plane without a device ----
def brute_hits(tris, rays, tmin=1e-4):
    """The closest triangle per ray by Moeller-Trumbore in float64 over every triangle (tris: an export); HITT_DTYPE records, a miss {0, -1, 0, 0}."""
    v0, v1, v2 = (tris[k].astype(np.float64) for k in ("v0", "v1", "v2"))
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    e1, e2 = v1 - v0, v2 - v0
    out = np.zeros(len(rays), binding.HITT_DTYPE)
    out["prim"] = -1
    best = np.full(len(rays), np.inf)
    for i in range(len(rays)):
        p = np.cross(d[i], e2)
        det = (e1 * p).sum(1)
        ok = np.abs(det) > 1e-14
        inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
        s = o[i] - v0
        u = (s * p).sum(1) * inv
        q = np.cross(s, e1)
        v = (q * d[i]).sum(1) * inv
        t = (q * e2).sum(1) * inv
        ok &= (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin)
        if ok.any():
            k = int(np.argmin(np.where(ok, t, np.inf)))
            out[i] = (t[k], k, u[k], v[k])
            best[i] = t[k]
    return out


# ---- T2 to T4 in float64 ----
def motion_f64(cam19, w, h, rays, hit, first=0, prev_positions=None):
    """Statements T2 to T4 in float64 on float32 inputs.  Returns a dict: prevX, prevY, prevT, status, and `sure` -- the pixels whose lambda is not within 1e-6
    relative of a sign change: |dot(e, w)| > 1e-6 |e| |w| and |dot(a, w)| > 1e-6 |a| |w| (elsewhere float32 may see the other sign)."""
    c = np.asarray(cam19, np.float64)
    po, pc, ph, pv = c[0:3], c[4:7], c[7:10], c[10:13]
    rays = np.asarray(rays, np.float64).reshape(-1, 7)
    hit = np.asarray(hit).reshape(-1)
    o, d = rays[:, 0:3], rays[:, 3:6]
    is_hit = hit["prim"] >= 0
    P = o + hit["t"].astype(np.float64)[:, None] * d
    if prev_positions is not None and len(prev_positions):
        pp = np.asarray(prev_positions, np.float64).reshape(-1, 3, 3)
        k = hit["prim"].astype(np.int64) - first
        moved = is_hit & (hit["prim"] < binding.PRIM_SPHERE) & (k >= 0) & (k < len(pp))
        kk = np.clip(k, 0, len(pp) - 1)
        b1, b2 = hit["b1"].astype(np.float64)[:, None], hit["b2"].astype(np.float64)[:, None]
        Pm = pp[kk, 0] + b1 * (pp[kk, 1] - pp[kk, 0]) + b2 * (pp[kk, 2] - pp[kk, 0])
        P = np.where(moved[:, None], Pm, P)
    e = np.where(is_hit[:, None], P - po, d)
    wv, a = np.cross(ph, pv), pc - po
    num, den = float(a @ wv), e @ wv
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = num / den
        ok = np.isfinite(lam) & (lam > 0)
        q = lam[:, None] * e - a
        s, u = (q @ ph) / (ph @ ph), (q @ pv) / (pv @ pv)
    norm = np.linalg.norm
    sure = (np.abs(den) > 1e-6 * norm(e, axis=1) * norm(wv)) & (abs(num) > 1e-6 * norm(a) * norm(wv))
    status = np.where(ok, np.where(is_hit, binding.MOTION_SURFACE, binding.MOTION_SKY), binding.MOTION_NONE).astype(np.uint32)
    z = lambda v: np.where(ok, v, 0.0)
    return dict(prevX=z(s * w), prevY=z((1.0 - u) * h), prevT=z(np.where(is_hit, norm(e, axis=1), 0.0)), status=status, sure=sure)


def motion_differences(got, want):
    """The largest |prevX|, |prevY| and relative prevT differences of a motion plane (MOTION_DTYPE) against motion_f64's answer, over the pixels both call
    projected; and whether the status agrees wherever it must."""
    got = got.reshape(-1)
    status_ok = bool((got["status"][want["sure"]] == want["status"][want["sure"]]).all())
    both = (got["status"] != binding.MOTION_NONE) & (want["status"] != binding.MOTION_NONE)
    surf = both & (want["status"] == binding.MOTION_SURFACE)
    dx = float(np.abs(got["prevX"][both] - want["prevX"][both]).max()) if both.any() else 0.0
    dy = float(np.abs(got["prevY"][both] - want["prevY"][both]).max()) if both.any() else 0.0
    dt = float((np.abs(got["prevT"][surf] - want["prevT"][surf]) / want["prevT"][surf]).max()) if surf.any() else 0.0
    return dict(prevX=dx, prevY=dy, prevT_rel=dt), status_ok


# ---- the host scenes and cases of the motion oracle ----
def host_scenes(lib, directory):
    d = os.path.join(str(directory), "temporal_host"); os.makedirs(d, exist_ok=True)
    return {"cornell": binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "c.obj"))[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0),
            "cornell_tess4": binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "c4.obj"), tess=4)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0),
            "cutout_sky": helpers.session_for_case(lib, "cutout_sky", os.path.join(d, "sky"))}


def partial_move(tris, shift=(0.11, -0.07, 0.05)):
    """A partial range (first > 0, first + count < n) and the previous positions of its triangles: where they are, shifted."""
    n = len(tris)
    first, end = n // 4, n - n // 3
    assert 0 < first < end < n
    pos = np.concatenate([tris["v0"], tris["v1"], tris["v2"]], 1).astype(F)
    return first, np.ascontiguousarray(pos[first:end] - np.tile(np.asarray(shift, F), 3), F)


def host_motion_cases(lib, ses):
    """(name, previous camera handle or None, first, previous positions or None) for one session; the caller destroys the handles it gets."""
    c19 = camera19(lib, ses.camera)
    origin = tuple(float(x) for x in c19[0:3])
    fwd = np.cross(c19[7:10].astype(np.float64), c19[10:13].astype(np.float64))       # h x v points from the scene to the camera
    fwd = -fwd / np.linalg.norm(fwd)
    right, up = c19[7:10] / np.linalg.norm(c19[7:10]), c19[10:13] / np.linalg.norm(c19[10:13])
    fov = float(np.degrees(2 * np.arctan(0.5 * np.linalg.norm(c19[10:13]) / abs(float((c19[4:7] - c19[0:3]).astype(np.float64) @ fwd)))))
    aspect = float(np.linalg.norm(c19[7:10]) / np.linalg.norm(c19[10:13]))
    moved_o = np.asarray(origin) + 0.3 * right + 0.15 * up - 0.2 * fwd
    moved = binding.create_camera(lib, moved_o, moved_o + fwd - 0.05 * right - 0.03 * up, fov, aspect)
    away = binding.create_camera(lib, origin, np.asarray(origin) - fwd, fov, aspect)
    first, pp = partial_move(ses.export_flat()[0])
    return [("same camera, nothing moved", None, 0, None), ("camera moved", moved, 0, None), ("triangles moved", None, first, pp), ("both", moved, first, pp),
            ("camera facing away", away, 0, None)], (moved, away)


def measure_accuracy(lib, directory):
    """The float32 oracle (RaylibAMD_MotionHost) against motion_f64 over the host scenes and cases, on the CPU: the largest differences."""
    worst = dict(prevX=0.0, prevY=0.0, prevT_rel=0.0)
    per_case = {}
    scenes = host_scenes(lib, directory)
    try:
        for name, ses in scenes.items():
            rays = pinhole_rays(lib, ses.camera)
            hit = brute_hits(ses.export_flat()[0], rays)
            cases, handles = host_motion_cases(lib, ses)
            try:
                for what, prev, first, pp in cases:
                    got = binding.motion_host(lib, ses.scene, ses.camera, W, H, rays, hit, prev, first, pp)
                    want = motion_f64(camera19(lib, prev or ses.camera), W, H, rays, hit, first, pp)
                    diff, status_ok = motion_differences(got, want)
                    assert status_ok, (name, what)
                    per_case["%s: %s" % (name, what)] = diff
                    for k in worst:
                        worst[k] = max(worst[k], diff[k])
            finally:
                for hnd in handles:
                    lib.Raylib_DestroyCamera(hnd)
    finally:
        for s in scenes.values():
            s.close()
    return dict(frame=[W, H], margin=MARGIN, worst=worst, cases=per_case)


def margins():
    """What the tests assert: MARGIN times the differences profiles/temporal_accuracy.json records (tools/temporal_accuracy.py wrote it from measure_accuracy)."""
    with open(ACCURACY_JSON) as f:
        rec = json.load(f)
    assert rec["frame"] == [W, H]
    return {k: MARGIN * float(v) for k, v in rec["worst"].items()}


# ---- T7 in float32, operation by operation ----
def accumulate_f32(colour, hit, motion, history, depth_tolerance, max_length, census=None):
    """Statement T7 with every operation rounded to float32.  colour (h, w, 4), hit (h, w) HITT_DTYPE, motion (h, w) MOTION_DTYPE, history None or (colour, hit,
    length).  census: a dict that receives, per branch name, how many pixels or taps took it.  Returns (outColour, outLength)."""
    h, w = colour.shape[:2]
    out_c = np.zeros((h, w, 4), F); out_l = np.zeros((h, w), F)
    tol, cap = F(depth_tolerance), F(max_length)
    seen = census if census is not None else {}

    def note(k, n=1):
        seen[k] = seen.get(k, 0) + n
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                c, m, prim = colour[y, x], motion[y, x], int(hit[y, x]["prim"])
                out_c[y, x] = (c[0], c[1], c[2], F(1)); out_l[y, x] = F(1)
                if int(m["status"]) == binding.MOTION_NONE:
                    note("status NONE"); continue
                if history is None:
                    note("no history"); continue
                px, py, pt = F(m["prevX"]), F(m["prevY"]), F(m["prevT"])
                fx, fy = np.floor(px), np.floor(py)
                if not (fx >= F(-1) and fx <= F(2147483648.0) and fy >= F(-1) and fy <= F(2147483648.0)):
                    note("far outside"); continue
                wx, wy = F(px - fx), F(py - fy)
                ox, oy = F(F(1) - wx), F(F(1) - wy)
                wt = (F(ox * oy), F(wx * oy), F(ox * wy), F(wx * wy))
                bound = F(tol * pt)
                Wsum, S, L = F(0), [F(0), F(0), F(0)], F(0)
                counted = mismatched = 0
                for k in range(4):
                    tx, ty = int(fx) + (k & 1), int(fy) + (k >> 1)
                    if tx < 0 or ty < 0 or tx >= w or ty >= h:
                        note("tap off the frame"); continue
                    wk = wt[k]
                    if not wk > 0:
                        note("tap of weight 0"); continue
                    if not history[2][ty, tx] > 0:
                        note("tap of length 0"); continue
                    if int(history[1][ty, tx]["prim"]) != prim:
                        mismatched += 1; continue
                    if int(m["status"]) == binding.MOTION_SURFACE and not (np.abs(F(F(history[1][ty, tx]["t"]) - pt)) <= bound):
                        note("tap outside the depth tolerance"); continue
                    if int(m["status"]) == binding.MOTION_SURFACE:
                        note("tap inside the depth tolerance")
                    counted += 1
                    Wsum = F(Wsum + wk)
                    for a in range(3):
                        S[a] = F(S[a] + F(wk * F(history[0][ty, tx, a])))
                    L = F(L + F(wk * F(history[2][ty, tx])))
                if mismatched:
                    note("prim mismatch on %d taps" % mismatched)
                if not Wsum > 0:
                    note("Wsum 0"); continue
                note("blend of %d taps" % counted)
                if prim == -1:
                    note("sky on sky")
                n1 = F(F(L / Wsum) + F(1))
                if not n1 < cap:
                    note("maxLength cap")
                npr = n1 if n1 < cap else cap
                for a in range(3):
                    hist = F(S[a] / Wsum)
                    out_c[y, x, a] = F(hist + F(F(c[a] - hist) / npr))
                out_l[y, x] = npr
    return out_c, out_l


# ---- crafted planes that reach every branch of T7 ----
TOL, CAP = 0.0625, 8.0


def crafted(seed=7, w=W, h=H):
    """(colour, hit, motion, history): a history of flat regions (prim constant over 5 x 4 blocks, some of them sky, t = 2 everywhere on surfaces), lengths from a
    small set with zeros, and per pixel one of a table of motions -- identity, fractional, across region borders (mismatches on 1 to 4 taps), off every edge and
    corner, far outside, NONE -- with prevT at, just inside and just outside the tolerance bound (2 +- 0.125 exactly: TOL is 2^-4)."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    region = (xs // 5 + 3 * (ys // 4)) % 7
    hprim = np.where(region == 3, -1, region * 11).astype(np.int32)
    hist_hit = np.zeros((h, w), binding.HITT_DTYPE)
    hist_hit["prim"] = hprim
    hist_hit["t"] = np.where(hprim >= 0, F(2.0), F(0.0))
    # some history taps sit just inside / just outside the bound of a pixel that looks for t = 2
    edge = rng.randint(0, 6, (h, w))
    hist_hit["t"] = np.where((hprim >= 0) & (edge == 0), F(2.125), hist_hit["t"])
    hist_hit["t"] = np.where((hprim >= 0) & (edge == 1), np.nextafter(F(2.125), F(3)), hist_hit["t"])
    hist_hit["t"] = np.where((hprim >= 0) & (edge == 2), np.nextafter(F(1.875), F(0)), hist_hit["t"])
    hist_colour = rng.uniform(0, 4, (h, w, 4)).astype(F); hist_colour[..., 3] = 1
    hist_len = rng.choice(np.asarray([0, 1, 2.5, 6.75, 7, 7.5, 8], F), (h, w)).astype(F)
    colour = rng.uniform(0, 4, (h, w, 4)).astype(F); colour[..., 3] = 1
    table = [(0, 0), (0.25, 0.5), (-0.5, 0.75), (2.5, 0), (0, -1.75), (-2.0, 2.0), (0.75, 0.25), (4.5, 3.5), (-40.0, 0), (0, 40.0), (1e12, 0), (-0.25, -0.25),
             (0.5, 0.5), (float("nan"), 0), (5.0, 4.0), (-5.0, -4.0)]
    pick = rng.randint(0, len(table), (h, w))
    motion = np.zeros((h, w), binding.MOTION_DTYPE)
    hit = np.zeros((h, w), binding.HITT_DTYPE)
    for y in range(h):
        for x in range(w):
            dx, dy = table[pick[y, x]]
            px, py = F(x + dx), F(y + dy)
            sx, sy = int(np.clip(np.nan_to_num(np.floor(px + F(0.5)), nan=0, posinf=w, neginf=-1), 0, w - 1)), int(np.clip(np.floor(py + F(0.5)), 0, h - 1))
            prim = int(hprim[sy, sx])            # the pixel believes it sees what the history holds nearest to where it looks ...
            if rng.randint(0, 6) == 0:
                prim = 999                       # ... or a surface the history has nowhere: a disocclusion
            status = binding.MOTION_SKY if prim < 0 else binding.MOTION_SURFACE
            if rng.randint(0, 12) == 0:
                status = binding.MOTION_NONE
            motion[y, x] = (px, py, F(2.0) if status == binding.MOTION_SURFACE else F(0), status) if status != binding.MOTION_NONE else (0, 0, 0, 0)
            hit[y, x] = (F(2.0) if prim >= 0 else F(0), prim, 0, 0)
    return colour, hit, motion, (hist_colour, hist_hit, hist_len)


WANTED_BRANCHES = ("status NONE", "far outside", "tap off the frame", "tap of weight 0", "tap of length 0", "prim mismatch on 1 taps", "prim mismatch on 2 taps",
                   "prim mismatch on 3 taps", "prim mismatch on 4 taps", "tap outside the depth tolerance", "tap inside the depth tolerance", "Wsum 0",
                   "blend of 1 taps", "blend of 2 taps", "blend of 3 taps", "blend of 4 taps", "sky on sky", "maxLength cap")
