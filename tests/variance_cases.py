"""What the variance-guided filter's tests share (include/raylib_amd.h statements S1 to S7): tests/test_variance_host.py (no device), tests/test_gpu_variance.py,
tests/variance_rank_child.py and tools/gpu_variance_filter.py.

- S1 and S3 to S6 restated in NumPy with every operation rounded to float32, in the stated order (accumulate_moments_f32, filter_f32).  expf is the host libm's
  through ctypes, one call per weight (tests/lightmap_filter_cases.expf), which tests/test_math_exact.py holds the library's expf_ to bit for bit: the
  restatement is exact, not approximate;
- crafted 37 x 21 planes on tests/temporal_cases.crafted() that reach every branch of the statements (crafted_filter, WANTED_BRANCHES);
- the no-bleed planes, and a dump of the crafted planes for the stand-alone sanitizer program (tools/variance_host_check.cc)."""
import numpy as np

import lightmap_filter_cases as lfc
import temporal_cases as tc
from raylib_amd import binding

F = np.float32
W, H = tc.W, tc.H
EDGE = 13                                  # the column where the two crafted surfaces meet: no multiple of 8 or 16
K5 = [F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16)]
K3 = [F(1) / F(4), F(1) / F(2), F(1) / F(4)]
DEFAULTS = dict(binding.VARIANCE_DEFAULTS)


def _expf(x):
    return F(lfc._EXPF(float(x)))


def luminance(r, g, b):
    return F(F(F(F(0.2126) * F(r)) + F(F(0.7152) * F(g))) + F(F(0.0722) * F(b)))


# ---- S1 (with T7) in float32, operation by operation ----
def accumulate_moments_f32(colour, hit, motion, history, depth_tolerance, max_length):
    """Statements T7 and S1 with every operation rounded to float32.  history: None or (colour, hit, length, moments).  Returns (outColour, outLength, outMoments);
    the first two by tests/temporal_cases.accumulate_f32's own statements, repeated here because the moments ride on its taps and weights."""
    h, w = colour.shape[:2]
    out_c = np.zeros((h, w, 4), F); out_l = np.zeros((h, w), F); out_m = np.zeros((h, w, 2), F)
    tol, cap = F(depth_tolerance), F(max_length)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                c, m, prim = colour[y, x], motion[y, x], int(hit[y, x]["prim"])
                out_c[y, x] = (c[0], c[1], c[2], F(1)); out_l[y, x] = F(1)
                yy = luminance(c[0], c[1], c[2])
                mom = (yy, F(yy * yy))
                out_m[y, x] = mom
                if int(m["status"]) == binding.MOTION_NONE or history is None:
                    continue
                px, py, pt = F(m["prevX"]), F(m["prevY"]), F(m["prevT"])
                fx, fy = np.floor(px), np.floor(py)
                if not (fx >= F(-1) and fx <= F(2147483648.0) and fy >= F(-1) and fy <= F(2147483648.0)):
                    continue
                wx, wy = F(px - fx), F(py - fy)
                ox, oy = F(F(1) - wx), F(F(1) - wy)
                wt = (F(ox * oy), F(wx * oy), F(ox * wy), F(wx * wy))
                bound = F(tol * pt)
                Wsum, S, L, M = F(0), [F(0), F(0), F(0)], F(0), [F(0), F(0)]
                for k in range(4):
                    tx, ty = int(fx) + (k & 1), int(fy) + (k >> 1)
                    if tx < 0 or ty < 0 or tx >= w or ty >= h:
                        continue
                    wk = wt[k]
                    if not wk > 0 or not history[2][ty, tx] > 0 or int(history[1][ty, tx]["prim"]) != prim:
                        continue
                    if int(m["status"]) == binding.MOTION_SURFACE and not (np.abs(F(F(history[1][ty, tx]["t"]) - pt)) <= bound):
                        continue
                    Wsum = F(Wsum + wk)
                    for a in range(3):
                        S[a] = F(S[a] + F(wk * F(history[0][ty, tx, a])))
                    L = F(L + F(wk * F(history[2][ty, tx])))
                    for a in range(2):
                        M[a] = F(M[a] + F(wk * F(history[3][ty, tx, a])))
                if not Wsum > 0:
                    continue
                n1 = F(F(L / Wsum) + F(1))
                npr = n1 if n1 < cap else cap
                for a in range(3):
                    hist = F(S[a] / Wsum)
                    out_c[y, x, a] = F(hist + F(F(c[a] - hist) / npr))
                out_l[y, x] = npr
                for a in range(2):
                    hist = F(M[a] / Wsum)
                    out_m[y, x, a] = F(hist + F(F(mom[a] - hist) / npr))
    return out_c, out_l, out_m


# ---- S3 to S6 in float32, operation by operation ----
def constants(params):
    """S4's invN and invPl as the host computes them once, sigmaLuminance and historyLength as they are."""
    p = dict(DEFAULTS, **(params or {}))
    sn, sp = F(p["sigma_normal"]), F(p["sigma_plane"])
    return int(p["iterations"]), F(p["sigma_luminance"]), F(F(1) / F(sn * sn)), F(F(1) / F(sp * sp)), F(p["history_length"])


def _guide(P, N, p, q, inv_n, inv_pl, note):
    """S4: g = dn + dp."""
    e = [F(N[q][a] - N[p][a]) for a in range(3)]
    dn = F(F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2])) * inv_n)
    d = [F(P[q][a] - P[p][a]) for a in range(3)]
    dd = F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))
    nd = F(F(F(N[p][0] * d[0]) + F(N[p][1] * d[1])) + F(N[p][2] * d[2]))
    if dd == 0:
        note("d = 0")
        dp = F(0)
    else:
        dp = F(F(F(nd * nd) / dd) * inv_pl)
    return F(dn + dp)


def filter_f32(colour, moments, length, hit, surface, params=None, census=None):
    """Statements S3 to S6 with every operation rounded to float32.  census: a dict that receives, per branch name, how often it was taken.  Returns
    (outColour (h, w, 4), outVariance (h, w))."""
    h, w = colour.shape[:2]
    K, sig_l, inv_n, inv_pl, hl = constants(params)
    seen = census if census is not None else {}

    def note(k, n=1):
        seen[k] = seen.get(k, 0) + n
    part = np.asarray(hit["prim"]).reshape(h, w) != -1
    P = np.asarray(surface["p"], F).reshape(h, w, 3); N = np.asarray(surface["n"], F).reshape(h, w, 3)
    Pl = [[tuple(F(v) for v in P[y, x]) for x in range(w)] for y in range(h)]
    Nl = [[tuple(F(v) for v in N[y, x]) for x in range(w)] for y in range(h)]
    flatP = [Pl[y][x] for y in range(h) for x in range(w)]; flatN = [Nl[y][x] for y in range(h) for x in range(w)]
    g = lambda p, q: _guide(flatP, flatN, p, q, inv_n, inv_pl, note)
    I = np.where(np.isfinite(colour[..., :3]), colour[..., :3], F(0)).astype(F)
    if not np.isfinite(colour[..., :3]).all():
        note("colour channel not finite", int((~np.isfinite(colour[..., :3])).sum()))
    var = np.zeros((h, w), F)
    mom = np.asarray(moments, F).reshape(h, w, 2); ln = np.asarray(length, F).reshape(h, w)
    with np.errstate(all="ignore"):
        # S5
        for y in range(h):
            for x in range(w):
                if not part[y, x]:
                    note("sky centre"); continue
                if ln[y, x] >= hl:
                    note("temporal variance")
                    v = F(mom[y, x, 1] - F(mom[y, x, 0] * mom[y, x, 0]))
                else:
                    note("spatial variance")
                    sw = s1 = s2 = F(0)
                    for dy in range(-3, 4):
                        for dx in range(-3, 4):
                            qx, qy = x + dx, y + dy
                            if qx < 0 or qy < 0 or qx >= w or qy >= h:
                                note("tap off the frame"); continue
                            if not part[qy, qx]:
                                note("sky tap"); continue
                            wq = _expf(-g(y * w + x, qy * w + qx))
                            sw = F(sw + wq); s1 = F(s1 + F(wq * mom[qy, qx, 0])); s2 = F(s2 + F(wq * mom[qy, qx, 1]))
                    m1, m2 = F(s1 / sw), F(s2 / sw)
                    v = F(m2 - F(m1 * m1))
                if not v > 0:
                    note("clamp at 0"); v = F(0)
                if not ln[y, x] >= hl:
                    v = F(v * F(hl / (ln[y, x] if ln[y, x] > 1 else F(1))))
                var[y, x] = v
        # S6
        for i in range(K):
            s = 1 << i
            J, nvar = I.copy(), var.copy()
            for y in range(h):
                for x in range(w):
                    if not part[y, x]:
                        continue
                    gw = gs = F(0)
                    for dy in range(-1, 2):
                        for dx in range(-1, 2):
                            qx, qy = x + dx, y + dy
                            if qx < 0 or qy < 0 or qx >= w or qy >= h or not part[qy, qx]:
                                continue
                            k = F(K3[dx + 1] * K3[dy + 1])
                            gw = F(gw + k); gs = F(gs + F(k * var[qy, qx]))
                    gv = F(gs / gw)
                    lam = F(F(1) / F(F(sig_l * np.sqrt(gv, dtype=F)) + F(1e-6)))
                    yp = luminance(*I[y, x])
                    sw, sc, sv, taps = F(0), [F(0), F(0), F(0)], F(0), 0
                    for dy in range(-2, 3):
                        qy = y + s * dy
                        if qy < 0 or qy >= h:
                            note("tap off the frame", 5)
                            if i == K - 1:
                                note("tap row off the frame at the largest step")
                            continue
                        for dx in range(-2, 3):
                            qx = x + s * dx
                            if qx < 0 or qx >= w:
                                note("tap off the frame"); continue
                            if not part[qy, qx]:
                                note("sky tap"); continue
                            taps += 1
                            dl = F(np.abs(F(luminance(*I[qy, qx]) - yp)) * lam)
                            wq = F(F(K5[dx + 2] * K5[dy + 2]) * _expf(-F(dl + g(y * w + x, qy * w + qx))))
                            sw = F(sw + wq)
                            for a in range(3):
                                sc[a] = F(sc[a] + F(wq * I[qy, qx, a]))
                            sv = F(sv + F(F(wq * wq) * var[qy, qx]))
                    if taps == 1 and i == K - 1:
                        note("only the centre tap at the largest step")
                    for a in range(3):
                        J[y, x, a] = F(sc[a] / sw)
                    nvar[y, x] = F(sv / F(sw * sw))
            I, var = J, nvar
    out = np.ones((h, w, 4), F); out[..., :3] = I
    return out, var


WANTED_BRANCHES = ("sky centre", "sky tap", "temporal variance", "spatial variance", "tap off the frame", "d = 0", "clamp at 0", "colour channel not finite",
                   "tap row off the frame at the largest step")
# ... and at K = 6, where the step of 32 exceeds the 21 rows and, for the columns 5 .. 31, the 37 columns on both sides:
WANTED_AT_K6 = ("only the centre tap at the largest step",)


def surface_plane(prim, P, N):
    """SURFACE_DTYPE records as the G-buffer writes them, from a prim plane (-1: a miss, zeros with material -1), positions and normals."""
    h, w = prim.shape
    s = np.zeros((h, w), binding.SURFACE_DTYPE)
    on = prim != -1
    s["hit"] = on; s["t"] = np.where(on, F(2), F(0))
    s["p"] = np.where(on[..., None], P, F(0)); s["n"] = np.where(on[..., None], N, F(0))
    s["material"] = np.where(on, 0, -1)
    return s


def crafted_filter(seed=7, w=W, h=H):
    """(colour, moments, length, hit, surface) on tests/temporal_cases.crafted(): its history's colour and flat prim regions (some of them sky); a floor z = 0 left of
    column EDGE and a wall x = const right of it -- perpendicular normals --, both with bumps off their planes so that dp is not 0; two pixels at one position
    (d = 0 off the centre); lengths from {0, 1, 2.5, 4, 8}; moments around the colour's luminance with m2 below m1^2 in places; an inf and a NaN channel."""
    _, _, _, (hist_colour, hist_hit, _) = tc.crafted(seed, w, h)
    rng = np.random.RandomState(seed + 100)
    ys, xs = np.mgrid[0:h, 0:w]
    colour = hist_colour.copy()
    colour[5, 7, 1] = np.inf; colour[10, 20, 0] = np.nan
    hit = hist_hit.copy()
    floor = xs < EDGE
    bump = rng.uniform(-0.02, 0.02, (h, w)).astype(F)
    P = np.zeros((h, w, 3), F); N = np.zeros((h, w, 3), F)
    P[..., 0] = np.where(floor, xs * F(0.1), F(EDGE * 0.1) + bump); P[..., 1] = ys * F(0.1); P[..., 2] = np.where(floor, bump, (xs - EDGE) * F(0.1))
    N[..., 2] = floor; N[..., 0] = ~floor
    P[8, 4] = P[8, 5]                                             # d = 0 between two neighbours
    length = rng.choice(np.asarray([0, 1, 2.5, 4, 8], F), (h, w)).astype(F)
    y_ = np.vectorize(luminance, otypes=[F])(np.nan_to_num(colour[..., 0], posinf=0), np.nan_to_num(colour[..., 1], posinf=0), colour[..., 2])
    m1 = (y_ + rng.uniform(-0.3, 0.3, (h, w))).astype(F)
    m2 = (m1 * m1 + rng.uniform(-0.2, 0.6, (h, w))).astype(F)
    moments = np.stack([m1, m2], -1).astype(F)
    return colour, moments, length, hit, surface_plane(hit["prim"], P, N)


def no_bleed_planes(w=W, h=H):
    """Two half-frames of colour exactly 0 and exactly 1 with perpendicular normals, meeting at column EDGE; moments of a converged history, length 8."""
    ys, xs = np.mgrid[0:h, 0:w]
    left = xs < EDGE
    colour = np.ones((h, w, 4), F); colour[left, :3] = 0
    y1 = luminance(1, 1, 1)
    moments = np.zeros((h, w, 2), F); moments[~left] = (y1, F(y1 * y1))
    length = np.full((h, w), 8, F)
    hit = np.zeros((h, w), binding.HITT_DTYPE); hit["t"] = 2; hit["prim"] = np.where(left, 3, 4)
    P = np.zeros((h, w, 3), F); N = np.zeros((h, w, 3), F)
    P[..., 0] = np.where(left, xs * F(0.1), F(EDGE * 0.1)); P[..., 1] = ys * F(0.1); P[..., 2] = np.where(left, F(0), (xs - EDGE) * F(0.1))
    N[..., 2] = left; N[..., 0] = ~left
    return colour, moments, length, hit, surface_plane(hit["prim"], P, N), left


def moments_history(seed=7):
    """tests/temporal_cases.crafted() with a moments plane in its history: (colour, hit, motion, (colour, hit, length, moments))."""
    colour, hit, motion, history = tc.crafted(seed)
    rng = np.random.RandomState(seed + 200)
    return colour, hit, motion, history + (rng.uniform(0, 6, (H, W, 2)).astype(F),)


def dump(path, seed=7):
    """The crafted planes of both calls as one flat little-endian file for tools/variance_host_check.cc: the words W, H, then the accumulation's colour, hit,
    motion, history colour, hit, length, moments, then the filter's colour, moments, length, hit, surface."""
    a = moments_history(seed)
    b = crafted_filter(seed)
    with open(path, "wb") as f:
        f.write(np.asarray([W, H], np.uint32).tobytes())
        for arr in (a[0], a[1], a[2]) + a[3] + b:
            f.write(np.ascontiguousarray(arr).tobytes())


def identity_motion(hit):
    """A motion plane that sends every pixel to itself, at the t its hit record holds."""
    h, w = hit.shape
    ys, xs = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), binding.MOTION_DTYPE)
    m["prevX"], m["prevY"] = xs, ys
    m["prevT"] = np.where(hit["prim"] >= 0, hit["t"], 0); m["status"] = np.where(hit["prim"] >= 0, binding.MOTION_SURFACE, binding.MOTION_SKY)
    return m


def quality(lib, ses, frame, w=64, h=40, frames=8, first_seed=10, reference_spp=1024):
    """(mse of the accumulated frame, mse of the filtered frame) against a reference_spp frame: `frames` 1-spp frames of the session's scene under the seeds
    first_seed, first_seed + 1, ..., accumulated with moments under identity motion and filtered with the defaults, on the device.  frame(lib, ses, seed, w, h, spp)
    renders one row-major (h, w, 4) frame."""
    gb = binding.gbuffer(lib, ses.scene, ses.camera, w, h, 1e-4, ("hit", "surface"))
    motion = identity_motion(gb["hit"])
    hist = None
    for k in range(frames):
        acc = binding.temporal_accumulate_moments(lib, frame(lib, ses, first_seed + k, w, h, 1), gb["hit"], motion, hist, 0.02, 32)
        hist = (acc[0], gb["hit"], acc[1], acc[2])
    out, _ = binding.filter_variance(lib, acc[0], acc[2], acc[1], gb["hit"], gb["surface"])
    ref = frame(lib, ses, 1, w, h, reference_spp)[..., :3].astype(np.float64)
    mse = lambda a: float(((a[..., :3].astype(np.float64) - ref) ** 2).mean())
    return mse(acc[0]), mse(out)
