"""The scattering event at its degenerate inputs (RaylibAMD_EvalScatter: Scatter / ScatteringPdf / Emitted, csrc/rl_dev_shade.h) against
the oracle, bit for bit, and whole frames of the same materials on every schedule.

In k_trace and the eval hook the event's divisions take a short exact form (rtm::div_by_) behind guards; when a lane fails its guard the
WHOLE wave takes the IEEE divisions through a ballot (rtm::wave_any_).  The records below are built so that each guard fails whatever the
RNG draws:
  - tanThetaI (BeckmannSample11, `cosThetaI >= 2^-126`): the GRAZING family.  d . n == 0 in float32 gives a local Wo.z of +-0, so
    wiStretched.z == 0 = cosThetaI; grazing by a subnormal (2^-140) fails it as well, while 2^-126 and 2^-20 sit just inside it.
  - CosSinPhi (`|w.x|, |w.y| >= 2^-102` unless sinTheta == 0): the ZERO-LOCAL family.  A direction with an exact zero local x or y
    component (and the TINY-LOCAL family, a subnormal or 2^-110 one) keeps it through the stretch, on a rough material sinTheta > 0.
  - DivSpecular (QuotientInRange): NORMAL incidence, d = -n on an axis-aligned normal, on `zero_kd_metal` (Ns 1e30, Ks 1, Pm 1, a zero
    Kd channel): the stretch leaves Wh = (~1e-15, ~1e-15, 1) and Wo = (0, 0, 1), so absDot(Wh, Wo) == 1, pow(0, 5) == 0 and that Fresnel
    channel is F0 = the zero albedo channel: a zero numerator.  On `tiny_kd_metal` (Pr 1e-6, Pm 1, subnormal Kd) the numerators are
    F0 * G * NDF ~ 2^-108 .. 2^-100, quotients below the guard's 2^-91 bound, where div_by_ is no longer exact.  Those products reach
    the reflectance only through F * specular, which underflows; `tiny_ndf` (Pr 7e-4, Pm 1, a normal map leaning 0.0055 rad, 7.4
    roughnesses) makes NDF = exp(-(tan theta_h / alpha)^2) itself tiny at normal incidence, with F ~ 0.9 and no diffuse term: quotients
    on both sides of 2^-91, visible in the reflectance, and most waves of the set keep every lane above 2^-127 (the TINY-NDF set, 4096
    records): a guard bound set too low lets such a wave take the short form where it is not exact.
A guard's fallback only changes bits where the short form and the division differ: a zero's sign or the last bit of a tiny quotient.
CosSinPhi's quotient meets the sampled slopes, which hide such a difference unless a slope is itself zero; the ZERO-LOCAL records are
therefore also run with a seed chosen so that the record's stream draws U2 == 0.5 exactly (slope_y = ErfInv(0) = 0): `seed_for_half`.

Each record set runs in three layouts: every family alone in whole waves of 64; one degenerate record among 63 regular ones at lane 0,
31 and 63; everything shuffled.  The stream of record i is (seed, i, 0) on both sides, so each layout is compared with the oracle run
on the same array: a regular lane must not depend on the degenerate lane of its wave.

CPU part: the float32 restatement of the frame k_eval_scatter builds (T, B, WorldToLocal in the operation order of rl_render.hip k_eval_scatter) proves the
exact zeros the families promise, and the seeds' draws."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from oracle import ffi

F = np.float32

# materials at the extremes MaterialFromMTL (csrc/rl_obj_loader.cc) can express
EDGE_MTL = """newmtl pr_tiny
Kd 0.6 0.5 0.4
Pr 1e-06

newmtl pr_one
Kd 0.6 0.5 0.4
Pr 1

newmtl ns_huge
Kd 0.7 0.6 0.5
Ns 1e+30
Ks 1 1 1

newmtl metal0
Kd 0.3 0.6 0.9
Pr 0.3
Pm 0

newmtl metal1
Kd 0.9 0.6 0.3
Pr 0.3
Pm 1

newmtl zero_kd_metal
Kd 0.5 0 0.25
Ns 1e+30
Ks 1 1 1
Pm 1

newmtl tiny_kd_metal
Kd 1.12103877e-44 2.80259693e-43 7.00649232e-42
Pr 1e-06
Pm 1

newmtl emissive
Kd 0.5 0.5 0.5
Pr 0.5
Ke 4 3 2

newmtl glass10
Kd 0 0 0
Tf 1 1 1
Ni 1
illum 4

newmtl glass24
Kd 0 0 0
Tf 0.9 0.95 1
Ni 2.4
illum 4

newmtl mirror
Kd 0.9 0.9 0.9
illum 3

newmtl light
Kd 0.78 0.78 0.78
Pr 1
Ke 17 12 4
"""
MAPPED_MTL = """newmtl mapped
Kd 0.5 0.5 0.5
Pm 0.5
map_Kd bw.png
map_Pr bw.png

newmtl tiny_ndf
Kd 0.9 0.8 0.7
Pm 1
Pr 0.0007
norm tilt.png
"""
ROUGH = ("pr_one", "metal0", "metal1", "emissive", "mapped")          # sinTheta > 0 for an oblique direction: CosSinPhi runs its test


def tilt_texture():
    """One texel (128, 128, 255): the microsurface normal normalize(1 / 255, 1 / 255, 1) leans 0.0055 rad off the geometric one."""
    return np.array([[[128, 128, 255, 255]]], np.uint8)


def bw_texture():
    """Texel values of exactly 0 and 1 (bytes 0 and 255), alpha 1: albedo and roughness of 0 or 1 reach the shading."""
    y, x = np.mgrid[0:4, 0:4]
    img = np.zeros((4, 4, 4), np.uint8)
    img[..., 0] = np.where((x + y) % 2 == 0, 255, 0); img[..., 1] = np.where(x % 2 == 0, 0, 255); img[..., 2] = np.where(y < 2, 255, 0)
    img[..., 3] = 255
    return img


# ---- the float32 frame of k_eval_scatter (and of the reference's HitResult::BuildOrthonormalBasis) ------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], -(a[..., 0] * b[..., 2] - a[..., 2] * b[..., 0]),
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _normalize(a):
    k = F(1.0) / np.sqrt(_dot(a, a))
    return a * k[..., None]


def frame(n):
    """T, B of `n` ((N, 3) float32) with the operations of rl_render.hip k_eval_scatter in their order: T0 = y if |n.x| > 0.9 else x, B = normalize(T0 x n),
    T = normalize(n x B)."""
    n = np.asarray(n, F)
    t0 = np.where((np.abs(n[:, 0]) > F(0.9))[:, None], np.array([0, 1, 0], F), np.array([1, 0, 0], F)).astype(F)
    B = _normalize(_cross(t0, n))
    T = _normalize(_cross(n, B))
    return T, B


def world_to_local(d, n):
    T, B = frame(n)
    v = -np.asarray(d, F)
    return np.stack([_dot(v, T), _dot(v, B), _dot(v, n)], -1)


# ---- RNG streams: a seed whose stream (seed, i, 0) draws U2 == 0.5 --------------------------------------------------------------------
M64 = (1 << 64) - 1
PCG_A, PCG_C = 6364136223846793005, 1442695040888963407


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _unxorshift(z, s):
    r = z
    for _ in range(64 // s + 1):
        r = z ^ (r >> s)
    return r


def _unmix64(z):
    z = _unxorshift(z, 31)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & M64
    z = _unxorshift(z, 27)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & M64
    z = _unxorshift(z, 30)
    return (z - 0x9E3779B97F4A7C15) & M64


def _pcg_out(old):
    xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
    rot = old >> 59
    return ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF


def stream_draws(seed, i, k):
    """The first k floats of stream (seed, i, 0) (include/raylib_amd_rng.h), in Python integers."""
    s = _mix64(_mix64(seed) ^ ((i << 32) | 0))
    out = []
    for _ in range(k):
        out.append((_pcg_out(s) >> 8) * 2.0 ** -24)
        s = (s * PCG_A + PCG_C) & M64
    return out


def seed_for_half(i, salt=0):
    """A seed whose stream (seed, i, 0) draws U2 = 0.5 exactly as its SECOND float (a microfacet event's u1, BeckmannSample's U2):
    pick the PCG state that outputs 0x80000000 (rot and the xorshifted word chosen, bits 27..63 solved from the top), step it back
    once, and invert the two splitmix64 finalisers of raylib_rng_begin."""
    rot = (salt * 7 + 3) & 31
    xs = ((0x80000000 << rot) | (0x80000000 >> ((32 - rot) & 31))) & 0xFFFFFFFF      # rotl: (xs >> rot) | (xs << (32 - rot)) == 0x80000000
    old = rot << 59
    for k in range(58, 26, -1):                    # bit k of ((old >> 18) ^ old) must be bit k - 27 of xs
        hi = (old >> (k + 18)) & 1 if k + 18 < 64 else 0
        old |= (((xs >> (k - 27)) & 1) ^ hi) << k
    old |= (0x2545F491 * (salt + 1)) & ((1 << 27) - 1)
    s0 = ((old - PCG_C) * pow(PCG_A, -1, 1 << 64)) & M64
    return _unmix64(_unmix64(s0) ^ (i << 32))


# ---- records ------------------------------------------------------------------------------------------------------------------------
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)


def _normals(rng, k):
    n = rng.normal(size=(k, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return np.concatenate([AXES, n.astype(F)]).astype(F)


def _perp(n):
    """A direction with float32 d . n == 0 exactly, in the dot's own operation order: (n.y, -n.x, 0), or (0, n.z, -n.y) on the z axis."""
    use_z = (n[:, 0] == 0) & (n[:, 1] == 0)
    a = np.stack([n[:, 1], -n[:, 0], np.zeros(len(n), F)], 1)
    b = np.stack([np.zeros(len(n), F), n[:, 2], -n[:, 1]], 1)
    return np.where(use_z[:, None], b, a).astype(F)


def families(seed=3):
    """name -> (N, 3) directions and (N, 3) normals."""
    rng = np.random.RandomState(seed)
    n = _normals(rng, 26)
    out = {}
    out["normal"] = (-n, n)
    p = _perp(n)
    out["grazing"] = (np.concatenate([p, -p]), np.concatenate([n, n]))
    ax = AXES
    pa = _perp(ax)
    g = []
    for eps in (2.0 ** -20, 2.0 ** -126, 2.0 ** -140):
        g.append((pa - F(eps) * ax).astype(F))                                      # axis normals: Wo.z = eps exactly
    nr = n[6:]
    g.append(np.stack([nr[:, 1], -nr[:, 0], -(F(2.0 ** -20) / nr[:, 2])], 1).astype(F))   # random normals: Wo.z ~ 2^-20
    out["grazing_eps"] = (np.concatenate(g), np.concatenate([ax, ax, ax, nr]))
    back = (n + F(0.3) * rng.normal(size=n.shape).astype(F)).astype(F)
    back[_dot(back, n) <= 0] = n[_dot(back, n) <= 0]
    out["back"] = (back, n)
    # exact zero local x (then y): -d = (T.y, -T.x, 0) is orthogonal to T in float32, whatever T is
    T, B = frame(n)
    zl = []
    for V in (T, B):
        w = _perp(V)
        mixn = (w + F(0)).astype(F)
        zl += [-mixn, mixn]
    out["zero_local"] = (np.concatenate(zl), np.concatenate([n] * 4))
    # axis normals, local x or y exactly +-0 or tiny, the other two components of either sign
    tl, tn = [], []
    for k, nn in enumerate(AXES):
        Tk, Bk = frame(nn[None])
        for tiny in (0.0, -0.0, 2.0 ** -140, -(2.0 ** -140), 2.0 ** -110, -(2.0 ** -110)):
            for sb in (0.6, -0.6):
                for sn in (0.8, -0.8):
                    for first in (0, 1):
                        a, b = (Tk[0], Bk[0]) if first == 0 else (Bk[0], Tk[0])
                        v = F(tiny) * a + F(sb) * b + F(sn) * nn
                        tl.append(-v.astype(F)); tn.append(nn)
    out["tiny_local"] = (np.array(tl, F), np.array(tn, F))
    bulk_n = _normals(rng, 400)[6:]
    bulk_d = rng.normal(size=bulk_n.shape).astype(F)
    flip = _dot(bulk_d, bulk_n) > 0
    bulk_d[flip] = -bulk_d[flip]
    out["regular"] = (bulk_d, bulk_n)
    return out


def to_records(d, n, rng):
    rec = np.zeros((len(d), 16), F)
    rec[:, 0:3] = rng.uniform(-1, 1, (len(d), 3))
    rec[:, 3:6] = d
    rec[:, 7] = 1.0
    rec[:, 8:11] = rng.uniform(-1, 1, (len(d), 3))
    rec[:, 11:14] = n
    rec[:, 14:16] = rng.uniform(0, 1, (len(d), 2))
    return np.ascontiguousarray(rec, F)


def layouts(fams, rng):
    """[(name, records)]: each family alone in whole waves of 64; one degenerate record among 63 regular ones at lane 0, 31, 63;
    everything shuffled."""
    regular = to_records(*fams["regular"], rng)
    degen = {k: to_records(d, n, rng) for k, (d, n) in fams.items() if k != "regular"}
    out = []
    for k, r in degen.items():
        reps = -(-len(r) // 64) * 64
        out.append(("alone:" + k, np.ascontiguousarray(np.resize(r, (reps, 16)), F)))
    every = np.concatenate(list(degen.values()))
    waves = []
    for j, rec in enumerate(every):
        w = regular[rng.randint(0, len(regular), 64)].copy()
        w[(0, 31, 63)[j % 3]] = rec
        waves.append(w)
    out.append(("one_in_a_wave", np.ascontiguousarray(np.concatenate(waves), F)))
    allr = np.concatenate([every, regular])
    out.append(("shuffled", np.ascontiguousarray(allr[rng.permutation(len(allr))], F)))
    return out


# ---- CPU part ------------------------------------------------------------------------------------------------------------------------
def test_degenerate_families_have_their_exact_zeros_in_the_device_frame():
    fams = families()
    wo = {k: world_to_local(d, n) for k, (d, n) in fams.items()}
    assert (wo["grazing"][:, 2] == 0).all()                                 # tanThetaI: wiStretched.z == 0
    z = wo["grazing_eps"][:, 2]
    assert ((z > 0) & (z < 2.0 ** -19)).all() and (z <= 2.0 ** -126).sum() == 12 and (z == 2.0 ** -140).sum() == 6
    assert (wo["normal"][:6] == np.array([0, 0, 1], F)).all()               # DivSpecular: axis normals, Wo = (0, 0, 1) exactly
    assert (wo["back"][:, 2] < 0).all()
    zl = wo["zero_local"]
    half = len(zl) // 2
    assert (zl[:half, 0] == 0).all() and (zl[half:, 1] == 0).all()          # CosSinPhi: an exact zero numerator
    assert ((np.abs(zl[:, 2]) > 0) & (np.abs(zl[:, 2]) < 0.999)).sum() > len(zl) // 2   # ... most with sinTheta > 0
    tl = wo["tiny_local"]
    small = np.minimum(np.abs(tl[:, 0]), np.abs(tl[:, 1]))
    assert (small < 2.0 ** -102).all() and (small == 0).sum() == len(tl) // 3 and (np.abs(tl[:, 2]) == F(0.8)).all()
    assert (tl[:, 0] == 0).any() and (tl[:, 1] == 0).any() and (np.abs(tl[:, :2]) == F(2.0 ** -140)).any()
    assert (wo["regular"][:, 2] > 0).all()


def test_seeds_for_a_zero_slope_draw():
    for i in (0, 31, 63, 100):
        for salt in range(3):
            s = seed_for_half(i, salt)
            assert stream_draws(s, i, 2)[1] == 0.5, (i, salt)
    # the restated stream is the shared header's: the oracle's camera rays consume (seed, i, 0)'s first three draws
    orc = helpers.ffi.load_oracle()
    cam = ffi.make_camera((0, 0, 0), (0, 0, -1), 60.0, 1.0, 0.5, 1.0, 0.0, 1.0)
    uv = np.full((4, 2), 0.5, F)
    t = orc.camera_rays(cam, uv, seed=12345)[:, 6]
    assert np.array_equal(t, np.array([stream_draws(12345, i, 3)[2] for i in range(4)], F))


# ---- GPU part ------------------------------------------------------------------------------------------------------------------------
def _edge_scene(lib, oracle, d, with_map=True, objects=None):
    os.makedirs(d, exist_ok=True)
    names = [l.split()[1] for l in (EDGE_MTL + (MAPPED_MTL if with_map else "")).split("\n") if l.startswith("newmtl")]
    if objects is None:
        objects = [("o_" + m, m, [helpers.scenes._quad((i, 0, 0), (i + 1, 0, 0), (i + 1, 1, 0), (i, 1, 0))]) for i, m in enumerate(names)]
    obj, ntri = helpers.scenes.write_obj(os.path.join(d, "edge.obj"), objects, EDGE_MTL + ("\n" + MAPPED_MTL if with_map else ""))
    maps = {"bw.png": bw_texture(), "tilt.png": tilt_texture()}
    if with_map:
        for k, img in maps.items():
            helpers.scenes.write_png_rgba(os.path.join(d, k), img)
    loader = lambda p: helpers.scenes.texture_as_float(maps[os.path.basename(p)]) if os.path.basename(p) in maps else None
    flat = helpers.objflat.load_obj(obj, oracle, texture_loader=loader)
    return obj, flat, names, ntri


@pytest.fixture(scope="module")
def edge_scene(gpu_lib, oracle, workdir):
    from raylib_amd import binding
    obj, flat, names, _ = _edge_scene(gpu_lib, oracle, os.path.join(str(workdir), "scatter_edges"))
    ses = binding.SceneSession(gpu_lib, obj, (0, 0.5, 4), (0, 0.5, 0), 45.0, 1.0)
    tris, mats = ses.export_flat()
    assert mats.tobytes() == flat.materials.tobytes(), "the product's MTL reading and the checker's disagree"
    yield ses, oracle.scene_create(flat), names, mats
    ses.close()


def _eval(lib, ses, mi, rec, seed):
    out = np.zeros((len(rec), 16), F)
    assert lib.RaylibAMD_EvalScatter(ses.scene, mi, rec.ctypes.data_as(C.POINTER(C.c_float)), len(rec), seed,
                                     out.ctypes.data_as(C.POINTER(C.c_float))) == 1
    return out


def _compare(out, want, what, rec):
    same = helpers.same(out, want)
    bad = ~same.all(1)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError("%s: %d of %d records differ (fields %s); first at %d: d=%r n=%r device=%r oracle=%r" % (
            what, int(bad.sum()), len(out), sorted(set(np.nonzero(~same)[1].tolist())), i, rec[i, 3:6].tolist(), rec[i, 11:14].tolist(),
            out[i].tolist(), want[i].tolist()))


@pytest.mark.gpu
def test_scatter_at_degenerate_inputs_matches_the_oracle_in_every_layout(gpu_lib, edge_scene, oracle):
    ses, scene, names, mats = edge_scene
    m = {k: mats[i] for i, k in enumerate(names)}
    assert m["zero_kd_metal"]["metallic"] == 1 and m["zero_kd_metal"]["albedo"][1] == 0 and m["zero_kd_metal"]["roughness"] < 1e-14
    assert m["ns_huge"]["roughness"] < 1e-14 and m["pr_tiny"]["roughness"] == F(1e-6) and m["mapped"]["texRoughness"] >= 0
    assert 0 < m["tiny_kd_metal"]["albedo"][0] < 1.2e-38
    fams = families()
    rng = np.random.RandomState(9)
    sets = layouts(fams, rng)
    for mi in range(len(mats)):
        for name, rec in sets:
            out = _eval(gpu_lib, ses, mi, rec, 1)
            _compare(out, oracle.scatter(scene, mi, rec, seed=1), "material %s, layout %s" % ((names + ["fallback"])[mi], name), rec)
    # TINY-NDF: normal incidence on axis normals, 4096 streams
    mi = names.index("tiny_ndf")
    rec = to_records(np.resize(-AXES, (4096, 3)), np.resize(AXES, (4096, 3)), rng)
    out = _eval(gpu_lib, ses, mi, rec, 1)
    want = oracle.scatter(scene, mi, rec, seed=1)
    spec = want[:, 1]
    assert ((spec > 0) & (spec < 2.0 ** -100)).sum() > 100 and (spec > 2.0 ** -80).sum() > 100, "the set no longer straddles the guard"
    _compare(out, want, "material tiny_ndf, normal incidence", rec)


@pytest.mark.gpu
def test_zero_local_component_with_a_zero_slope_matches_the_oracle(gpu_lib, edge_scene, oracle):
    """CosSinPhi's zero and tiny numerators where the sampled slope is 0 (U2 == 0.5): the quotient's sign and last bit reach the
    scattered direction.  One degenerate record per wave of 63 regular ones, at lane 0, 31 or 63, with a seed made for that lane."""
    ses, scene, names, mats = edge_scene
    fams = families()
    rng = np.random.RandomState(17)
    regular = to_records(*fams["regular"], rng)
    degen = np.concatenate([to_records(*fams["zero_local"], rng), to_records(*fams["tiny_local"], rng)])
    for k in ROUGH:
        mi = names.index(k)
        for j, rec in enumerate(degen):
            lane = (0, 31, 63)[j % 3]
            w = regular[rng.randint(0, len(regular), 64)].copy()
            w[lane] = rec
            seed = seed_for_half(lane, j)
            _compare(_eval(gpu_lib, ses, mi, w, seed), oracle.scatter(scene, mi, w, seed=seed), "material %s, record %d at lane %d" % (k, j, lane), w)


# ---- whole frames (D) ----------------------------------------------------------------------------------------------------------------
def _room_objects():
    """The Cornell room (36 triangles) on the edge materials: axis-aligned walls, both boxes, the light."""
    mats = {"floor": "zero_kd_metal", "ceiling": "pr_one", "backwall": "tiny_kd_metal", "leftwall": "metal1", "rightwall": "ns_huge",
            "light": "light", "shortbox": "glass24", "tallbox": "mirror"}
    objs = helpers.scenes.cornell_objects()
    out = [(name, mats[name], quads) for name, _, quads in objs]
    # the pieces not on a wall: a glass slab of Ni 1, a tiny-roughness and an emissive panel, a metal0 card (the room stays <= 108 triangles)
    q = helpers.scenes._quad
    out.append(("slab", "glass10", [q((-0.9, 0.8, 0.6), (-0.5, 0.8, 0.6), (-0.5, 1.2, 0.6), (-0.9, 1.2, 0.6))]))
    out.append(("tiny", "pr_tiny", [q((0.5, 1.0, -0.99), (0.9, 1.0, -0.99), (0.9, 1.6, -0.99), (0.5, 1.6, -0.99))]))
    out.append(("panel", "emissive", [q((-0.2, 1.5, -0.995), (0.2, 1.5, -0.995), (0.2, 1.8, -0.995), (-0.2, 1.8, -0.995))]))
    out.append(("card", "metal0", [q((0.99, 0.2, -0.6), (0.99, 0.2, -0.2), (0.99, 0.7, -0.2), (0.99, 0.7, -0.6))]))
    return out


@pytest.mark.gpu
def test_frames_of_the_edge_materials_match_the_oracle_on_every_schedule(gpu_lib, oracle, workdir, monkeypatch):
    from raylib_amd import binding
    obj, flat, names, ntri = _edge_scene(gpu_lib, oracle, os.path.join(str(workdir), "scatter_room"), with_map=False, objects=_room_objects())
    assert ntri <= 108
    w, h = 65, 49
    origin, look = (0.0, 1.0, 3.9), (0.0, 1.0, -1.0)
    ses = binding.SceneSession(gpu_lib, obj, origin, look, 45.0, w / h)
    try:
        tris, mats = ses.export_flat()
        assert tris.tobytes() == flat.triangles.tobytes() and mats.tobytes() == flat.materials.tobytes()
        scene = oracle.scene_create(flat)
        cam = ffi.make_camera(origin, look, 45.0, w / h)
        ties = helpers.tie_mask(oracle, flat, cam, w, h)
        assert ties.mean() < 0.01, ties.sum()                  # a few pixels of the boxes' edges
        for spp in (1, 16):
            want = oracle.render(scene, cam, ffi.make_settings(w, h, spp), seed=1)
            for env, plain in (({"RAYLIB_POOL": "0"}, 1), ({"RAYLIB_POOL": "0", "RAYLIB_PLAIN_KERNEL": "0"}, 0),
                               ({"RAYLIB_POOL": "2"}, None), ({"RAYLIB_POOL": "4"}, None)):
                monkeypatch.delenv("RAYLIB_PLAIN_KERNEL", raising=False)
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                img = ses.render(w, h, spp)
                st = ses.stats()
                p = helpers.assert_planned(gpu_lib, ses, st, w, h, spp)
                if plain is not None:                       # k_trace, the leaf-list kernel: plain or general instance
                    assert gpu_lib.RaylibAMD_LastTracePlain() == plain and st.treeWidth == 0, (env, p)
                helpers.assert_same_outside_ties(img, want, ties, "spp %d %r" % (spp, env))
        monkeypatch.delenv("RAYLIB_PLAIN_KERNEL", raising=False)
        monkeypatch.delenv("RAYLIB_POOL", raising=False)
    finally:
        ses.close()
