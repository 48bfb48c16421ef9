"""Device math at its edges (RaylibAMD_EvalDeviceMath, csrc/rl_math.h / rl_glibc_math.h) against the host libm, one call per element.

tests/test_math_exact.py samples the functions on their typical ranges.  This file feeds every hook the inputs where a device build
goes wrong and a typical input never looks: subnormal arguments and results (an instruction that flushes them: v_rcp_f32, v_exp_f32,
v_log_f32, v_rsq_f32), signed zeros, infinities, NaN, the thresholds of each function (expf's overflow / underflow, sinf's large-argument
reduction, acosf at +-1, the integer tests of powf, fmodf past 2^23) and the range guards of the short exact sequences (rcp1_, sqrt_).

Expected values come from the host's libm (glibc 2.35, which rl_glibc_math.h restates), computed by a small C program compiled at test
time: the same calls ctypes makes, a million at a time.  The CPU part checks the input generator and that program; the GPU part runs
the device hooks and wants the host's bits, NaN meeting NaN (helpers.same)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers

# hook -> libm name of the host function it must equal (include/raylib_amd.h, RaylibAMD_EvalDeviceMath)
ONE_ARG = {0: "sinf", 1: "cosf", 2: "tanf", 3: "acosf", 4: "asinf", 6: "expf", 7: "logf", 9: "sinf", 10: "cosf", 11: "sqrtf",
           13: "fmodf1", 14: "rcp", 15: "sqrtf"}
TWO_ARG = {5: "atan2f", 8: "powf"}
STRIDE = 4093                    # prime: about 2^32 / 4093 = 1.05 M bit patterns per function, every binade of both signs

HOST_LIBM_C = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
/* out[i] = f(x[i] [, y[i]]) by the host libm, one call per element.  argv: fn in out.  The calls go through volatile pointers so that
 * the compiler can neither fold nor vectorise them. */
static float rcp(float x) { volatile float one = 1.0f; return one / x; }
static float fmod1(float x) { return fmodf(x, 1.0f); }
int main(int argc, char** argv)
{
	if (argc != 4) return 2;
	const int fn = atoi(argv[1]);
	FILE* f = fopen(argv[2], "rb");
	if (!f) return 3;
	int64_t n = 0;
	if (fread(&n, 8, 1, f) != 1) return 4;
	float* x = (float*)malloc(n * 4 + 4); float* y = (float*)malloc(n * 4 + 4); float* o = (float*)malloc(n * 4 + 4);
	if (fread(x, 4, n, f) != (size_t)n) return 5;
	const int two = fn == 5 || fn == 8;
	if (two && fread(y, 4, n, f) != (size_t)n) return 6;
	fclose(f);
	float (*volatile g1)(float) = 0;
	float (*volatile g2)(float, float) = 0;
	switch (fn) {
		case 0: case 9: g1 = sinf; break;
		case 1: case 10: g1 = cosf; break;
		case 2: g1 = tanf; break;
		case 3: g1 = acosf; break;
		case 4: g1 = asinf; break;
		case 5: g2 = atan2f; break;
		case 6: g1 = expf; break;
		case 7: g1 = logf; break;
		case 8: g2 = powf; break;
		case 11: case 15: g1 = sqrtf; break;
		case 13: g1 = fmod1; break;
		case 14: g1 = rcp; break;
		default: return 7;
	}
	for (int64_t i = 0; i < n; ++i) o[i] = two ? g2(x[i], y[i]) : g1(x[i]);
	f = fopen(argv[3], "wb");
	if (!f || fwrite(o, 4, n, f) != (size_t)n) return 8;
	fclose(f);
	return 0;
}
"""


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def f32(bits_):
    return np.asarray(bits_, np.uint64).astype(np.uint32).view(np.float32)


def around(values, k):
    """Every float within k ulps of each value (both directions, across zero by bit pattern of the same sign only)."""
    b = helpers.bits(np.asarray(values, np.float32)).astype(np.int64)
    d = np.arange(-k, k + 1, dtype=np.int64)
    out = (b[:, None] + d[None, :]).ravel()
    sign = b[:, None].repeat(len(d), 1).ravel() & 0x80000000
    keep = ((out & 0x80000000) == sign) & (out >= 0) & (out <= 0xFFFFFFFF)
    return f32(out[keep])


FLT_MIN, FLT_MAX, DENORM_MIN = np.float32(1.17549435e-38), np.float32(3.4028235e38), f32([1])[0]
QNAN, SNAN = f32([0x7FC00000, 0xFFC00000]), f32([0x7FA00000, 0xFFA00000])


def special_values():
    """The classes every one-argument hook gets: signed zeros, FLT_MIN, FLT_MAX, infinities, quiet and signalling NaN, 1 +- 1 ulp."""
    v = np.array([0.0, -0.0, np.inf, -np.inf], np.float32)
    return np.concatenate([v, around([FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, 1.0, -1.0, DENORM_MIN, -DENORM_MIN], 1), QNAN, SNAN])


def subnormal_band():
    """The lowest 2^16 subnormal patterns and the 2^16 just below FLT_MIN, both signs."""
    lo = np.arange(1, 1 << 16, dtype=np.uint64)
    hi = np.arange(0x00800000 - (1 << 16), 0x00800000, dtype=np.uint64)
    b = np.concatenate([lo, hi])
    return f32(np.concatenate([b, b | 0x80000000]))


def thresholds(fn):
    """Each function's own edges."""
    if fn == 6:                                   # expf: overflow, the last normal result, the last subnormal one, the round-to-0 edge
        return around([88.72283935546875, 88.7228317, -87.3365478515625, -103.27893066, -103.97207642, -103.9720840, -150.0, 1e-7, -1e-7], 64)
    if fn in (0, 1, 2, 9, 10):                    # the reduction: 2^28, the large-argument path, multiples of pi / 2 near and far
        k = np.concatenate([np.arange(1, 65), 2.0 ** np.arange(7, 120, 3), np.array([1e5, 355.0 / 2, 102943.0, 1e9])])
        mult = np.float32(k * np.pi / 2)
        return np.concatenate([around([2.0 ** 28, -(2.0 ** 28), 2.0 ** 27, 2.0 ** 29, 120.0, 2.0 ** 63, 1e38], 8), around(mult, 3),
                               -around(mult, 3), around([np.pi, np.pi / 4, 3 * np.pi / 4], 16)])
    if fn in (3, 4):                              # acosf / asinf at +-1 and the polynomial switch points
        return around([1.0, -1.0, 0.5, -0.5, 0.9999999, 2.0 ** -12, -(2.0 ** -12), 2.0 ** -26, 0.975, -0.975], 16)
    if fn == 7:                                   # logf around 1, FLT_MIN, the largest subnormal
        return around([1.0, 2.0, 0.5, FLT_MIN, FLT_MAX, 0.9999, 1.0001], 64)
    if fn == 13:                                  # fmodf(x, 1): 2^23 +- ulps, integers and half-integers up to 2^24 and past it
        ints = np.concatenate([np.arange(0, 4097, dtype=np.float64), 2.0 ** 23 + np.arange(-1024, 1025), 2.0 ** 24 + 2 * np.arange(-512, 513),
                               2.0 ** np.arange(24, 128)])
        half = np.arange(0, 4096) + 0.5
        v = np.concatenate([ints, half, 2.0 ** 23 - 0.5 - np.arange(64), 2.0 ** 22 + 0.25 + np.arange(64)]).astype(np.float32)
        return np.concatenate([v, -v, around([2.0 ** 23, 2.0 ** 24, 1.0, 0.5], 32), -around([2.0 ** 23, 2.0 ** 24, 1.0, 0.5], 32)])
    if fn in (11, 14, 15):                        # rcp1_ / sqrt_'s range guards: 2^-126, 2^126, 2^-101
        e = [2.0 ** -126, 2.0 ** 126, 2.0 ** -101, 2.0 ** -102, 2.0 ** 127, 2.0 ** -127, 2.0 ** -149 * 3]
        return np.concatenate([around(e, 16), -around(e, 16)])
    return np.zeros(0, np.float32)


def one_arg_inputs(fn):
    sweep = f32(np.arange(0, 1 << 32, STRIDE, dtype=np.uint64))
    return np.ascontiguousarray(np.concatenate([sweep, subnormal_band(), special_values(), thresholds(fn)]), np.float32)


def pair_specials():
    """About 100 floats of the two-argument cross product: what powf_checkint / atan2f's quadrant code decide on."""
    pos = np.array([0.0, DENORM_MIN, f32([0x007FFFFF])[0], FLT_MIN, 1.0, 0.5, 2.0, 3.0, 4.0, 5.0, 0.25, 1.5, 2.5, 10.0, 1e-10, 1e10,
                    1.0 / 3, 100.0, 126.0, 127.0, 128.0, 149.0, 150.0, 2.0 ** 23 + 1, 2.0 ** 23 + 2, 2.0 ** 24, FLT_MAX, np.inf,
                    1e-30, 65535.0, 0.999, 7.0, 2.0 ** 31, 1e30, 6.0, 9.0, 0.75, 1e-5, 1e5, 16.0, 33.0,
                    2.0 ** 25 - 2, 2.0 ** -75, 1e38], np.float32)
    near = around([1.0, 2.0 ** 24, 2.0 ** 23], 1)
    v = np.unique(np.concatenate([pos, near]))
    return np.concatenate([v, -v, QNAN[:1], SNAN[:1]]).astype(np.float32)


def pow_inputs(rng):
    s = pair_specials()
    x1, y1 = np.repeat(s, len(s)), np.tile(s, len(s))
    # x in [1 - 2^-10, 1 + 2^-10], every float of it, with |y| up to 2^20
    xb = f32(np.arange(int(helpers.bits(np.float32(1 - 2.0 ** -10))), int(helpers.bits(np.float32(1 + 2.0 ** -10))) + 1, dtype=np.uint64))
    yb = (rng.choice([-1.0, 1.0], len(xb)) * 2.0 ** rng.uniform(-4, 20, len(xb))).astype(np.float32)
    # x^y near 2^128 and near 2^-149 (the overflow and the round-to-zero thresholds), from both sides
    xo = (2.0 ** rng.uniform(0.05, 40, 40000)).astype(np.float32)
    tgt = rng.choice([128.0, -126.0, -149.0, -150.0], len(xo)) + rng.uniform(-0.02, 0.02, len(xo))
    yo = (tgt / np.log2(xo.astype(np.float64))).astype(np.float32)
    flip = rng.rand(len(xo)) < 0.5
    xo[flip] = 1 / xo[flip]; yo[flip] = -yo[flip]
    # negative x: integer y (odd and even, the sign of the result) and non-integer y (NaN)
    xn = -(2.0 ** rng.uniform(-20, 20, 40000)).astype(np.float32)
    yn = np.where(rng.rand(len(xn)) < 0.7, rng.randint(-300, 300, len(xn)), rng.uniform(-30, 30, len(xn))).astype(np.float32)
    x = np.concatenate([x1, xb, xo, xn]).astype(np.float32)
    y = np.concatenate([y1, yb, yo, yn]).astype(np.float32)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def atan2_inputs(rng):
    s = pair_specials()
    x1, y1 = np.repeat(s, len(s)), np.tile(s, len(s))
    # |a / b| near 2^100 and 2^-100, every quadrant
    b = (2.0 ** rng.uniform(-20, 20, 40000)).astype(np.float32)
    a = (b.astype(np.float64) * 2.0 ** (rng.choice([-100.0, 100.0, -126.0, 24.0, -24.0], len(b)) + rng.uniform(-1, 1, len(b)))).astype(np.float32)
    sa, sb = rng.choice([-1, 1], len(b)), rng.choice([-1, 1], len(b))
    a, b = (a * sa).astype(np.float32), (b * sb).astype(np.float32)
    # unit-vector pairs like the sky lookup's (atan2 of two components of a normalised direction), axes included
    d = rng.normal(size=(60000, 3)).astype(np.float32)
    d /= np.sqrt((d * d).sum(1, dtype=np.float32))[:, None]
    axes = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [0.0, -0.0], [-0.0, 1], [-0.0, -1]], np.float32)
    x = np.concatenate([x1, a, d[:, 2], axes[:, 0]]).astype(np.float32)
    y = np.concatenate([y1, b, d[:, 0], axes[:, 1]]).astype(np.float32)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def all_inputs():
    rng = np.random.RandomState(11)
    out = {fn: (one_arg_inputs(fn), None) for fn in ONE_ARG}
    out[8] = pow_inputs(rng)
    out[5] = atan2_inputs(rng)
    return out


# ---- the host reference ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_libm(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_libm")
    src, exe = str(d / "host_libm.c"), str(d / "host_libm")
    with open(src, "w") as f:
        f.write(HOST_LIBM_C)
    subprocess.check_call(["gcc", "-O1", "-fno-builtin", "-ffp-contract=off", src, "-o", exe, "-lm"])

    def run(fn, x, y=None):
        x = np.ascontiguousarray(x, np.float32)
        inp, outp = str(d / "in.bin"), str(d / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.int64(len(x)).tobytes() + x.tobytes() + (np.ascontiguousarray(y, np.float32).tobytes() if y is not None else b""))
        subprocess.check_call([exe, str(fn), inp, outp], timeout=300)
        return np.fromfile(outp, np.float32)
    return run


def _ctypes_host(fn, x, y=None):
    m = C.CDLL("libm.so.6")
    name = (ONE_ARG if y is None else TWO_ARG)[fn]
    if name == "rcp":
        return np.array([np.float32(1.0) / np.float32(v) for v in x], np.float32)
    f = getattr(m, "fmodf" if name == "fmodf1" else name)
    f.restype = C.c_float
    f.argtypes = [C.c_float] * (1 if y is None and name != "fmodf1" else 2)
    if name == "fmodf1":
        return np.array([f(float(v), 1.0) for v in x], np.float32)
    if y is None:
        return np.array([f(float(v)) for v in x], np.float32)
    return np.array([f(float(a), float(b)) for a, b in zip(x, y)], np.float32)


# ---- CPU part ----------------------------------------------------------------------------------------------------------------------
def test_edge_inputs_cover_every_class_they_claim():
    inputs = all_inputs()
    for fn, (x, y) in inputs.items():
        b = helpers.bits(x)
        exp, sign = (b >> 23) & 0xFF, b >> 31
        mant = b & 0x7FFFFF
        if y is None:
            # every binade, every sign, from the strided sweep
            for s in (0, 1):
                assert set(np.unique(exp[sign == s]).tolist()) == set(range(256)), (fn, s)
            sub = (exp == 0) & (mant != 0)
            assert (sub & (sign == 0)).sum() >= 1 << 17 and (sub & (sign == 1)).sum() >= 1 << 17, fn
            for v in (0x00000000, 0x80000000, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
                      0x7FC00000, 0x7FA00000, 0xFFA00000, 0x3F800000, 0x3F800001, 0x3F7FFFFF, 0x00000001, 0x807FFFFF, 0x007FFFFF):
                assert (b == v).any(), (fn, hex(v))
            assert len(x) >= 1000000, fn
        else:
            by = helpers.bits(y)
            pairs = set(zip(b.tolist(), by.tolist()))
            sp = helpers.bits(pair_specials()).tolist()
            assert len(sp) >= 90
            assert all((a, c) in pairs for a in sp for c in sp), fn        # the whole cross product
            assert np.isnan(x).any() and np.isnan(y).any() and np.isinf(x).any() and np.isinf(y).any()
    t = {fn: helpers.bits(thresholds(fn)) for fn in (6, 0, 3, 13, 14)}
    assert (t[6] == helpers.bits(np.float32(88.72283935546875))).any() and (t[6] == helpers.bits(np.float32(88.72283935546875)) + 1).any()
    assert (t[0] == helpers.bits(np.float32(2.0 ** 28))).any() and (t[3] == helpers.bits(np.float32(1.0)) + 1).any()
    f13 = thresholds(13)
    assert (f13 == 2.0 ** 24).any() and (f13 == 2.0 ** 24 + 2).any() and (f13 == -(2.0 ** 23 - 0.5)).any() and (f13 == 2.0 ** 100).any()
    assert (t[14] == 0x00800000).any() and (t[14] == 0x00800000 - 1).any() and (t[14] == 0x7E800000).any()
    # powf's hardest band and its thresholds
    x, y = inputs[8]
    band = (x >= np.float32(1 - 2.0 ** -10)) & (x <= np.float32(1 + 2.0 ** -10))
    assert band.sum() >= (1 << 14) + (1 << 13) and np.nanmax(np.abs(y[band])) > 2.0 ** 19
    with np.errstate(all="ignore"):
        lg = y.astype(np.float64) * np.log2(np.abs(x.astype(np.float64)))
    assert (np.abs(lg - 128) < 0.02).sum() > 1000 and (np.abs(lg + 149) < 0.02).sum() > 1000
    neg = x < 0
    assert ((y[neg] == np.round(y[neg])) & (y[neg] % 2 == 1)).sum() > 1000 and (y[neg] != np.round(y[neg])).sum() > 1000
    x, y = inputs[5]
    with np.errstate(all="ignore"):
        r = np.log2(np.abs(x.astype(np.float64) / y))
    assert (np.abs(r - 100) < 1).sum() > 1000 and (np.abs(r + 100) < 1).sum() > 1000
    for sx in (1, -1):
        for sy in (1, -1):
            assert ((np.sign(x) == sx) & (np.sign(y) == sy) & (np.abs(r - 100) < 1)).any()


def test_host_helper_agrees_with_ctypes(host_libm):
    for fn, (x, y) in all_inputs().items():
        pick = np.concatenate([np.arange(0, len(x), max(1, len(x) // 1500)), len(x) - 1 - np.arange(300)])
        xs = x[pick]; ys = y[pick] if y is not None else None
        got = host_libm(fn, xs, ys)
        want = _ctypes_host(fn, xs, ys)
        same = helpers.same(got, want)
        assert same.all(), "fn %d: helper and ctypes differ at x=%r" % (fn, xs[~same][:3])


# ---- GPU part ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_math_at_the_edges_is_bit_identical_to_host_libm(gpu_lib, host_libm):
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    bad = []
    for fn, (x, y) in sorted(all_inputs().items()):
        out = np.zeros_like(x)
        assert gpu_lib.RaylibAMD_EvalDeviceMath(fn, fp(x), fp(y) if y is not None else None, len(x), fp(out)) == 1
        want = host_libm(fn, x, y)
        same = helpers.same(out, want)
        if not same.all():
            i = np.nonzero(~same)[0][:4]
            bad.append("fn %d (%s): %d of %d differ, e.g. x=%s%s device=%s host=%s" % (
                fn, (ONE_ARG if y is None else TWO_ARG)[fn], (~same).sum(), len(x), [hex(v) for v in helpers.bits(x[i])],
                "" if y is None else " y=%s" % [hex(v) for v in helpers.bits(y[i])],
                [hex(v) for v in helpers.bits(out[i])], [hex(v) for v in helpers.bits(want[i])]))
    assert not bad, "\n".join(bad)
