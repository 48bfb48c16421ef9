"""Host restatement of the short divisions of the scattering event (csrc/rl_math.h div_by_, csrc/rl_dev_shade.h RL_EXACT_DIV bits 1 and 2):
q0 = a * y, q = fma(fma(-b, q0, a), y, q0) with y = RN(1 / b), evaluated here with exact rational arithmetic and one rounding per operation,
and the sign predicate that replaces `dot(V, H) / dot(V, N) <= 0`.  Wherever a site's guard lets the short form through, it must be the
IEEE quotient bit for bit; the edge cases are zeros of both signs, denormals, 2^-102 / 2^-103 numerators, divisors at 2^-126 and 2^126,
infinities and NaN."""
from fractions import Fraction
import itertools
import math

import numpy as np

f32 = np.float32


def rn32(x):
    """Fraction -> the nearest float32 (ties to even), with gradual underflow and overflow to infinity."""
    if x == 0:
        return f32(0.0)
    s = -1 if x < 0 else 1
    m = abs(x)
    e = math.floor(math.log2(m.numerator) - math.log2(m.denominator))
    while Fraction(2) ** e > m:
        e -= 1
    while Fraction(2) ** (e + 1) <= m:
        e += 1
    e = max(e, -126)                           # denormals: a fixed quantum of 2^-149
    quantum = Fraction(2) ** (e - 23)
    k = m / quantum
    n = math.floor(k)
    r = k - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    v = n * quantum
    if v >= Fraction(2) ** 128:
        return f32(s * np.inf)
    return f32(s * float(v))


def fmaf(a, b, c):
    a, b, c = f32(a), f32(b), f32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return f32(np.float64(a) * np.float64(b) + np.float64(c))   # inf / NaN: exact enough, no rounding involved
    r = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if r == 0:                                  # the sign of an exact zero sum under round-to-nearest
        p_neg = (np.signbit(a) != np.signbit(b)) if (a == 0 or b == 0) else (a * b < 0)
        return f32(-0.0) if (p_neg and np.signbit(c)) else f32(0.0)
    return rn32(r)


def div_by(a, b, y):
    with np.errstate(all="ignore"):
        q0 = f32(a) * f32(y)
    return fmaf(fmaf(-f32(b), q0, a), y, q0)


def ieee(a, b):
    with np.errstate(all="ignore"):
        return f32(a) / f32(b)


def same(x, y):
    return (np.isnan(x) and np.isnan(y)) or f32(x).view(np.uint32) == f32(y).view(np.uint32)


def rcp(b):
    with np.errstate(all="ignore"):
        return f32(1.0) / f32(b)


def in_range(q):   # csrc/rl_dev_shade.h QuotientInRange
    return abs(q) >= 2.0 ** -91 and abs(q) < 2.0 ** 126


TINY = [0.0, -0.0, 1e-45, -1e-45, 2.0 ** -140, 2.0 ** -126, 2.0 ** -110, 2.0 ** -103, -(2.0 ** -103), float(f32(2.0 ** -102) - f32(2.0 ** -126)),
        2.0 ** -102, -(2.0 ** -102), 2.0 ** -101 * 1.5, 2.0 ** -91, 2.0 ** -90]
ORDINARY = [1e-30, 1e-10, 0.04, 0.3333333, 0.5, 1.0, -1.0, 0.75, 3.0, 1919.0, 1e10, 1e30]
HUGE = [2.0 ** 100, 2.0 ** 115, 2.0 ** 116, 2.0 ** 120, float(np.finfo(np.float32).max), np.inf, -np.inf, np.nan]
NUMERATORS = [f32(v) for v in TINY + ORDINARY + HUGE]


def test_div_by_is_the_quotient_under_its_stated_conditions():
    """2^-126 <= |b| < 2^126, |a| >= 2^-102, 2^-126 <= |a / b| < 2^127: the short form is the division (rl_math.h)."""
    divisors = [f32(v) for v in (2.0 ** -126, -(2.0 ** -126), 2.0 ** -125 * 1.5, 1e-20, 0.001, 0.1, 1.0, 3.0, -7.0, 1920.0, 9.5e10, 2.0 ** 125,
                                 float(np.nextafter(f32(2.0 ** 126), f32(0))))]
    checked = 0
    for a, b in itertools.product(NUMERATORS, divisors):
        q = ieee(a, b)
        if np.isfinite(a) and abs(a) >= 2.0 ** -102 and 2.0 ** -126 <= abs(q) < 2.0 ** 127:
            assert same(div_by(a, b, rcp(b)), q), (a, b)
            checked += 1
    assert checked > 100


def test_zero_numerators_are_outside_the_conditions():
    """-0 / b comes out +0 in the short form: why every guard rejects zero numerators."""
    assert same(div_by(f32(0.0), f32(3.0), rcp(3.0)), f32(0.0))
    assert not same(div_by(f32(-0.0), f32(3.0), rcp(3.0)), ieee(-0.0, 3.0))


def test_specular_guard():
    """DivSpecular: b = 4 |N.Wi| |N.Wo| + 0.001 in [0.001, 4.001] or NaN; the quotient is used only when every |q| is in [2^-91, 2^126)."""
    divisors = [f32(v) for v in (0.001, 0.0010000001, 0.01, 0.5, 1.0, 2.0, 4.0, 4.001)] + [f32(np.nan)]
    let_through = 0
    for a, b in itertools.product(NUMERATORS, divisors):
        q = div_by(a, b, rcp(b))
        if in_range(q):
            assert same(q, ieee(a, b)), (a, b)
            let_through += 1
        else:
            assert not (np.isfinite(a) and abs(a) >= 2.0 ** -88 and abs(a) < 2.0 ** 110 and np.isfinite(b)), (a, b)   # only the edges go to the division
    assert let_through > 100


def test_cos_sin_phi_guard():
    """CosSinPhi: s = sqrt(max(0, 1 - z z)) is 0 or in [2^-12, 1]; numerators |w.x|, |w.y| <= 1 of at least 2^-102 take the short form.
    (w is a normalized vector: its components are at most 1 + 2^-22 in magnitude, or NaN; never infinite.)"""
    zs = [f32(v) for v in (0.0, 0.5, 0.9, 0.99999994, 0.9999999, -0.7, 1.0)]
    ss = [f32(np.sqrt(max(f32(0.0), f32(1.0) - z * z))) for z in zs]
    assert min(s for s in ss if s > 0) >= 2.0 ** -12
    for a, s in itertools.product([v for v in NUMERATORS if np.isnan(v) or abs(v) <= 1.0], ss):
        if s != 0 and abs(a) >= 2.0 ** -102:
            assert same(div_by(a, s, rcp(s)), ieee(a, s)), (a, s)


def test_tan_theta_guard():
    """BeckmannSample11: cosThetaI <= .9999 so sinThetaI is in [0.014, 1]; cosThetaI >= 2^-126 takes the short form."""
    for c in [f32(v) for v in (2.0 ** -126, 1e-30, 1e-7, 0.001, 0.3, 0.9999, float(np.nextafter(f32(0.9999), f32(0))))]:
        s = f32(np.sqrt(max(f32(0.0), f32(1.0) - c * c)))
        assert s >= 0.014
        for a in (s, f32(0.014), f32(1.0)):
            assert same(div_by(a, c, rcp(c)), ieee(a, c)), (a, c)


def not_positive(n, d):   # csrc/rl_dev_shade.h QuotientNotPositive
    n, d = f32(n), f32(d)
    opposite = bool(np.signbit(n)) != bool(np.signbit(d))
    if n == 0:
        return bool(d < 0 or d > 0)
    return bool(not (np.isnan(n) or np.isnan(d)) and opposite)


def test_sign_predicate_is_the_comparison_of_the_quotient():
    """dot(V, H) / dot(V, N) <= 0 without the division, for every |d| <= 1 + 2^-21 (a dot product of unit vectors), zeros and NaN."""
    ns = [f32(v) for v in TINY + ORDINARY + HUGE] + [-f32(v) for v in ORDINARY + HUGE[:5]]
    ds = [f32(v) for v in (0.0, -0.0, 1e-45, -1e-45, 2.0 ** -126, -(2.0 ** -126), 1e-20, -1e-20, 0.5, -0.5, 1.0, -1.0, 1.0000001, -1.0000001,
                           1.0 + 2.0 ** -21, -(1.0 + 2.0 ** -21), np.nan)]
    for n, d in itertools.product(ns, ds):
        assert not_positive(n, d) == bool(ieee(n, d) <= 0), (n, d)
