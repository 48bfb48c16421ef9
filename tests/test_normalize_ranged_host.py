"""What can be checked of the ranged normalisations without a device (csrc/rl_dev_core.h "normalize without the two range guards"): the setting is made in the
lazy instance's unit and nowhere else, and the vote's bit test is the interval it claims."""
import glob
import os
import re

import numpy as np

import helpers

PKG = os.path.join(helpers.ROOT, "software-raytracing_amd")
CSRC = os.path.join(PKG, "csrc")


def _read(path):
    with open(path) as f:
        return f.read()


def test_setting_is_on_in_the_lazy_unit_only():
    assert re.search(r"^#ifndef RL_NORMALIZE_RANGED\n#define RL_NORMALIZE_RANGED 0\n#endif", _read(os.path.join(CSRC, "rl_dev_core.h")), re.M)
    setters = []
    sources = [p for p in glob.glob(os.path.join(CSRC, "*")) if p.endswith((".h", ".inl", ".hip", ".cc"))]
    assert len(sources) > 40
    for path in sorted(sources + [os.path.join(PKG, "Makefile")]):
        text = _read(path)
        if re.search(r"^\s*#\s*define\s+RL_NORMALIZE_RANGED\s+[^0\s]", text, re.M) or "-DRL_NORMALIZE_RANGED" in text:
            setters.append(os.path.basename(path))
    assert setters == ["rl_render_lazy.hip"], setters
    # ... before the unit's includes, and overridable for variant builds
    lazy = _read(os.path.join(CSRC, "rl_render_lazy.hip"))
    assert lazy.index("#ifndef RL_NORMALIZE_RANGED\n#define RL_NORMALIZE_RANGED ") < lazy.index("#include")


def test_vote_domain():
    """(bits - 0x0d000000) < (0x7f800000 - 0x0d000000), unsigned: exactly the floats of [2^-101, FLT_MAX] -- whose roots lie inside the short reciprocal's
    [2^-126, 2^126)."""
    m = re.search(r"NormalizeInRange\(float len2\) \{ return \(__float_as_uint\(len2\) - (0x[0-9a-f]+)u\) < \((0x[0-9a-f]+)u - (0x[0-9a-f]+)u\); \}", _read(os.path.join(CSRC, "rl_dev_core.h")))
    assert m, "NormalizeInRange not found"
    lo, hi, lo2 = (int(g, 16) for g in m.groups())
    assert lo == lo2
    f = lambda b: float(np.array([b], np.uint32).view(np.float32)[0])
    assert f(lo) == 2.0 ** -101 and f(hi) == float("inf") and f(hi - 1) == float(np.finfo(np.float32).max)
    rng = np.random.default_rng(20261021)
    bits = np.concatenate([np.array([0, 1, lo - 1, lo, hi - 1, hi, hi + 1, 0x7fc00000, 0x80000000, lo | 0x80000000, 0xff800000, 0xffffffff], np.uint64),
                           rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64)]).astype(np.uint32)
    x = bits.view(np.float32)
    with np.errstate(invalid="ignore"):
        want = (x >= np.float32(2.0 ** -101)) & (x <= np.finfo(np.float32).max)
    got = (bits - np.uint32(lo)) < np.uint32(hi - lo)
    assert (got == want).all()
    with np.errstate(invalid="ignore"):
        root = np.sqrt(x[want])
    assert (root >= np.float32(2.0 ** -126)).all() and (root < np.float32(2.0 ** 126)).all()
