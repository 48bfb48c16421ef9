"""Texture2D::Sample at its edges (RaylibAMD_EvalTexture: TexFetch, csrc/rl_dev_scene.h) against the oracle, bit for bit.

Every lookup wraps its UVs with the device's fmodf (rtm::fmod1_ -- ocml's, not glibc's), adds 1 to a negative remainder, flips v and
scales by (size - 1).  The known-answer test of the contract tier uses one 16 x 16 texture and UVs in [-3, 3]; here the textures are 1,
3, 7, 16 and 17 texels wide or high, and the UVs are the ones where a wrap goes wrong: signed zeros and subnormals, +-1 and the floats
beside them, integers and half-integers up to and past 2^24 (where every float is an even integer), fractional values in [2^23, 2^24),
huge values up to FLT_MAX, infinities, NaN, and negative values so small that u + 1 rounds to 1.0 (the last texel, still in range).
(x - truncf(x) would give these lookups the same texels: it differs from fmodf(x, 1) only in the sign of a zero remainder, which the
wrap discards.  tests/test_math_edges.py checks hook 13, fmodf(x, 1) itself, bit for bit.)"""
import ctypes as C
import os

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

SIZES = {"t1x1": (1, 1), "t1x7": (1, 7), "t7x1": (7, 1), "t3x5": (3, 5), "t16x16": (16, 16), "t17x9": (17, 9)}   # name -> (H, W)


def _image(h, w, seed):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    img.flat[0] = 0
    img.flat[-1] = 255
    return img


def edge_uvs():
    """(N, 2) float32: every value of the list below as u and as v, each paired with a random bulk value, plus a random bulk."""
    rng = np.random.RandomState(21)
    sub = np.float32([1e-45, 2.8e-45, 1e-40, 1.1754942e-38])
    one = np.float32([1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))])
    ints = np.concatenate([np.arange(0, 9), 2.0 ** np.arange(3, 31), 2.0 ** 24 + np.array([1.0, 2.0, 3.0, 4.0, 6.0]),
                           2.0 ** 23 + np.arange(-3, 4), 2.0 ** np.arange(31, 128, 8)])
    halves = np.concatenate([np.arange(0, 9) + 0.5, 2.0 ** np.arange(3, 23) + 0.5, 2.0 ** 23 - np.array([0.5, 1.5])])
    frac = 2.0 ** 23 + rng.randint(0, 1 << 23, 64) + 0.5                       # [2^23, 2^24): the fraction is exactly 0.5
    huge = np.float32([1e30, 1e38, 3.4028235e38, np.inf])
    tiny_neg = np.float32([2.0 ** -25, 2.0 ** -30, 1e-20, 2.0 ** -24 * 0.75])    # -x + 1 rounds to 1.0
    v = np.concatenate([[0.0], sub, one, ints, halves, frac, huge, tiny_neg, [0.25, 0.75, 1.0 / 3, 0.999]]).astype(np.float32)
    v = np.concatenate([v, -v, np.float32([np.nan, -np.nan])]).astype(np.float32)
    bulk = rng.uniform(-3, 3, len(v)).astype(np.float32)
    uv = np.concatenate([np.stack([v, bulk], 1), np.stack([bulk, v], 1), np.stack([v, v[::-1]], 1),
                         np.stack([rng.uniform(-1e4, 1e4, 4000), rng.uniform(-4, 4, 4000)], 1)]).astype(np.float32)
    return np.ascontiguousarray(uv)


@pytest.fixture(scope="module")
def texture_scene(gpu_lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "texture_edges"); os.makedirs(d, exist_ok=True)
    imgs = {name: _image(h, w, i) for i, (name, (h, w)) in enumerate(SIZES.items())}
    mtl = "".join("newmtl m_%s\nKd 0.5 0.5 0.5\nPr 0.5\nmap_Pr %s.png\n\n" % (name, name) for name in imgs)
    objs = [("q_%s" % name, "m_" + name, [helpers.scenes._quad((i, 0, 0), (i + 1, 0, 0), (i + 1, 1, 0), (i, 1, 0))]) for i, name in enumerate(imgs)]
    obj, _ = helpers.scenes.write_obj(os.path.join(d, "tex.obj"), objs, mtl)
    for name, img in imgs.items():
        helpers.scenes.write_png_rgba(os.path.join(d, name + ".png"), img)
    ses = binding.SceneSession(gpu_lib, obj, (0, 0.5, 4), (0, 0.5, 0), 45.0, 1.0)
    yield ses, imgs
    ses.close()


def _product_textures(lib, ses):
    out = []
    for i in range(lib.RaylibAMD_SceneNumTextures(ses.scene)):
        w, h = C.c_int32(0), C.c_int32(0)
        lib.RaylibAMD_SceneTextureSize(ses.scene, i, C.byref(w), C.byref(h))
        t = np.zeros((h.value, w.value, 4), np.float32)
        lib.RaylibAMD_SceneExportTexture(ses.scene, i, t.ctypes.data_as(C.POINTER(C.c_float)))
        out.append(t)
    return out


def test_texture_lookup_at_edge_uvs_matches_the_oracle(gpu_lib, texture_scene, oracle, ref):
    ses, imgs = texture_scene
    tex = _product_textures(gpu_lib, ses)
    assert len(tex) == len(imgs)
    by_size = {t.shape[:2]: (i, t) for i, t in enumerate(tex)}
    uv = edge_uvs()
    checkers = [oracle] + ([ref] if ref is not None else [])
    for name, img in imgs.items():
        i, t = by_size[img.shape[:2]]
        want_tex = helpers.scenes.texture_as_float(img)
        assert t.tobytes() == want_tex.tobytes(), "%s: the product did not decode the PNG to byte / 255" % name
        for srgb in (0, 1):
            out = np.zeros((len(uv), 4), np.float32)
            assert gpu_lib.RaylibAMD_EvalTexture(ses.scene, i, srgb, uv.ctypes.data_as(C.POINTER(C.c_float)), len(uv),
                                                 out.ctypes.data_as(C.POINTER(C.c_float))) == 1
            for chk in checkers:
                want = chk.texture_sample(want_tex, srgb, uv)
                same = helpers.same(out, want).all(1)
                k = np.nonzero(~same)[0][:4]
                assert same.all(), "%s srgb %d: %d of %d lookups differ (%s), e.g. uv=%r device=%r want=%r" % (
                    name, srgb, (~same).sum(), len(uv), chk.prefix, uv[k].tolist(), out[k].tolist(), want[k].tolist())
