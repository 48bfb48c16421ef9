"""The leaf-list kernel's plain instance (k_trace<16, false, true, 2, PLAIN = true>: no texture, cut-out or sky code).

It is chosen for a scene of at most 108 triangles without texture slots or cut-out leaves, rendered without a sky image; it must
give the bits and the counters of the general instance (RAYLIB_PLAIN_KERNEL=0) on every such scene, and a scene with a texture,
a cut-out or a sky must keep the general instance."""
import os

import numpy as np
import pytest

import helpers
from helpers import golden, tie_mask, assert_same_outside_ties

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "nodesVisited", "trisTested", "shadedHits", "texFetches", "cameraSamples", "culledSamples")


def _render_both(ses, lib, monkeypatch, w, h, spp, **kw):
    monkeypatch.delenv("RAYLIB_PLAIN_KERNEL", raising=False)
    a = ses.render(w, h, spp, **kw)
    plain = lib.RaylibAMD_LastTracePlain()
    sa = ses.stats()
    helpers.assert_planned(lib, ses, sa, w, h, spp, **kw)
    monkeypatch.setenv("RAYLIB_PLAIN_KERNEL", "0")
    b = ses.render(w, h, spp, **kw)
    general = lib.RaylibAMD_LastTracePlain()
    sb = ses.stats()
    helpers.assert_planned(lib, ses, sb, w, h, spp, **kw)
    monkeypatch.delenv("RAYLIB_PLAIN_KERNEL")
    assert sa.treeWidth == 0 and sb.treeWidth == 0, "not the leaf-list kernel"
    assert general == 0
    return a, b, plain, sa, sb


def _pbr_constants_mtl(seed):
    """PBR_MTL's material names with random microfacet constants (Pr / Ns / Ks / Pm / Ke) and no map statement."""
    rng = np.random.RandomState(seed)
    text = helpers.scenes.random_pbr_mtl(rng)
    return "\n".join(l for l in text.split("\n") if not l.startswith(("map_", "norm"))) + "\n"


def _plain_sessions(lib, workdir):
    from raylib_amd import binding
    out = []
    for name in ("cornell", "cornell_glass_sun", "cornell_flat_normals"):
        out.append((name, helpers.session_for_case(lib, name, workdir)))
    d = os.path.join(str(workdir), "plain_mirror"); os.makedirs(d, exist_ok=True)
    obj, _ = helpers.scenes.cornell(os.path.join(d, "mirror.obj"), tall_material=helpers.scenes.MIRROR, short_material=helpers.scenes.MIRROR)
    out.append(("mirror", binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 16 / 9)))
    for seed in (3, 8):
        d = os.path.join(str(workdir), "plain_pbr_%d" % seed); os.makedirs(d, exist_ok=True)
        obj, n = helpers.scenes.pbr_maps(os.path.join(d, "pbr.obj"), mtl=_pbr_constants_mtl(seed))
        assert n <= 108
        out.append(("pbr_constants_%d" % seed, binding.SceneSession(lib, obj, (0.1, 1.1, 4), (0, 0.95, -1), 45.0, 1.0)))
    return out


def test_plain_instance_is_bit_identical_to_the_general_one(gpu_lib, workdir, monkeypatch):
    monkeypatch.setenv("RAYLIB_POOL", "0")
    for name, ses in _plain_sessions(gpu_lib, workdir):
        assert gpu_lib.RaylibAMD_ScenePlain(ses.scene) == 1, name
        # configs[0] and configs[1] shapes at reduced size (square and 16:9), long paths too
        for (w, h, spp, mp) in ((128, 128, 4, 5), (192, 108, 8, 5), (96, 64, 2, 12)):
            a, b, plain, sa, sb = _render_both(ses, gpu_lib, monkeypatch, w, h, spp, max_path=mp)
            assert plain == 1, (name, "the plain instance was not chosen")
            assert helpers.same(a, b).all(), (name, w, h, spp, int((~helpers.same(a, b)).any(-1).sum()))
            for k in COUNTERS:
                assert getattr(sa, k) == getattr(sb, k), (name, k, getattr(sa, k), getattr(sb, k))
            assert sa.texFetches == 0
        ses.close()


def test_cornell_goldens_through_the_plain_instance(gpu_lib, oracle, workdir, monkeypatch):
    """The reference's own renders (tests/golden) of the untextured, sky-less cases, through the plain instance."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    for name in ("cornell", "cornell_glass_sun"):
        g = golden(name)
        ses = helpers.session_for_case(gpu_lib, name, workdir)
        obj, c, flat = helpers.flat_for_case(name, workdir, oracle)
        ties = tie_mask(oracle, flat, helpers.ffi.make_camera(c["origin"], c["look_at"], c["fov"], c["aspect"]), 64, 64)
        img = ses.render(64, 64, 4)
        assert gpu_lib.RaylibAMD_LastTracePlain() == 1, name
        helpers.assert_planned(gpu_lib, ses, ses.stats(), 64, 64, 4)
        assert_same_outside_ties(img, g["mode0_spp4"], ties, name)
        ses.close()


def test_textures_cutouts_and_sky_keep_the_general_instance(gpu_lib, oracle, workdir, monkeypatch):
    monkeypatch.setenv("RAYLIB_POOL", "0")
    # a textured scene (normal / roughness / metallic / emissive / albedo maps) and a cut-out card with a sky: against the reference's renders
    for name in ("pbr_maps", "cutout_sky"):
        g = golden(name)
        ses = helpers.session_for_case(gpu_lib, name, workdir)
        assert gpu_lib.RaylibAMD_ScenePlain(ses.scene) == 0, name
        obj, c, flat = helpers.flat_for_case(name, workdir, oracle)
        ties = tie_mask(oracle, flat, helpers.ffi.make_camera(c["origin"], c["look_at"], c["fov"], c["aspect"]), 64, 64)
        img = ses.render(64, 64, 4)
        assert ses.stats().treeWidth == 0 and gpu_lib.RaylibAMD_LastTracePlain() == 0, name
        helpers.assert_planned(gpu_lib, ses, ses.stats(), 64, 64, 4)
        assert_same_outside_ties(img, g["mode0_spp4"], ties, name)
        ses.close()
    # the cut-out scene without a sky: the cut-out bit alone keeps the general instance
    from raylib_amd import binding
    d = os.path.join(str(workdir), "plain_cutout"); os.makedirs(d, exist_ok=True)
    obj, _ = helpers.scenes.cutout(os.path.join(d, "cutout.obj"))
    ses = binding.SceneSession(gpu_lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    assert gpu_lib.RaylibAMD_ScenePlain(ses.scene) == 0
    img = ses.render(96, 96, 4)
    assert ses.stats().treeWidth == 0 and gpu_lib.RaylibAMD_LastTracePlain() == 0
    helpers.assert_planned(gpu_lib, ses, ses.stats(), 96, 96, 4)
    monkeypatch.setenv("RAYLIB_LEAF_LIST", "0")   # the BVH4 walk of the same scene: an independent kernel
    ref = ses.render(96, 96, 4)
    monkeypatch.delenv("RAYLIB_LEAF_LIST")
    assert helpers.same(img, ref).all()
    ses.close()
    # the plain Cornell box WITH a sky image: the per-render condition; the sky is read on every miss
    ses = binding.SceneSession(gpu_lib, helpers.build_case("cornell", workdir)[0], (0, 1, 4), (0, 1, -1), 45.0, 16 / 9, sky_image=helpers.scenes.sky_panorama())
    assert gpu_lib.RaylibAMD_ScenePlain(ses.scene) == 1
    img = ses.render(160, 90, 4)
    assert ses.stats().treeWidth == 0 and gpu_lib.RaylibAMD_LastTracePlain() == 0
    helpers.assert_planned(gpu_lib, ses, ses.stats(), 160, 90, 4)
    assert ses.stats().texFetches > 0
    monkeypatch.setenv("RAYLIB_LEAF_LIST", "0")
    ref = ses.render(160, 90, 4)
    monkeypatch.delenv("RAYLIB_LEAF_LIST")
    assert helpers.same(img, ref).all()
    ses.close()
