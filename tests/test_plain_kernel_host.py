"""The scene half of the choice of the leaf-list kernel's plain instance (RaylibAMD_ScenePlain, csrc/rl_scene.cc ScenePlain): no material
with a texture slot, no leaf of the leaf list with the cut-out bit.  No device needed."""
import os

import numpy as np

import helpers
from helpers import scenes


def _session(lib, obj, **kw):
    from raylib_amd import binding
    return binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0, **kw)


def test_scene_plain_predicate(lib, workdir):
    d = os.path.join(str(workdir), "plain_host"); os.makedirs(d, exist_ok=True)
    cases = [
        (lambda p: scenes.cornell(p), 1),
        (lambda p: scenes.cornell(p, short_material=scenes.GLASS), 1),
        (lambda p: scenes.cornell(p, tess=2), 1),                       # no leaf list (144 triangles): still no texture
        (lambda p: scenes.cutout(p), 0),                                # alpha-tested albedo map: cut-out leaves
        (lambda p: scenes.pbr_maps(p), 0),                              # normal / roughness / metallic / emissive maps
    ]
    for k, (make, want) in enumerate(cases):
        obj = make(os.path.join(d, "s%d.obj" % k))[0]
        ses = _session(lib, obj)
        assert lib.RaylibAMD_ScenePlain(ses.scene) == want, k
        ses.close()
    # one map on one material is enough, whatever its slot (albedo 0, normal 1, roughness 2, metallic 3, emissive 4)
    tex = np.ones((4, 4, 4), np.float32)
    for slot in range(5):
        obj = scenes.cornell(os.path.join(d, "slot%d.obj" % slot))[0]
        ses = _session(lib, obj, textures=[("white", slot, tex)])
        assert lib.RaylibAMD_ScenePlain(ses.scene) == 0, slot
        ses.close()
    # a sky image is a per-render condition, not the scene's
    obj = scenes.cornell(os.path.join(d, "sky.obj"))[0]
    ses = _session(lib, obj, sky_image=scenes.sky_panorama())
    assert lib.RaylibAMD_ScenePlain(ses.scene) == 1
    ses.close()
    # not finalized / no scene
    sc = lib.Raylib_CreateScene()
    assert lib.RaylibAMD_ScenePlain(sc) == 0
    lib.Raylib_FinalizeScene(sc)
    assert lib.RaylibAMD_ScenePlain(sc) == 1
    lib.Raylib_DestroyScene(sc)
    assert lib.RaylibAMD_ScenePlain(None) == 0

