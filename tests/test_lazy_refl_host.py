"""The scene half of the choice of the leaf-list kernel's lazy-reflectance instance (RaylibAMD_SceneLazyRefl, csrc/rl_scene.cc SceneLazyRefl): a plain
scene of triangles whose materials are microfacet -- finite emission, roughness in [2^-10, 1], |albedo| and |metallic| <= 16 -- or mirrors.  No device needed."""
import os

import numpy as np

import helpers
from helpers import scenes

MTL = """newmtl white
Kd %(kd)s
Ks %(ks)s
Ns %(ns)s
%(pr)s
illum 2

newmtl red
Kd 0.63 0.065 0.05
Ks 0 0 0
Ns 10
illum 2

newmtl green
Kd 0.14 0.45 0.091
Ks 0 0 0
Ns 10
illum 2

newmtl light
Kd 0.78 0.78 0.78
Ks 0 0 0
Ns 10
Ke 17 12 4
illum 2
"""


def box_with(path, kd="0.725 0.71 0.68", ks="0 0 0", ns="10", pr=""):
    """The Cornell box, both boxes white, with the white material's constants as given."""
    mtl = MTL % dict(kd=kd, ks=ks, ns=ns, pr=pr)
    return scenes.write_obj(path, scenes.cornell_objects(scenes.WHITE, scenes.WHITE), mtl)[0]


def _session(lib, obj):
    from raylib_amd import binding
    return binding.SceneSession(lib, obj, (0, 1, 4), (0, 1, -1), 45.0, 1.0)


def test_scene_lazy_refl_predicate(lib, workdir):
    d = os.path.join(str(workdir), "lazy_host"); os.makedirs(d, exist_ok=True)
    cases = [
        ("cornell", lambda p: scenes.cornell(p)[0], 1),                                    # microfacet walls, a mirror box; the loader's fallback material is unused
        ("all microfacet", lambda p: box_with(p), 1),
        ("glass box", lambda p: scenes.cornell(p, short_material=scenes.GLASS)[0], 0),     # a dielectric
        ("textured room", lambda p: scenes.textured(p, tess=1)[0], 0),                     # albedo maps, cut-out cards
        ("maps", lambda p: scenes.pbr_maps(p)[0], 0),
        # (the OBJ loader's min(0.95, Kd) -- the reference's -- turns a NaN Kd into 0.95, and the predicate judges the scene it is given; the loader copies a NaN
        #  emission.  NaN albedo, roughness and metallic reach a triangle's material through RaylibAMD_CreateMaterial: test_materials_made_through_the_abi)
        ("NaN Kd", lambda p: box_with(p, kd="nan 0.5 0.5"), 1),
        ("NaN emission", lambda p: scenes.write_obj(p, scenes.cornell_objects(scenes.WHITE, scenes.WHITE), MTL.replace("Ke 17 12 4", "Ke 17 nan 4")
                                                    % dict(kd="0.7 0.7 0.7", ks="0 0 0", ns="10", pr=""))[0], 0),
        ("roughness 0", lambda p: box_with(p, ks="1 1 1", ns="inf"), 0),                   # sqrt(2 / (inf + 2)) = 0
        ("roughness 2^-10", lambda p: box_with(p, pr="Pr 0.0009765625"), 1),               # the interval's lower end
        ("roughness below 2^-10", lambda p: box_with(p, pr="Pr 0.00097"), 0),
        ("roughness 1", lambda p: box_with(p, pr="Pr 1"), 1),                              # the largest value the loader lets through (it saturates)
        ("infinite emission", lambda p: scenes.write_obj(p, scenes.cornell_objects(scenes.WHITE, scenes.WHITE), MTL.replace("Ke 17 12 4", "Ke inf 12 4")
                                                         % dict(kd="0.7 0.7 0.7", ks="0 0 0", ns="10", pr=""))[0], 0),
    ]
    for k, (name, make, want) in enumerate(cases):
        ses = _session(lib, make(os.path.join(d, "s%d.obj" % k)))
        if name in ("NaN Kd", "roughness 0", "roughness 2^-10"):                           # the scene holds what the case means to test
            white = ses.export_flat()[1][0]
            assert (name != "NaN Kd" or white["albedo"][0] == np.float32(0.95)) and (name != "roughness 0" or white["roughness"] == 0.0) \
                and (name != "roughness 2^-10" or white["roughness"] == 2.0 ** -10), (name, white)
        assert lib.RaylibAMD_SceneLazyRefl(ses.scene) == want, name
        if want:
            assert lib.RaylibAMD_ScenePlain(ses.scene) == 1, name
        ses.close()
    # a procedural scene with a Lambertian sphere: not triangles, not microfacet
    from raylib_amd import binding
    mats, spheres, cubes, cam = helpers.procedural_case()
    ps = binding.ProceduralSession(lib, mats, spheres, cubes)
    assert lib.RaylibAMD_SceneLazyRefl(ps.scene) == 0
    ps.close()
    # not finalized / empty / no scene
    sc = lib.Raylib_CreateScene()
    assert lib.RaylibAMD_SceneLazyRefl(sc) == 0
    lib.Raylib_FinalizeScene(sc)
    assert lib.RaylibAMD_SceneLazyRefl(sc) == 0
    lib.Raylib_DestroyScene(sc)
    assert lib.RaylibAMD_SceneLazyRefl(None) == 0


def _triangle_scene(lib, mtype, albedo=(0.5, 0.5, 0.5), roughness=0.5, metallic=0.0, emissive=(0.0, 0.0, 0.0)):
    """Two triangles of one material made with RaylibAMD_CreateMaterial (which saturates a microfacet's albedo, roughness and metallic with compares a NaN
    passes, and leaves a mirror's albedo alone)."""
    import ctypes as C
    f3 = lambda *v: (C.c_float * 3)(*[float(x) for x in v])
    m = lib.RaylibAMD_CreateMaterial(mtype, f3(*albedo), float(roughness), float(metallic), f3(*emissive), 1.0, None, 0.0)
    assert m
    sc = lib.Raylib_CreateScene()
    elems = [lib.RaylibAMD_CreateTriangle(f3(0, 0, z), f3(1, 0, z), f3(0, 1, z), f3(0, 0, 1), f3(0, 0, 1), f3(0, 0, 1), None, m) for z in (0.0, -1.0)]
    assert all(elems)
    for e in elems:
        lib.Raylib_AddSceneElement(sc, e)
    lib.Raylib_FinalizeScene(sc)
    assert lib.RaylibAMD_SceneNumTriangles(sc) == 2
    got = lib.RaylibAMD_SceneLazyRefl(sc), lib.RaylibAMD_ScenePlain(sc)
    lib.Raylib_DestroyScene(sc)
    for e in elems:
        lib.RaylibAMD_DestroySceneElement(e)
    lib.RaylibAMD_DestroyMaterial(m)
    return got


def test_materials_made_through_the_abi(lib):
    """What the OBJ loader cannot produce: NaN and infinite parameters in a triangle's material.  Every compare of the predicate must fail on them."""
    MICROFACET, MIRROR, LAMBERTIAN = 3, 1, 0
    nan, inf = float("nan"), float("inf")
    assert _triangle_scene(lib, MICROFACET) == (1, 1)
    assert _triangle_scene(lib, MIRROR, albedo=(0.9, 0.9, 0.9)) == (1, 1)
    assert _triangle_scene(lib, MIRROR, albedo=(-16.0, 16.0, 0.0)) == (1, 1)                 # the interval's ends, either sign
    assert _triangle_scene(lib, MICROFACET, roughness=2.0 ** -10) == (1, 1)
    assert _triangle_scene(lib, MICROFACET, roughness=7.0) == (1, 1)                       # saturated to 1, the interval's upper end
    for name, kw in (("NaN albedo", dict(albedo=(0.5, nan, 0.5))), ("NaN albedo, first", dict(albedo=(nan, 0.5, 0.5))), ("NaN metallic", dict(metallic=nan)),
                     ("NaN roughness", dict(roughness=nan)), ("roughness 0", dict(roughness=0.0)), ("roughness below 2^-10", dict(roughness=0.0009)),
                     ("NaN emission", dict(emissive=(0.0, nan, 0.0))), ("infinite emission", dict(emissive=(inf, 0.0, 0.0)))):
        assert _triangle_scene(lib, MICROFACET, **kw) == (0, 1), name
    for name, albedo in (("NaN", (0.9, nan, 0.9)), ("inf", (inf, 0.9, 0.9)), ("-inf", (0.9, 0.9, -inf)), ("beyond 16", (0.9, 16.5, 0.9))):
        assert _triangle_scene(lib, MIRROR, albedo=albedo) == (0, 1), name
    assert _triangle_scene(lib, LAMBERTIAN) == (0, 1)
