"""The scenes of the leaf-list walk's tests (test_gpu_leaf_walk_scenes.py, test_leaf_walk_host.py), not a test file: triangle soups fixed by seed whose leaf
lists (csrc/rl_bvh.cc "the leaf list") have 1, 2, 3, 4, 5 and 6 records of four leaves, the 24-leaf soup of large overlapping triangles in which many rays
meet every leaf's box, and the Cornell box.  Every soup carries an emitting microfacet material, so that the lazy-reflectance instance takes it and paths end
lit.  Which seed gives which leaf count was found on the host with the builder; test_leaf_walk_host.py checks it again without a device."""
import ctypes as C
import os

from helpers import scenes
from test_lazy_refl_host import MTL

# records of the leaf list -> scenes.soup's arguments and the leaves the builder makes of them.  A scene below 8 triangles has no leaf list, and 8 triangles
# make 4 leaves only where they overlap heavily: the first soup's triangles are large and share a centre.  Leaf counts that are no multiple of 4 leave unused
# slots (the box [+inf, -inf]) in the last record.
SOUPS = {1: dict(n_tris=8, seed=1, extent=0.05, size=0.8, leaves=4), 2: dict(n_tris=8, seed=1, extent=0.6, size=0.5, leaves=7),
         3: dict(n_tris=14, seed=1, extent=0.6, size=0.5, leaves=11), 4: dict(n_tris=19, seed=1, extent=0.6, size=0.5, leaves=15),
         5: dict(n_tris=26, seed=3, extent=0.6, size=0.5, leaves=19), 6: dict(n_tris=32, seed=3, extent=0.6, size=0.5, leaves=23)}
# test_gpu_parity.py test_leaf_list_with_every_leaf_a_candidate: 103 large triangles, 24 leaves
DENSE = dict(n_tris=103, seed=11, extent=0.6, size=1.8, leaves=24)
CORNELL_LEAVES = 22
EYE, AT = (0, 0.2, 4), (0, 0, -1)


def records_of(leaves):
    return (leaves + 3) // 4


def _lit_soup(d, name, **kw):
    obj, _ = scenes.soup(os.path.join(d, name + ".obj"), **kw)
    text = open(obj).read()
    with open(obj, "w") as f:
        f.write("mtllib %s.mtl\n" % name + text.replace("o soup\n", "o soup\nusemtl light\n", 1))
    with open(os.path.join(d, name + ".mtl"), "w") as f:
        f.write(MTL % dict(kd="0.725 0.71 0.68", ks="0 0 0", ns="10", pr=""))
    return obj


def soup_obj(d, records):
    return _lit_soup(d, "soup_r%d" % records, **{k: v for k, v in SOUPS[records].items() if k != "leaves"})


def dense_obj(d):
    return _lit_soup(d, "soup_dense", **{k: v for k, v in DENSE.items() if k != "leaves"})


def cornell_obj(d):
    return scenes.cornell(os.path.join(d, "cornell.obj"))[0]


def leaves_of(lib, ses):
    most = C.c_uint32()
    return lib.RaylibAMD_SceneLeafListInfo(ses.scene, C.byref(most))
