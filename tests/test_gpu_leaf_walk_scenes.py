"""The leaf-list walk (csrc/rl_dev_walk.h TraverseLeafList) against the tree walk on leaf lists of every record count.  The walk hands its candidate rule
the reciprocal it computed for the box loop instead of a second ExactInv(d): the same bits, so every frame must still be the tree walk's
(RAYLIB_LEAF_LIST=0, whose candidate rule divides for itself) bit for bit, with the same rays, shaded hits and lit paths.  The kernels that inline the
walk are all asked: the hit-queue and the ray-queue form of the lazy-reflectance instance, the eager plain instance (RAYLIB_LAZY_REFL=0) and the general one
(RAYLIB_PLAIN_KERNEL=0).

Frames are 64 x 48 at 4 spp.  The scenes are leaf_walk_scenes.py's: soups of 1 .. 6 records (unused slots in the last record of most), the 24-leaf soup in
which many rays meet every box, the Cornell box (22 leaves); each without and with a sun, so that the occlusion walk runs, at maxPathLength 1 and 5, and 0
(the path that ends before its first ray) on two.  All renders are made once (the module's `runs`)."""
import os

import pytest

import helpers
import leaf_walk_scenes as L

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 4
COUNTERS = ("rays", "shadedHits", "texFetches", "cameraSamples", "pixels", "traceLaunches", "culledCells", "listedCells", "culledSamples", "culledRays")
SCENES = ["soup%d" % r for r in sorted(L.SOUPS)] + ["dense", "cornell"]
SUN = dict(sun=(20, 20, 20), sun_dir=(0.2, -0.3, -1.0))
# the kernel that walks the list: (name, environment, what RaylibAMD_LastTracePlain / LastTraceLazy / LastHitQueue say of it at maxPathLength >= 1)
KERNELS = [("hit queue", {"RAYLIB_HIT_QUEUE": "1"}, (1, 1, 1)), ("ray queue", {"RAYLIB_HIT_QUEUE": "0"}, (1, 1, 0)),
           ("eager plain", {"RAYLIB_LAZY_REFL": "0"}, (1, 0, 0)), ("general", {"RAYLIB_PLAIN_KERNEL": "0"}, (0, 0, 0))]
CASES = [(s, sun, mp) for s in SCENES for sun in (False, True) for mp in (1, 5)] + [("soup6", False, 0), ("soup3", True, 0)]


def _render(lib, ses, max_path, env):
    env = dict(env, RAYLIB_POOL="0")
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        img = ses.render(W, H, SPP, max_path=max_path)
    finally:
        for k, v in keep.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    s = ses.stats()
    counters = {k: getattr(s, k) for k in COUNTERS}
    counters["treeWidth"] = s.treeWidth
    return img, counters, (lib.RaylibAMD_LastTracePlain(), lib.RaylibAMD_LastTraceLazy(), lib.RaylibAMD_LastHitQueue()), s.litPaths


@pytest.fixture(scope="module")
def runs(gpu_lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "leaf_walk"); os.makedirs(d, exist_ok=True)
    objs = dict([("soup%d" % r, L.soup_obj(d, r)) for r in L.SOUPS] + [("dense", L.dense_obj(d)), ("cornell", L.cornell_obj(d))])
    out = {}
    for name in SCENES:
        eye, at = ((0, 1, 4), (0, 1, -1)) if name == "cornell" else (L.EYE, L.AT)
        for sun in (False, True):
            ses = binding.SceneSession(gpu_lib, objs[name], eye, at, 45.0, W / H, **(SUN if sun else {}))
            for (s, sn, mp) in CASES:
                if (s, sn) == (name, sun):
                    out[(s, sn, mp)] = dict([(k, _render(gpu_lib, ses, mp, env)) for k, env, _ in KERNELS] + [("tree", _render(gpu_lib, ses, mp, {"RAYLIB_LEAF_LIST": "0"}))])
            ses.close()
    return out


@pytest.mark.parametrize("scene,sun,max_path", CASES)
def test_leaf_list_walk_is_the_tree_walk(runs, scene, sun, max_path):
    r = runs[(scene, sun, max_path)]
    t, ct, _, _ = r["tree"]
    assert ct["treeWidth"] in (2, 4)                                # the tree walk
    assert ct["cameraSamples"] + ct["culledSamples"] == W * H * SPP
    if max_path >= 1:
        assert ct["rays"] > 0 and ct["shadedHits"] > 0
    for name, _, ran in KERNELS:
        a, ca, ran_a, lit = r[name]
        if max_path < 1 and name == "hit queue":
            ran = (1, 1, 0)                                         # the planner keeps the ray-queue form for a path without a ray
        assert ran_a == ran, (name, ran_a)
        assert ca["treeWidth"] == 0, name                           # the leaf list: no tree
        differ = ~helpers.same(a, t)
        assert not differ.any(), "%s: %d pixels differ from the tree walk" % (name, int(differ.any(-1).sum()))
        assert {k: ca[k] for k in COUNTERS} == {k: ct[k] for k in COUNTERS}, (name, {k: (ca[k], ct[k]) for k in COUNTERS if ca[k] != ct[k]})
        if sun and max_path >= 1 and ran[1]:
            assert lit > 0, name                                    # paths ended in the sun: the occlusion walk ran
