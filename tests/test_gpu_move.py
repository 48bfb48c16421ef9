"""RaylibAMD_SceneMoveTriangles on the device: after a move, every call on the scene returns the bits it returns on a scene created from the moved triangles.

The oracle throughout is that second scene (tests/move_cases.py), finalized and given the same call; comparisons are on the float bits.  Scenes are the smallest
that reach each structure: a soup of 600 triangles walked on the binary tree, the 4-wide float boxes, the 4-wide grid and the 8-wide tree (the planner's
switches, asserted through RaylibAMD_PlanRender / PlanRayQuery and the stats' treeWidth), the Cornell box (LDS scene, leaf list, lazy and plain instances),
spheres and a moving cube beside triangles, and the cut-out scene under a sky panorama.  Frames of 64 x 48 at 4 spp, path length 5."""
import ctypes as C
import os

import numpy as np
import pytest
import torch    # before the library is loaded: the device entry is handed torch's tensors, and both must run on one HIP runtime

import helpers
import move_cases as mc
from raylib_amd import binding

pytestmark = pytest.mark.gpu
F = np.float32

# name -> (the planner's switches, RaylibAMDRenderPlan.tree, the render's treeWidth, the queries' treeWidth)
STRUCTURES = {
    "binary": ({"RAYLIB_POOL": "0", "RAYLIB_BVH4": "0", "RAYLIB_QUERY_TREE": "2"}, 1, 2, 2),
    "box4": ({"RAYLIB_POOL": "0", "RAYLIB_QUERY_TREE": "2"}, 2, 4, 2),
    "grid4": ({"RAYLIB_POOL": "2", "RAYLIB_BVH8": "0", "RAYLIB_QUERY_TREE": "4"}, 3, 4, 4),
    "wide8": ({"RAYLIB_POOL": "2", "RAYLIB_BVH8": "1", "RAYLIB_QUERY_TREE": "8"}, 4, 8, 8),
}
QUERY_KINDS = (binding.QUERY_ANY, binding.QUERY_CLOSEST, binding.QUERY_SURFACE)


def use_structure(monkeypatch, name):
    for k in ("RAYLIB_POOL", "RAYLIB_BVH4", "RAYLIB_BVH8", "RAYLIB_QUERY_TREE", "RAYLIB_LAZY_REFL", "RAYLIB_LEAF_LIST", "RAYLIB_LDS_SCENE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in STRUCTURES[name][0].items():
        monkeypatch.setenv(k, v)


def render_on(lib, ses, structure=None):
    """A frame of the session; with a structure, the launch is asserted to have walked it (a combination that does not reach the tree fails here)."""
    img = ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH)
    if structure is not None:
        plan = helpers.assert_planned(lib, ses, ses.stats(), mc.W, mc.H, mc.SPP, mc.MAX_PATH)
        assert plan["tree"] == STRUCTURES[structure][1] and ses.stats().treeWidth == STRUCTURES[structure][2], (structure, plan)
    return img


def queries_on(lib, ses, rays, structure=None):
    """ANY, CLOSEST and SURFACE records with the primitive, as bytes; with a structure, each query is asserted to have walked its tree."""
    out = []
    for kind in QUERY_KINDS:
        got = binding.trace_rays(lib, ses.scene, rays, kind, with_prim=(kind == binding.QUERY_SURFACE))
        if structure is not None:
            rc, plan = binding.plan_ray_query(lib, ses.scene, kind)
            assert rc == 1 and plan["treeWidth"] == STRUCTURES[structure][3] and ses.stats().treeWidth == STRUCTURES[structure][3], (structure, plan)
        out += [a.tobytes() for a in (got if isinstance(got, tuple) else (got,))]
    return out


def rigid(tris, lo, hi):
    """Triangles [lo, hi) turned about z by the angle whose cosine and sine are 3/5 and 4/5 and shifted: a rigid move of a contiguous range."""
    rot = np.array([[0.6, -0.8, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]])
    out = np.array(tris, np.float64, copy=True)
    out[lo:hi] = out[lo:hi] @ rot.T + np.array([0.4, -0.3, 0.5])
    return out.astype(F).astype(np.float64)


@pytest.fixture(scope="module")
def soup():
    # (this seed: the 4-wide tree of the soup and of every variant the tests below make of it needs at most the 16 stack entries of k_trace's smallest
    #  instance, so RAYLIB_POOL=0 walks the float boxes; another soup may fall back to the binary tree there, and render_on says so)
    return mc.soup_triangles(600, seed=12)


@pytest.fixture(scope="module")
def rays():
    return mc.query_rays()


def assert_trees(lib, ses, refitted=True):
    """What the device holds of a moved scene: the builder's validity checks pass on it (containment); every wide format is, byte for byte, the host's rule
    applied to the device's binary boxes (RaylibAMD_SceneCompareTrees); and the binary boxes are move_cases.refit_boxes of the moved triangles -- bit for bit
    where the device's refit wrote them last (refitted), as values behind a rebuild."""
    assert mc.check_trees(lib, ses.scene) == (1, 0)
    mc.assert_wide_trees_exact(lib, ses.scene)
    mc.assert_refit_exact(lib, ses, bits=refitted)


# ---- case 1: a rigid move of a contiguous third, through either entry, on every structure ----
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("structure", list(STRUCTURES))
def test_rigid_move_soup(gpu_lib, workdir, monkeypatch, soup, rays, structure, device):
    use_structure(monkeypatch, structure)
    tag = "%s_%d" % (structure, device)
    ses = mc.soup_session(gpu_lib, workdir, "rigid_a_" + tag, soup)
    fresh = mc.soup_session(gpu_lib, workdir, "rigid_b_" + tag, rigid(soup, 200, 400))
    want_img, want_q = render_on(gpu_lib, fresh, structure), queries_on(gpu_lib, fresh, rays, structure)
    before = render_on(gpu_lib, ses, structure)       # (the scene is on the device, with the plan's tree, before it moves)
    assert not mc.same_bits(before, want_img)
    rc, first, end = mc.move_to(gpu_lib, ses, fresh, device)
    assert (rc, first, end) == (1, 200, 400)
    assert mc.same_bits(render_on(gpu_lib, ses, structure), want_img)
    assert queries_on(gpu_lib, ses, rays, structure) == want_q
    assert mc.export(ses).tobytes() == mc.export(fresh).tobytes()
    assert_trees(gpu_lib, ses)
    ses.close(); fresh.close()


def test_trees_uploaded_after_a_move_are_refitted(gpu_lib, workdir, monkeypatch, soup, rays):
    """A wide tree the device did not hold when the triangles moved is uploaded from the host's copy, which must have been refitted first: the move happens
    under the binary tree's switches, then every other structure renders and answers queries."""
    use_structure(monkeypatch, "binary")
    ses = mc.soup_session(gpu_lib, workdir, "late_a", soup)
    fresh = mc.soup_session(gpu_lib, workdir, "late_b", rigid(soup, 200, 400))
    render_on(gpu_lib, ses, "binary")
    assert mc.move_to(gpu_lib, ses, fresh, True)[0] == 1
    for structure in ("wide8", "grid4", "box4", "binary"):
        use_structure(monkeypatch, structure)
        assert mc.same_bits(render_on(gpu_lib, ses, structure), render_on(gpu_lib, fresh, structure)), structure
        assert queries_on(gpu_lib, ses, rays, structure) == queries_on(gpu_lib, fresh, rays, structure), structure
    assert_trees(gpu_lib, ses)
    ses.close(); fresh.close()


# ---- the Cornell box: LDS scene, leaf list, the lazy and the eager plain instance ----
def cornell_pair(lib, workdir, tag, move_v, move_vn=None):
    obj, _ = helpers.build_case("cornell", os.path.join(str(workdir), "move_" + tag))
    moved = mc.edit_obj(obj, os.path.join(os.path.dirname(obj), "moved_" + tag + ".obj"), move_v, move_vn)
    return mc.case_session(lib, "cornell", obj), mc.case_session(lib, "cornell", moved)


def shift_some(k, p, lo=8, hi=20, d=(0.11, 0.07, -0.13)):
    return p + np.asarray(d, F) if lo <= k < hi else p


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("lazy", ["1", "0"], ids=["lazy", "plain"])
def test_rigid_move_cornell(gpu_lib, workdir, monkeypatch, lazy, device):
    use_structure(monkeypatch, "box4")
    monkeypatch.delenv("RAYLIB_POOL")       # the planner's own choice for a scene this small: k_trace, the scene in LDS, its leaf list
    monkeypatch.setenv("RAYLIB_LAZY_REFL", lazy)
    ses, fresh = cornell_pair(gpu_lib, workdir, "rigid_%s_%d" % (lazy, device), shift_some)
    want = fresh.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH)
    plan = helpers.assert_planned(gpu_lib, fresh, fresh.stats(), mc.W, mc.H, mc.SPP, mc.MAX_PATH)
    assert plan["lds"] == 2 and plan["plain"] == 1 and plan["lazy"] == int(lazy) and gpu_lib.RaylibAMD_LastTraceLazy() == int(lazy), plan
    assert not mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), want)
    assert mc.move_to(gpu_lib, ses, fresh, device)[0] == 1
    assert mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), want)
    assert helpers.assert_planned(gpu_lib, ses, ses.stats(), mc.W, mc.H, mc.SPP, mc.MAX_PATH)["lds"] == 2
    assert mc.export(ses).tobytes() == mc.export(fresh).tobytes()
    assert_trees(gpu_lib, ses)
    ses.close(); fresh.close()


# ---- spheres and a moving cube beside triangles ----
def procedural_pair(lib, move):
    mats, sph, cub, cam = helpers.procedural_case()
    tris = mc.quad_triangles([(-1.5, -0.45, 0.9), (-0.7, -0.45, 0.9), (-0.7, 0.5, 0.7), (-1.5, 0.5, 0.7)], (0, 0.2, 1), 2) + \
        mc.quad_triangles([(0.6, -0.4, 0.8), (1.1, -0.4, 0.8), (1.1, 0.2, 0.6), (0.6, 0.2, 0.6)], (0, 0.3, 1), 4)
    moved = [(np.asarray(v, F) + (np.asarray(move, F) if i >= 2 else F(0)), n, uv, m) for i, (v, n, uv, m) in enumerate(tris)]
    kw = dict(spheres=sph, cubes=cub, origin=cam["origin"], look_at=cam["look_at"], fov=cam["fov"], aspect=cam["aspect"], shutter=cam["shutter"], sun=cam["sun"], sun_dir=cam["sun_dir"])
    return mc.ElementSession(lib, mats, tris, **kw), mc.ElementSession(lib, mats, moved, **kw)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_rigid_move_beside_spheres_and_a_moving_cube(gpu_lib, rays, device):
    ses, fresh = procedural_pair(gpu_lib, (-0.9, 0.5, -0.4))
    want, want_q = fresh.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), queries_on(gpu_lib, fresh, rays)
    assert fresh.stats().treeWidth == 2
    assert not mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), want)
    assert mc.move_to(gpu_lib, ses, fresh, device) == (1, 2, 4)
    assert mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), want)
    assert queries_on(gpu_lib, ses, rays) == want_q
    assert_trees(gpu_lib, ses)
    # another shutter interval rebuilds the scene of a moving cube on the host: from the MOVED triangles
    for s in (ses, fresh):
        gpu_lib.Raylib_CameraSetMotion(s.camera, 0.0, 0.5)
    assert mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), fresh.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH))
    ses.close(); fresh.close()


# ---- alpha-tested leaves under a sky panorama ----
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_rigid_move_cutout_sky(gpu_lib, workdir, rays, device):
    obj, _ = helpers.build_case("cutout_sky", os.path.join(str(workdir), "move_cutout_%d" % device))
    n_v = sum(1 for line in open(obj) if line.startswith("v "))
    moved = mc.edit_obj(obj, os.path.join(os.path.dirname(obj), "moved.obj"), lambda k, p: p + np.asarray((0.2, 0.1, 0.15), F) if k >= n_v - 8 else p)
    ses, fresh = mc.case_session(gpu_lib, "cutout_sky", obj), mc.case_session(gpu_lib, "cutout_sky", moved)
    want, want_q = fresh.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), queries_on(gpu_lib, fresh, rays)
    assert not mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), want)
    assert mc.move_to(gpu_lib, ses, fresh, device)[0] == 1
    assert mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), want)
    assert queries_on(gpu_lib, ses, rays) == want_q
    assert_trees(gpu_lib, ses)
    ses.close(); fresh.close()


# ---- case 2: a move far outside the old bounds: the cull's bounds grow where the triangle went and shrink where it left ----
def outlier(soup, x):
    t = np.array(soup[:300], np.float64, copy=True)
    t[0] = np.array([[x - 0.5, -0.5, 0.0], [x + 0.5, -0.5, 0.1], [x, 0.6, 0.0]])
    return t


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("structure", list(STRUCTURES))
def test_move_far_outside_the_old_bounds(gpu_lib, workdir, monkeypatch, soup, structure, device):
    use_structure(monkeypatch, structure)
    tag = "%s_%d" % (structure, device)
    ses = mc.soup_session(gpu_lib, workdir, "far_a_" + tag, outlier(soup, -10.0))
    fresh = mc.soup_session(gpu_lib, workdir, "far_b_" + tag, outlier(soup, 10.0))
    there = binding.create_camera(gpu_lib, (10, 0, 6), (10, 0, 0), 30.0, mc.W / mc.H)    # sees only where the triangle goes
    left = binding.create_camera(gpu_lib, (-10, 0, 6), (-10, 0, 0), 30.0, mc.W / mc.H)   # ... and only where it was
    whole = mc.W * mc.H * mc.SPP
    assert not mc.render_camera(gpu_lib, ses, there)[..., :3].any() and ses.stats().culledSamples == whole     # empty, and outside the old bounds: every cell dropped
    assert mc.render_camera(gpu_lib, ses, left)[..., :3].any()
    assert mc.move_to(gpu_lib, ses, fresh, device) == (1, 0, 1)
    got = mc.render_camera(gpu_lib, ses, there)
    assert got[..., :3].any(), "the moved triangle does not appear: stale bounds"
    assert mc.same_bits(got, mc.render_camera(gpu_lib, fresh, there))
    got = mc.render_camera(gpu_lib, ses, left)
    assert not got[..., :3].any() and ses.stats().culledSamples == whole, "the bounds did not shrink"
    assert mc.same_bits(got, mc.render_camera(gpu_lib, fresh, left)) and fresh.stats().culledSamples == whole
    assert mc.same_bits(render_on(gpu_lib, ses, structure), render_on(gpu_lib, fresh, structure))
    assert_trees(gpu_lib, ses)
    for cam in (there, left):
        gpu_lib.Raylib_DestroyCamera(cam)
    ses.close(); fresh.close()


# ---- case 3: move, render, move back, render ----
@pytest.mark.parametrize("structure", list(STRUCTURES))
def test_move_and_move_back(gpu_lib, workdir, monkeypatch, soup, rays, structure):
    use_structure(monkeypatch, structure)
    ses = mc.soup_session(gpu_lib, workdir, "back_a_" + structure, soup)
    fresh = mc.soup_session(gpu_lib, workdir, "back_b_" + structure, rigid(soup, 200, 400))
    origin = mc.soup_session(gpu_lib, workdir, "back_c_" + structure, soup)
    first, first_q = render_on(gpu_lib, ses, structure), queries_on(gpu_lib, ses, rays, structure)
    h0, t0 = gpu_lib.RaylibAMD_SceneBVHHash(ses.scene), gpu_lib.RaylibAMD_SceneTopologyHash(ses.scene)
    assert mc.move_to(gpu_lib, ses, fresh, True)[0] == 1
    assert gpu_lib.RaylibAMD_SceneTopologyHash(ses.scene) == t0 != gpu_lib.RaylibAMD_SceneTopologyHash(fresh.scene)      # the topology is kept: not the fresh scene's
    assert mc.same_bits(render_on(gpu_lib, ses, structure), render_on(gpu_lib, fresh, structure))
    assert mc.move_to(gpu_lib, ses, origin, False)[0] == 1
    assert mc.same_bits(render_on(gpu_lib, ses, structure), first) and queries_on(gpu_lib, ses, rays, structure) == first_q
    assert gpu_lib.RaylibAMD_SceneBVHHash(ses.scene) == h0 and gpu_lib.RaylibAMD_SceneTopologyHash(ses.scene) == t0      # (the boxes are the builder's again: exact unions, the host's selection of zeros)
    assert_trees(gpu_lib, ses)
    for s in (ses, fresh, origin):
        s.close()


def test_move_and_move_back_cornell(gpu_lib, workdir):
    ses, fresh = cornell_pair(gpu_lib, workdir, "back", shift_some)
    origin, _ = cornell_pair(gpu_lib, workdir, "back0", lambda k, p: p)
    first = ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH)
    assert mc.move_to(gpu_lib, ses, fresh, False)[0] == 1
    assert mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), fresh.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH))
    assert mc.move_to(gpu_lib, ses, origin, True)[0] == 1
    assert mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), first)
    for s in (ses, fresh, origin, _):
        s.close()


# ---- case 4: degenerate and edge records ----
POINT = np.array([[0.25, 0.5, -0.25]] * 3)
SEGMENT = np.array([[0.25, 0.5, -0.25], [0.375, 0.5, -0.25], [0.5, 0.5, -0.25]])     # u = (1/8, 0, 0), v = (1/4, 0, 0): uv uv = uu vv exactly, denom = 0
TINY = np.array([[0, 0, 0], [1e-5, 0, 0], [0, 1e-5, 0]])                             # denom = -1e-20: nonzero, below 2^-62 -- the scene leaves the short divisions


def in_the_roots_split(lib, scene, size=0.15):
    """A triangle lying exactly in the plane in which the built tree's root splits the scene (the tree is read back: RaylibAMD_SceneExportBVHNodes): along the
    axis on which the root's two child boxes are furthest apart, the upper face of the lower child's box -- a face the other child's box reaches across, so the
    plane is the one both meet in --, in the middle of that face.  The triangle's own box has no extent along that axis."""
    root = mc.bvh_nodes(lib, scene)[0]
    assert root["left"] >= 0 and root["right"] >= 0, "the root's children are inner nodes"
    lo, hi = (root["lmin"], root["lmax"]), (root["rmin"], root["rmax"])
    centre = lambda b: 0.5 * (b[0].astype(np.float64) + b[1])
    axis = int(np.argmax(np.abs(centre(lo) - centre(hi))))
    if centre(lo)[axis] > centre(hi)[axis]:
        lo, hi = hi, lo
    c = lo[1][axis]
    assert hi[0][axis] <= c <= hi[1][axis], "the lower child's upper face lies within the upper child's box: the plane of the split"
    u, v = [k for k in range(3) if k != axis]
    t = np.zeros((3, 3), np.float64)
    t[:, axis] = c
    mu, mv = 0.5 * (float(lo[0][u]) + float(lo[1][u])), 0.5 * (float(lo[0][v]) + float(lo[1][v]))     # the face's middle; a triangle of the soup's size
    t[0, u], t[0, v] = mu - size, mv - size
    t[1, u], t[1, v] = mu + size, mv
    t[2, u], t[2, v] = mu, mv + size
    return t.astype(F).astype(np.float64)


def with_triangles(soup, edits):
    t = np.array(soup, np.float64, copy=True)
    for k, v in edits.items():
        t[k] = v
    return t.astype(F).astype(np.float64)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("structure", list(STRUCTURES))
def test_degenerate_and_edge_records(gpu_lib, workdir, monkeypatch, soup, rays, structure, device):
    use_structure(monkeypatch, structure)
    tag = "%s_%d" % (structure, device)
    ses = mc.soup_session(gpu_lib, workdir, "edge_a_" + tag, soup)
    first, first_q = render_on(gpu_lib, ses, structure), queries_on(gpu_lib, ses, rays, structure)
    FLAT = in_the_roots_split(gpu_lib, ses.scene)
    steps = [("point and segment", {100: POINT, 101: SEGMENT}), ("a divisor below 2^-62 comes in", {100: POINT, 101: SEGMENT, 300: TINY}),
             ("in the root's splitting plane", {100: POINT, 101: SEGMENT, 300: TINY, 450: FLAT}), ("the last such divisor goes out", {100: POINT, 101: SEGMENT, 450: FLAT})]
    for i, (what, edits) in enumerate(steps):
        fresh = mc.soup_session(gpu_lib, workdir, "edge_b%d_%s" % (i, tag), with_triangles(soup, edits))
        assert mc.move_to(gpu_lib, ses, fresh, device)[0] == 1, what
        assert mc.same_bits(render_on(gpu_lib, ses, structure), render_on(gpu_lib, fresh, structure)), what
        assert queries_on(gpu_lib, ses, rays, structure) == queries_on(gpu_lib, fresh, rays, structure), what
        assert mc.same_triangles(mc.export(ses), mc.export(fresh)), what
        assert_trees(gpu_lib, ses)
        fresh.close()
    origin = mc.soup_session(gpu_lib, workdir, "edge_c_" + tag, soup)
    assert mc.move_to(gpu_lib, ses, origin, device)[0] == 1
    assert mc.same_bits(render_on(gpu_lib, ses, structure), first) and queries_on(gpu_lib, ses, rays, structure) == first_q
    ses.close(); origin.close()


def test_degenerate_records_in_the_leaf_list(gpu_lib, workdir):
    """The Cornell box with three vertices of a quad in one point and two of its neighbour on a segment through it -- a triangle that is a point, triangles that
    are segments --, then all of them back."""
    def collapse(k, p):
        if k in (8, 9, 10):
            return np.asarray(POINT[0], F) + F(0.25)
        if k in (12, 13):
            return np.asarray(SEGMENT[k - 12], F) + F(0.25)
        return p
    ses, fresh = cornell_pair(gpu_lib, workdir, "collapse", collapse)
    first = ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH)
    for device in (False, True):
        assert mc.move_to(gpu_lib, ses, fresh, device)[0] == 1
        assert mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), fresh.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH))
        assert helpers.assert_planned(gpu_lib, ses, ses.stats(), mc.W, mc.H, mc.SPP, mc.MAX_PATH)["lds"] == 2
        assert_trees(gpu_lib, ses)
        origin, other = cornell_pair(gpu_lib, workdir, "collapse0_%d" % device, lambda k, p: p)
        assert mc.move_to(gpu_lib, ses, origin, device)[0] == 1
        assert mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), first)
        origin.close(); other.close()
    ses.close(); fresh.close()


# ---- case 5: with normals given, and with NULL ----
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_normals_given_and_kept(gpu_lib, workdir, device):
    turn = lambda k, n: np.asarray((n[0] * 0.6 - n[2] * 0.8, n[1], n[0] * 0.8 + n[2] * 0.6), F)
    ses, both = cornell_pair(gpu_lib, workdir, "normals_%d" % device, shift_some, turn)       # other vertices and other shading normals
    a, b = mc.export(ses), mc.export(both)
    first, end = mc.changed_range(a, b)
    assert (helpers.bits(mc.nrm9(a)) != helpers.bits(mc.nrm9(b))).any()
    kept = b.copy()
    for k in ("n0", "n1", "n2"):
        kept[k] = a[k]
    want = both.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH)
    to = (lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()) if device else (lambda x: x)
    # NULL keeps the shading normals: the export says so, and the frame differs from the scene whose normals turned
    assert binding.move_triangles(gpu_lib, ses.scene, first, to(mc.pos9(b[first:end]))) == 1
    assert mc.export(ses).tobytes() == kept.tobytes()
    img = ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH)
    assert not mc.same_bits(img, want)
    # ... and given, they change: the scene loaded with those normals
    assert binding.move_triangles(gpu_lib, ses.scene, first, to(mc.pos9(b[first:end])), to(mc.nrm9(b[first:end]))) == 1
    assert mc.export(ses).tobytes() == b.tobytes()
    assert mc.same_bits(ses.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH), want)
    # the kept-normals frame against a fresh scene with those normals: the vertices moved in the file, the normal lines as they were
    ses.close(); both.close()
    ses, only_v = cornell_pair(gpu_lib, workdir, "normals_kept_%d" % device, shift_some)
    assert mc.export(only_v).tobytes() == kept.tobytes()
    assert mc.same_bits(img, only_v.render(mc.W, mc.H, mc.SPP, mc.MAX_PATH))
    ses.close(); only_v.close()


# ---- case 6: count == 0 and every refusal; a refused call leaves the old bits ----
def test_refusals_leave_the_scene_as_it_was(gpu_lib, workdir, soup, rays):
    ses = mc.soup_session(gpu_lib, workdir, "refuse", soup)
    first, first_q, tris = render_on(gpu_lib, ses), queries_on(gpu_lib, ses, rays), mc.export(ses)
    n = len(tris)
    P = mc.pos9(tris[:8]) + F(0.5)
    dP = torch.from_numpy(P).cuda()
    move, moved = gpu_lib.RaylibAMD_SceneMoveTriangles, gpu_lib.RaylibAMD_SceneMoveTrianglesDevice
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    dev = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert move(ses.scene, 0, 0, None, None) == 1 and moved(ses.scene, n, 0, None, None, None) == 1
    assert move(ses.scene, n - 7, 8, fp(P), None) == 0 and moved(ses.scene, -1, 8, dev(dP), None, None) == 0 and moved(ses.scene, 0, 8, None, None, None) == 0
    assert moved(ses.scene, 0, 8, C.c_void_p(P.ctypes.data), None, None) == 0                 # host memory through the device entry
    assert moved(ses.scene, 0, 7, dev(dP, 2), None, None) == 0                                # misaligned
    assert moved(ses.scene, 0, 8, dev(dP), C.c_void_p(P.ctypes.data), None) == 0              # the normals off the device
    bad = P.copy(); bad[3, 4] = np.nan
    assert move(ses.scene, 0, 8, fp(bad), None) == 0
    dBad = torch.from_numpy(bad).cuda()
    assert moved(ses.scene, 0, 8, dev(dBad), None, None) == 0                                 # the library's stream: synchronous, the kernel's flag is the answer
    assert moved(ses.scene, 0, 8, dev(dP), dev(dBad), None) == 0
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        assert binding.move_triangles(gpu_lib, ses.scene, 0, dBad) == 1                       # enqueued: accepted, found out on the device, not applied
    prog = binding.Progressive(ses, mc.W, mc.H, 8)
    assert prog.handle and move(ses.scene, 0, 8, fp(P), None) == 0 and moved(ses.scene, 0, 8, dev(dP), None, None) == 0
    prog.close()
    assert mc.same_bits(render_on(gpu_lib, ses), first) and queries_on(gpu_lib, ses, rays) == first_q
    assert mc.export(ses).tobytes() == tris.tobytes()
    assert_trees(gpu_lib, ses)
    assert move(ses.scene, 0, 8, fp(P), None) == 1                                            # ... and the same call without a reason to refuse it moves
    assert not mc.same_bits(render_on(gpu_lib, ses), first)
    ses.close()


# ---- case 7: radiance, gather, and a lightmap of a moved quad ----
def room_pair(lib, move):
    mats, _, _, _ = helpers.procedural_case()
    floor = mc.quad_triangles([(-2, -0.5, 2), (2, -0.5, 2), (2, -0.5, -2), (-2, -0.5, -2)], (0, 1, 0), 2)
    lamp = mc.quad_triangles([(-0.5, 1.5, -0.5), (-0.5, 1.5, 0.5), (0.5, 1.5, 0.5), (0.5, 1.5, -0.5)], (0, -1, 0), 4)
    quad = mc.quad_triangles([(-0.6, -0.2, -0.3), (0.4, -0.2, -0.3), (0.4, 0.1, 0.5), (-0.6, 0.1, 0.5)], (0, 1, 0), 3)
    tris = floor + lamp + quad
    moved = [(np.asarray(v, F) + (np.asarray(move, F) if i >= 4 else F(0)), n, uv, m) for i, (v, n, uv, m) in enumerate(tris)]
    return mc.ElementSession(lib, mats, tris), mc.ElementSession(lib, mats, moved)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_radiance_gather_and_lightmap_after_a_move(gpu_lib, device):
    ses, fresh = room_pair(gpu_lib, (0.5, 0.3, -0.4))
    rng = np.random.RandomState(4)
    path_rays = mc.query_rays(2000, seed=12, extent=1.5)
    path_rays[:, 3] = 0.0; path_rays[:, 7] = np.arange(2000, dtype=np.uint32).view(F)
    pts = np.zeros((500, 8), F)
    pts[:, 0:3] = rng.uniform(-1.5, 1.5, (500, 3)); pts[:, 1] = -0.49; pts[:, 5] = 1.0; pts[:, 7] = np.arange(500, dtype=np.uint32).view(F)
    calls = [lambda s: binding.trace_radiance(gpu_lib, s.scene, path_rays, sample_count=2), lambda s: binding.gather(gpu_lib, s.scene, pts, binding.GATHER_IRRADIANCE, sample_count=4),
             lambda s: binding.gather(gpu_lib, s.scene, pts, binding.GATHER_SH9, sample_count=4)]
    bake = lambda s: binding.bake_lightmap(gpu_lib, s.scene, 16, 16, tri_first=4, tri_count=2, sample_count=4)
    before = [c(ses) for c in calls] + [bake(ses)[0]]
    assert mc.move_to(gpu_lib, ses, fresh, device) == (1, 4, 6)
    want = [c(fresh) for c in calls]
    got = [c(ses) for c in calls]
    for b, g, w in zip(before, got, want):
        assert mc.same_bits(g, w) and not mc.same_bits(b, w)
    (atlas, cov), (want_atlas, want_cov) = bake(ses), bake(fresh)
    assert cov.any() and np.array_equal(cov, want_cov) and mc.same_bits(atlas, want_atlas) and not mc.same_bits(before[-1], want_atlas)
    for host in (False, True):      # the raster on the device, and its host oracle on the host's copy of the moved triangles
        p, t, k = binding.lightmap_points(gpu_lib, ses.scene, 16, 16, tri_first=4, tri_count=2, host=host)
        wp, wt, wk = binding.lightmap_points(gpu_lib, fresh.scene, 16, 16, tri_first=4, tri_count=2, host=host)
        assert k == wk > 0 and np.array_equal(t, wt) and mc.same_bits(p, wp)
    ses.close(); fresh.close()


# ---- case 8: RaylibAMD_SceneRebuild after a move ----
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_rebuild_after_a_move(gpu_lib, workdir, soup, rays, device):
    ses = mc.soup_session(gpu_lib, workdir, "rebuild_a_%d" % device, soup)
    fresh = mc.soup_session(gpu_lib, workdir, "rebuild_b_%d" % device, rigid(soup, 200, 400))
    want, want_q = render_on(gpu_lib, fresh), queries_on(gpu_lib, fresh, rays)
    ok, nodes, depth, fresh_sah = mc.bvh_info(gpu_lib, fresh.scene)
    assert ok == 1
    h0, t0 = gpu_lib.RaylibAMD_SceneBVHHash(ses.scene), gpu_lib.RaylibAMD_SceneTopologyHash(ses.scene)
    render_on(gpu_lib, ses)
    assert mc.move_to(gpu_lib, ses, fresh, device)[0] == 1
    ok, n1, d1, refit_sah = mc.bvh_info(gpu_lib, ses.scene)       # (the validity check runs on the refitted host copy and the moved triangles)
    assert ok == 1 and np.isfinite(refit_sah) and refit_sah >= fresh_sah, (refit_sah, fresh_sah)
    moved_hash = gpu_lib.RaylibAMD_SceneBVHHash(ses.scene)
    assert moved_hash not in (h0, gpu_lib.RaylibAMD_SceneBVHHash(fresh.scene))      # the hash covers the boxes: the old topology around the moved triangles
    assert gpu_lib.RaylibAMD_SceneTopologyHash(ses.scene) == t0                      # ... which the topology hash says
    assert mc.same_bits(render_on(gpu_lib, ses), want)
    assert gpu_lib.RaylibAMD_SceneRebuild(ses.scene) == 1
    assert gpu_lib.RaylibAMD_SceneBVHHash(ses.scene) == gpu_lib.RaylibAMD_SceneBVHHash(fresh.scene)
    assert gpu_lib.RaylibAMD_SceneTopologyHash(ses.scene) == gpu_lib.RaylibAMD_SceneTopologyHash(fresh.scene) != t0
    ok, n2, d2, sah = mc.bvh_info(gpu_lib, ses.scene)
    assert ok == 1 and (n2, d2) == (nodes, depth) and F(sah).tobytes() == F(fresh_sah).tobytes()
    assert mc.same_bits(render_on(gpu_lib, ses), want) and queries_on(gpu_lib, ses, rays) == want_q
    assert_trees(gpu_lib, ses, refitted=False)
    ses.close(); fresh.close()


# ---- case 9: a move and a query on one stream of the caller's, nothing of the caller's between them (the query call itself waits for the move on the host:
# include/raylib_amd.h) ----
@pytest.mark.parametrize("structure", ["binary", "grid4", "wide8"])
def test_move_then_trace_on_one_stream(gpu_lib, workdir, monkeypatch, soup, rays, structure):
    use_structure(monkeypatch, structure)
    ses = mc.soup_session(gpu_lib, workdir, "stream_a_" + structure, soup)
    fresh = mc.soup_session(gpu_lib, workdir, "stream_b_" + structure, rigid(soup, 200, 400))
    want = binding.trace_rays(gpu_lib, fresh.scene, rays, binding.QUERY_CLOSEST)
    old = binding.trace_rays(gpu_lib, ses.scene, rays, binding.QUERY_CLOSEST)
    assert ses.stats().treeWidth == STRUCTURES[structure][3] and old.tobytes() != want.tobytes()
    b = mc.export(fresh)
    host_p, host_n = torch.from_numpy(mc.pos9(b[200:400])).pin_memory(), torch.from_numpy(mc.nrm9(b[200:400])).pin_memory()
    d_rays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        # the values reach the device on the stream too: the move must take them from there, behind the copies
        p, n = host_p.to("cuda", non_blocking=True), host_n.to("cuda", non_blocking=True)
        assert binding.move_triangles(gpu_lib, ses.scene, 200, p, n) == 1
        got = binding.trace_rays(gpu_lib, ses.scene, d_rays, binding.QUERY_CLOSEST)
    stream.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert mc.export(ses).tobytes() == b.tobytes()            # the host's copy, read back
    assert_trees(gpu_lib, ses)
    ses.close(); fresh.close()
