"""The VALUES of refitted boxes, and random sequences of moves, rebuilds, reads and queries against a model (RaylibAMD_SceneMoveTriangles, csrc/rl_refit.hip).

tests/test_gpu_move.py holds a moved scene to a fresh scene's results, and a closest hit does not depend on how tight a box is: a refit that never shrinks a
box, or puts a grid plane one step too far out, returns every bit of every result.  Here the boxes themselves are compared:
  * the binary tree, bit for bit, with move_cases.refit_boxes -- csrc/rl_k_refit.inl k_refit_level restated in NumPy, which tests/test_move_host.py holds to the
    builder's own boxes without a device;
  * the 4-wide float and grid records, the leaf list and the 8-wide records the device holds, byte for byte, with the host's statement of csrc/rl_grid.h applied
    to the device's binary boxes (RaylibAMD_SceneCompareTrees): the double-precision grid rule compiled for the device is the host's.
And the state a move leaves behind -- records and five tree formats rewritten in place, trees uploaded lazily, three staleness flags, the count of divisors
outside [2^-62, 2^125] -- is walked along random paths: move_cases.Sequence draws 12 ops per seed (moves through the host entry, the device entry and a
caller's stream, of five shapes, with and without normals; refused moves; reads of the host's copies; switches of structure, so that a wide tree is first
uploaded after some moves; rebuilds; progressive sessions; shutter changes beside a moving cube), applies each to a NumPy model and to the scene, checks the
trees behind every op and, behind every third, every result against a fresh scene made from the model.  A move marked quiet has nothing of the test's behind it
-- no check, no read-back -- before the next op runs: a move on a caller's stream always, a third of the others.

Every comparison is on bits.  Exact-t ties: a moved scene keeps its slots and the slot decides a tie (statement M2), so multi-hit primitives are compared
only on rays whose row of the fresh scene's host oracle holds no two equal t, and at most 1 % of a check's rays may be left out so.  The generator makes no two
coplanar overlapping triangles; run dry (move_cases.replay(seed, klass=1, dry=True): the model and RaylibAMD_TraceRaysAllHost alone, no device) over the seeds
below, the largest share of tied rays at any check was 0 of 512."""
import numpy as np
import pytest
import torch    # before the library is loaded

import move_cases as mc
import nearest_cases
from raylib_amd import binding
from test_gpu_move import STRUCTURES, assert_trees, queries_on, render_on, use_structure

pytestmark = pytest.mark.gpu
F = np.float32


# ---- B: random sequences ----
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6, 7, 8])
def test_random_sequence_soup(gpu_lib, workdir, monkeypatch, seed):
    seq = mc.Sequence(gpu_lib, workdir, seed, 1, lambda name: use_structure(monkeypatch, name), STRUCTURES)
    try:
        seq.run()
    finally:
        seq.close()
    print("largest share of rays left out of the primitive comparison: %.4f" % seq.max_tied)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_sequence_beside_spheres_and_a_moving_cube(gpu_lib, workdir, monkeypatch, seed):
    seq = mc.Sequence(gpu_lib, workdir, seed, 2, lambda name: use_structure(monkeypatch, name), STRUCTURES)
    try:
        seq.run()
    finally:
        seq.close()


# ---- what every fixed test below compares with a fresh scene: the frame, the three query families, the export ----
def nearest_on(lib, ses, points):
    return [binding.nearest_points(lib, ses.scene, p, kind).tobytes() for kind, p in ((binding.NEAREST_CLOSEST, points), (binding.NEAREST_WITHIN, nearest_cases.with_max_dist(points, 0.05)))]


def multihit_on(lib, ses, rays, host=False):
    out = []
    for k in (1, 4, binding.MAX_HITS):
        for count in (False, True):
            got = binding.trace_rays_all(lib, ses.scene, rays, k, count=count, host=host)
            out += [a.tobytes() for a in (got if count else (got,))]
    return out


def assert_same_as_fresh(lib, ses, fresh, rays, points, what):
    assert mc.same_triangles(mc.export(ses), mc.export(fresh)), what
    assert mc.same_bits(ses.render(mc.FW, mc.FH, mc.FSPP, mc.MAX_PATH), fresh.render(mc.FW, mc.FH, mc.FSPP, mc.MAX_PATH)), what
    assert queries_on(lib, ses, rays) == queries_on(lib, fresh, rays), what
    assert nearest_on(lib, ses, points) == nearest_on(lib, fresh, points), what
    assert not mc.tied_rays(binding.trace_rays_all(lib, fresh.scene, rays, binding.MAX_HITS, host=True)).any(), what      # (no exact-t tie on these rays: the primitives compare too)
    assert multihit_on(lib, ses, rays) == multihit_on(lib, fresh, rays, host=True), what


@pytest.fixture(scope="module")
def soup():
    return mc.soup_triangles(300, seed=21)


@pytest.fixture(scope="module")
def rays():
    return mc.query_rays(mc.N_RAYS, seed=31)


def points_of(ses, seed=41):
    return nearest_cases.point_set(np.random.RandomState(seed), mc.export(ses), mc.N_RAYS)


# ---- two sequences written out ----
def test_rebuild_straight_behind_a_move_on_a_stream(gpu_lib, workdir, monkeypatch, soup, rays):
    """(a) A device move on a caller's stream, RaylibAMD_SceneRebuild as the very next call -- the host's triangles and trees are stale, the move may still be in
    flight --, then the frame and the three query families against the fresh scene, whose trees the rebuilt ones now are."""
    use_structure(monkeypatch, "wide8")
    moved = soup.copy(); moved[100:200] = moved[100:200] @ mc.ROTATIONS[0].T + np.array([0.4, -0.3, 0.5])
    moved = moved.astype(F).astype(np.float64)
    ses, fresh = mc.soup_session(gpu_lib, workdir, "fix_a_a", soup), mc.soup_session(gpu_lib, workdir, "fix_a_b", moved)
    render_on(gpu_lib, ses)
    b = mc.export(fresh)
    host_p, host_n = torch.from_numpy(mc.pos9(b[100:200])).pin_memory(), torch.from_numpy(mc.nrm9(b[100:200])).pin_memory()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        p, n = host_p.to("cuda", non_blocking=True), host_n.to("cuda", non_blocking=True)
        assert binding.move_triangles(gpu_lib, ses.scene, 100, p, n) == 1
    assert gpu_lib.RaylibAMD_SceneRebuild(ses.scene) == 1
    assert gpu_lib.RaylibAMD_SceneBVHHash(ses.scene) == gpu_lib.RaylibAMD_SceneBVHHash(fresh.scene)
    assert gpu_lib.RaylibAMD_SceneTopologyHash(ses.scene) == gpu_lib.RaylibAMD_SceneTopologyHash(fresh.scene)
    assert_same_as_fresh(gpu_lib, ses, fresh, rays, points_of(fresh), "behind the rebuild")
    assert_trees(gpu_lib, ses, refitted=False)
    stream.synchronize()
    ses.close(); fresh.close()


def test_a_second_stale_period_ends_in_a_first_upload(gpu_lib, workdir, monkeypatch, soup, rays):
    """(b) A move under the binary tree's switches, a read of RaylibAMD_SceneBVHHash (the host's copies are brought up to date), a second move (stale again), then
    the first use of the 8-wide tree and of the 4-wide grid: both are uploaded from the host's copy, which must have been refitted a second time."""
    use_structure(monkeypatch, "binary")
    once = soup.copy(); once[50:150] = once[50:150] @ mc.ROTATIONS[1].T + np.array([-0.3, 0.2, 0.1])
    once = once.astype(F).astype(np.float64)
    twice = once.copy(); twice[120:260] = twice[120:260] @ mc.ROTATIONS[2].T + np.array([0.2, 0.4, -0.3])
    twice = twice.astype(F).astype(np.float64)
    ses = mc.soup_session(gpu_lib, workdir, "fix_b_a", soup)
    first, second = mc.soup_session(gpu_lib, workdir, "fix_b_b", once), mc.soup_session(gpu_lib, workdir, "fix_b_c", twice)
    render_on(gpu_lib, ses, "binary")
    h0 = gpu_lib.RaylibAMD_SceneBVHHash(ses.scene)
    assert mc.move_to(gpu_lib, ses, first, True)[0] == 1
    h1 = gpu_lib.RaylibAMD_SceneBVHHash(ses.scene)
    assert h1 not in (0, h0)
    assert mc.move_to(gpu_lib, ses, second, True)[0] == 1
    points = points_of(second)
    for structure in ("wide8", "grid4"):
        use_structure(monkeypatch, structure)
        assert mc.same_bits(render_on(gpu_lib, ses, structure), render_on(gpu_lib, second, structure)), structure
        assert queries_on(gpu_lib, ses, rays, structure) == queries_on(gpu_lib, second, rays, structure), structure
        assert_same_as_fresh(gpu_lib, ses, second, rays, points, structure)
        assert_trees(gpu_lib, ses)
    assert gpu_lib.RaylibAMD_SceneBVHHash(ses.scene) not in (0, h0, h1)
    for s in (ses, first, second):
        s.close()


# ---- A3: the grid rule's edges on the device ----
def scaled(tris, lo, hi, factor, about):
    out = np.array(tris, np.float64, copy=True)
    out[lo:hi] = about + (out[lo:hi] - about) * factor
    return out.astype(F).astype(np.float64)


@pytest.mark.parametrize("structure", ["grid4", "wide8"])
def test_grid_rule_edges_on_the_device(gpu_lib, workdir, monkeypatch, soup, rays, structure):
    """Moves that drive csrc/rl_grid.h to its edges, each followed by the value checks and a fresh scene's results: (i) a 100-triangle range scaled by 2^-40 about
    its centroid (steps far below the scene's: the exponent search runs down), then by 2^40 about the origin (coordinates near 2^40 beside coordinates near 1), then
    back; (ii) a range flattened into the plane x = 0 -- an axis of zero extent, on which GridAxisOf takes its smallest step, and zeros of both signs in the boxes
    --; (iii) one triangle at coordinates of magnitude 2^100: its record's products overflow, as they do on the host, and the exponent search runs to its upper clamp."""
    use_structure(monkeypatch, structure)
    centroid = soup[100:200].reshape(-1, 3).mean(0)
    tiny = scaled(soup, 100, 200, 2.0 ** -40, centroid)
    flat = soup.copy(); flat[30:90, :, 0] *= 0.0       # (-0.0 where x was negative)
    far = soup.copy(); far[7] = np.array([[1.0, 0.5, -0.75], [-0.5, 1.0, 0.25], [0.25, -1.0, 1.0]]) * 2.0 ** 100
    steps = [("(i) by 2^-40 about the centroid", tiny), ("(i) by 2^40 about the origin", scaled(soup, 100, 200, 2.0 ** 40, np.zeros(3))), ("(i) back", soup),
             ("(ii) flattened into x = 0", flat), ("(ii) back", soup), ("(iii) one triangle at 2^100", far), ("(iii) back", soup)]
    ses = mc.soup_session(gpu_lib, workdir, "grid_a_" + structure, soup)
    render_on(gpu_lib, ses)
    queries_on(gpu_lib, ses, rays, structure)         # the structure's trees are on the device before anything moves
    mc.assert_wide_trees_exact(gpu_lib, ses.scene)    # ... where they are the builder's, which quantises with the same rule from the same boxes
    mc.assert_refit_exact(gpu_lib, ses, bits=False)
    for i, (what, tris) in enumerate(steps):
        fresh = mc.soup_session(gpu_lib, workdir, "grid_b%d_%s" % (i, structure), tris)
        assert mc.move_to(gpu_lib, ses, fresh, device=bool(i % 2))[0] == 1, what
        assert mc.compare_trees(gpu_lib, ses.scene) == (1, 0), (what, mc.compare_trees(gpu_lib, ses.scene))
        assert mc.check_trees(gpu_lib, ses.scene) == (1, 0), what
        mc.assert_refit_exact(gpu_lib, ses)
        points = points_of(fresh, seed=50 + i)
        assert binding.trace_rays(gpu_lib, ses.scene, rays, binding.QUERY_CLOSEST).tobytes() == binding.trace_rays(gpu_lib, fresh.scene, rays, binding.QUERY_CLOSEST).tobytes(), what
        rc, plan = binding.plan_ray_query(gpu_lib, ses.scene, binding.QUERY_CLOSEST)
        assert rc == 1 and plan["treeWidth"] == STRUCTURES[structure][3], (what, plan)
        assert binding.nearest_points(gpu_lib, ses.scene, points, binding.NEAREST_CLOSEST).tobytes() == binding.nearest_points(gpu_lib, fresh.scene, points, binding.NEAREST_CLOSEST).tobytes(), what
        got, want = (binding.trace_rays_all(gpu_lib, s.scene, rays, 4, count=True) for s in (ses, fresh))
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), what
        assert mc.same_triangles(mc.export(ses), mc.export(fresh)), what
        fresh.close()
    ses.close()
