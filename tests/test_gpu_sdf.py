"""Signed distance fields baked on the device (RaylibAMD_BakeDistanceField / RaylibAMD_BakeDistanceFieldDevice, csrc/rl_k_sdf.inl): the result equals the host
oracle RaylibAMD_BakeDistanceFieldHost -- a loop over every triangle, itself pinned by tests/test_sdf_host.py -- BYTE FOR BYTE, with no tolerance: in every
sign mode, with and without outPrim, on every tree either walk can take, on grids whose rows spill into a second word and whose bricks are partial, for
bands that cut nothing, something and everything, on a caller's stream, back to back on the library's bit volumes, after the scene's triangles have moved
and its trees were refitted or rebuilt, at the capacity edges of the distance kernel's stacks, and behind a multi-rank frame in flight."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch    # before the library is loaded: the device entry is handed torch's tensors

import helpers
from helpers import scenes
import move_cases as mc
import sdf_cases as sc
import stack_edges as se
from raylib_amd import binding

pytestmark = pytest.mark.gpu

INF = float("inf")
# 33 on each axis in turn: bit 33 of a row (n_a + 1 = 34 bits) lies in a second word, 65 reaches a third; partial 4 x 4 x 4 bricks on every axis
GRIDS = [(20, 17, 9), (33, 5, 3), (3, 33, 2), (2, 3, 33), (65, 4, 4), (1, 1, 1)]
TREES = (2, 4, 8)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


@pytest.fixture(scope="module")
def S(gpu_lib, workdir):
    d = os.path.join(str(workdir), "sdf_gpu")
    out = sc.make_sessions(gpu_lib, d)
    out["soup"] = sc.session(gpu_lib, scenes.soup(os.path.join(d, "soup.obj"), 10000)[0])
    yield out
    for s in out.values():
        s.close()


def _oracle(lib, ses, grid, max_dist, sign):
    origin, spacing, dims = grid
    return sc.bake(lib, ses, origin, spacing, dims, max_dist, sign, prim=True, host=True)


def _device(lib, ses, grid, max_dist, sign, prim=True, **kw):
    origin, spacing, dims = grid
    return sc.bake(lib, ses, origin, spacing, dims, max_dist, sign, prim=prim, **kw)


def _grid(dims, lo=-1.6, hi=1.6):
    origin, spacing = sc.grid_around(dims, lo=lo, hi=hi, shift=sc.IRRATIONAL)
    return origin, spacing, dims


def _force(lib, monkeypatch, ses, grid, tree):
    """RAYLIB_QUERY_TREE=tree (read per call); returns the widths of the trees the distance kernel and the row kernel then walk."""
    monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))
    rc, near, rows = binding.plan_distance_field(lib, ses.scene, grid[0], grid[1], grid[2], INF, sc.MAJORITY)
    assert rc == 1
    return near["treeWidth"], rows["treeWidth"]


def _same(got, want, what):
    d, p = got
    wd, wp = want
    if d.tobytes() != wd.tobytes():
        bad = np.argwhere(d.view(np.uint32) != wd.view(np.uint32))
        raise AssertionError("%s: %d voxels' distances differ, first [k, j, i] = %s got %r want %r" % (what, len(bad), bad[0], d[tuple(bad[0])], wd[tuple(bad[0])]))
    assert p.tobytes() == wp.tobytes(), "%s: %d voxels' triangles differ" % (what, int((p != wp).sum()))


def _check_every_mode(lib, monkeypatch, ses, grids, what, max_dist=INF, lo=-1.6, hi=1.6):
    near_widths, row_widths = set(), set()
    for dims in grids:
        grid = _grid(dims, lo, hi)
        want = {sign: _oracle(lib, ses, grid, max_dist, sign) for sign in sc.SIGNS}
        for tree in TREES:
            nw, rw = _force(lib, monkeypatch, ses, grid, tree)
            near_widths.add(nw); row_widths.add(rw)
            for sign in sc.SIGNS:
                _same(_device(lib, ses, grid, max_dist, sign), want[sign], "%s %r tree %d sign %d" % (what, dims, tree, sign))
                assert _device(lib, ses, grid, max_dist, sign, prim=False).tobytes() == want[sign][0].tobytes(), (what, dims, tree, sign, "outPrim null")
    return near_widths, row_widths


@pytest.mark.parametrize("name", ["cube", "sphere", "torus", "doubled"])
def test_device_is_the_oracle_in_every_mode_on_every_tree(gpu_lib, S, monkeypatch, name):
    near_widths, row_widths = _check_every_mode(gpu_lib, monkeypatch, S[name], GRIDS, name)
    if name != "cube":   # (twelve triangles carry no wide tree)
        assert near_widths == {2, 4} and row_widths == {2, 8}, (near_widths, row_widths)
    grid = _grid(GRIDS[0])
    signed = _oracle(gpu_lib, S[name], grid, INF, sc.MAJORITY)[0]
    assert np.signbit(signed).any() != (name == "doubled"), "a closed mesh has an inside; the doubled one's parity is even everywhere"


def test_soup_is_open_and_still_the_oracle(gpu_lib, S, monkeypatch):
    """10 000 random triangles: the sign means nothing, the bytes are the statements' all the same."""
    near_widths, row_widths = _check_every_mode(gpu_lib, monkeypatch, S["soup"], GRIDS[:1], "soup", lo=-4.2, hi=4.2)
    assert near_widths == {2, 4} and row_widths == {2, 8}, (near_widths, row_widths)


def test_room_unsigned_in_a_band(gpu_lib, mid_scene, monkeypatch):
    ses = mid_scene[0]
    dims = (24, 20, 12)
    origin, spacing = sc.grid_around(dims, lo=-1.1, hi=2.1, shift=sc.IRRATIONAL)
    grid = (origin, spacing, dims)
    band = 3.0 * float(spacing.max())
    want = _oracle(gpu_lib, ses, grid, band, sc.UNSIGNED)
    missed = (want[1] < 0).mean()
    assert 0.05 < missed < 0.95, missed
    for tree in TREES:
        _force(gpu_lib, monkeypatch, ses, grid, tree)
        _same(_device(gpu_lib, ses, grid, band, sc.UNSIGNED), want, "room tree %d" % tree)


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_max_dist_values(gpu_lib, S, name):
    """0, one voxel, a band that cuts about half the voxels, +inf."""
    ses = S[name]
    grid = _grid(GRIDS[0])
    voxel = float(grid[1].max())
    full = _oracle(gpu_lib, ses, grid, INF, sc.UNSIGNED)[0]
    half = float(np.median(full))
    for max_dist in (0.0, voxel, half, INF):
        for sign in (sc.UNSIGNED, sc.SIGN_Y, sc.MAJORITY):
            want = _oracle(gpu_lib, ses, grid, max_dist, sign)
            if max_dist == half:
                missed = (want[1] < 0).mean()
                assert 0.1 <= missed <= 0.9, "the band must cut: %g of the voxels missed" % missed
            if max_dist == 0.0:
                assert (want[1] < 0).all() and (np.abs(want[0]) == 0).all()
            _same(_device(gpu_lib, ses, grid, max_dist, sign), want, "%s maxDist %g sign %d" % (name, max_dist, sign))


def test_device_entry_on_a_torch_stream(gpu_lib, S):
    ses = S["torus"]
    grid = _grid(GRIDS[0])
    n = int(np.prod(GRIDS[0]))
    s = torch.cuda.Stream()
    outs = {}
    with torch.cuda.stream(s):
        for sign in sc.SIGNS:
            outs[sign] = _device(gpu_lib, ses, grid, INF, sign, device=True)
    s.synchronize()
    for sign in sc.SIGNS:
        want = _oracle(gpu_lib, ses, grid, INF, sign)
        got = (outs[sign][0].cpu().numpy(), outs[sign][1].cpu().numpy())
        _same(got, want, "device entry, sign %d" % sign)
        _same(_device(gpu_lib, ses, grid, INF, sign), want, "plain entry, sign %d" % sign)
    # the null stream: synchronous, with stats; nothing is written behind the volume
    p = binding.distance_field_params(grid[0], grid[1], grid[2], INF, sc.MAJORITY)
    dist = torch.full((n + 4,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    prim = torch.full((n + 4,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    f = gpu_lib.RaylibAMD_BakeDistanceFieldDevice
    assert f(ses.scene, C.byref(p), ptr(dist), ptr(prim), None) == 1
    want = _oracle(gpu_lib, ses, grid, INF, sc.MAJORITY)
    d, q = dist.cpu().numpy(), prim.cpu().numpy()
    assert d[:n].tobytes() == want[0].tobytes() and q[:n].tobytes() == want[1].tobytes() and (d[n:] == 0x5a5a5a5a).all() and (q[n:] == 0x5a5a5a5a).all()
    # V7 on the device entry: a host pointer, an output off 4-byte alignment -- nothing written
    dist.fill_(0x5a5a5a5a); prim.fill_(0x5a5a5a5a)
    host = np.zeros(n, np.float32)
    torch.cuda.synchronize()
    assert f(ses.scene, C.byref(p), host.ctypes.data, None, None) == 0
    assert f(ses.scene, C.byref(p), ptr(dist), host.ctypes.data, None) == 0
    assert f(ses.scene, C.byref(p), ptr(dist, 2), None, None) == 0
    assert f(ses.scene, C.byref(p), ptr(dist), ptr(prim, 2), None) == 0
    torch.cuda.synchronize()
    assert (dist.cpu().numpy() == 0x5a5a5a5a).all() and (prim.cpu().numpy() == 0x5a5a5a5a).all() and not host.any()


def test_second_smaller_bake_sees_none_of_the_first_ones_bits(gpu_lib, S):
    ses = S["torus"]
    for first, second in (((33, 17, 9), (7, 5, 3)), ((20, 17, 9), (2, 3, 33))):
        big, small = _grid(first), _grid(second)
        _same(_device(gpu_lib, ses, big, INF, sc.MAJORITY), _oracle(gpu_lib, ses, big, INF, sc.MAJORITY), "the first bake")
        for sign in (sc.MAJORITY, sc.SIGN_Z, sc.SIGN_X):
            _same(_device(gpu_lib, ses, small, INF, sign), _oracle(gpu_lib, ses, small, INF, sign), "the second, smaller bake, sign %d" % sign)


@pytest.mark.parametrize("device", [False, True], ids=["host-entry", "device-entry"])
def test_after_a_move_and_after_a_rebuild(gpu_lib, workdir, monkeypatch, device):
    """The sphere translated by 0.37 voxel: the moved scene's bake is the oracle's on the moved triangles and, byte for byte, the bake of a scene built fresh
    from them -- on the refitted trees, and again on the trees RaylibAMD_SceneRebuild makes."""
    d = os.path.join(str(workdir), "sdf_move_%d" % device); os.makedirs(d, exist_ok=True)
    grid = _grid(GRIDS[0])
    shift = 0.37 * grid[1].astype(np.float64)
    obj = sc.write_mesh(os.path.join(d, "sphere.obj"), "sphere")
    moved = sc.write_mesh(os.path.join(d, "sphere_moved.obj"), "sphere", centre=tuple(shift))
    ses, fresh = sc.session(gpu_lib, obj), sc.session(gpu_lib, moved)
    try:
        before = {}
        for tree in TREES:   # (the scene is on the device with every tree: the move refits them there)
            _force(gpu_lib, monkeypatch, ses, grid, tree)
            before[tree] = _device(gpu_lib, ses, grid, INF, sc.MAJORITY)
        monkeypatch.delenv("RAYLIB_QUERY_TREE")
        ok, first, end = mc.move_to(gpu_lib, ses, fresh, device=device)
        assert ok == 1 and end - first == len(ses.export_flat()[0])
        want = {sign: _oracle(gpu_lib, fresh, grid, INF, sign) for sign in (sc.MAJORITY, sc.SIGN_X)}
        assert want[sc.MAJORITY][0].tobytes() != before[2][0].tobytes(), "the move must change answers"
        for stage in ("refitted", "rebuilt"):
            if stage == "rebuilt":
                assert gpu_lib.RaylibAMD_SceneRebuild(ses.scene) == 1
            for tree in TREES:
                _force(gpu_lib, monkeypatch, ses, grid, tree); _force(gpu_lib, monkeypatch, fresh, grid, tree)
                for sign in want:
                    got = _device(gpu_lib, ses, grid, INF, sign)
                    _same(got, _oracle(gpu_lib, ses, grid, INF, sign), "%s tree %d sign %d: the oracle reads the moved triangles" % (stage, tree, sign))
                    _same(got, want[sign], "%s tree %d sign %d: the fresh scene's oracle" % (stage, tree, sign))
                    _same(got, _device(gpu_lib, fresh, grid, INF, sign), "%s tree %d sign %d: the fresh scene's bake" % (stage, tree, sign))
    finally:
        ses.close(); fresh.close()


def test_stats(gpu_lib, S, monkeypatch):
    ses = S["torus"]
    nx, ny, nz = GRIDS[0]
    grid = _grid(GRIDS[0])
    rows = {sc.UNSIGNED: 0, sc.SIGN_X: ny * nz, sc.SIGN_Y: nx * nz, sc.SIGN_Z: nx * ny, sc.MAJORITY: ny * nz + nx * nz + nx * ny}
    for tree in (2, 8):
        near_width, _ = _force(gpu_lib, monkeypatch, ses, grid, tree)
        for sign in sc.SIGNS:
            _device(gpu_lib, ses, grid, INF, sign)
            st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
            assert st.rays == nx * ny * nz + rows[sign], (sign, st.as_dict())
            assert st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0 and st.wallMs >= st.kernelMs and st.treeWidth == near_width, st.as_dict()


# the stacks' capacity edges (tests/stack_edges.py): tests/test_gpu_nearest.py's EDGES that plan a walk for the distance kernel -- (scene, RAYLIB_QUERY_TREE, the
# tree and the stack the planner must pick for it)
EDGES = [("cone_d32", 2, 2, 32), ("cone_d33", 2, 2, 64), ("cone_d32", 4, 4, 32), ("cone_d33", 4, 4, 64), ("cone_n64", 4, 4, 64), ("chain_l16", 2, 2, 32),
         ("chain_l17", 2, 2, 64)]
EDGE_DIMS, EDGE_APEX = (5, 6, 7), (2, 2, 3)


def edge_grid(spec):
    """5 x 6 x 7 voxels (partial bricks on every axis) of a power-of-two spacing near the scene's smallest triangle, voxel EDGE_APEX's centre exactly at the origin
    -- the apex, where every level's boxes are equally far, nothing is culled before the first leaf and the far child is pushed at every level.  Every operand of
    V1 is a small multiple of the spacing: each step is exact."""
    if spec["kind"] == "cone":
        spacing = 2.0 ** round(float(np.log2(se.cone_scales(spec["n"], spec["ratio"], spec["pace"], spec["size"])[-1])))
    else:
        spacing = 2.0 ** -spec["n_chain"]
    origin = np.array([-(k + 0.5) * spacing for k in EDGE_APEX], np.float32)
    return origin, np.full(3, spacing, np.float32), EDGE_DIMS


@pytest.mark.parametrize("name,env,width,stack", EDGES, ids=["%s-tree%d" % (e[0], e[1]) for e in EDGES])
def test_stack_capacity_edges(gpu_lib, workdir, monkeypatch, name, env, width, stack):
    """The distance kernel with its stack exactly full, and one past on the next size: a dropped push shows as a difference from the oracle.  The same voxel centres
    sent as points are k_nearest's CLOSEST answers, and -- one walk on the same points, however the lanes are cut into bricks or chunks -- its node and
    triangle counts (an UNSIGNED bake launches the distance kernel alone: test_stats)."""
    spec = se.SCENES[name]
    ses, _ = se.make_session(gpu_lib, spec, os.path.join(str(workdir), "sdf_edges"), name)
    try:
        tn = se.tree_numbers(gpu_lib, ses.scene)
        assert (tn["depth"], tn["need4"]) == (spec["depth"], spec["need4"]), tn
        grid = edge_grid(spec)
        cen = sc.centres(*grid)
        k, j, i = EDGE_APEX[2], EDGE_APEX[1], EDGE_APEX[0]
        assert cen.shape == (7, 6, 5, 3) and not cen[k, j, i].any() and np.isfinite(cen).all(), cen[k, j, i]
        monkeypatch.setenv("RAYLIB_QUERY_TREE", str(env))
        rc, near, _ = binding.plan_distance_field(gpu_lib, ses.scene, grid[0], grid[1], grid[2], INF, sc.UNSIGNED)
        assert rc == 1 and (near["treeWidth"], near["stack"]) == (width, stack), near
        want = _oracle(gpu_lib, ses, grid, INF, sc.UNSIGNED)
        assert (want[1] >= 0).all(), "maxDist +inf: every voxel finds a triangle"
        _same(_device(gpu_lib, ses, grid, INF, sc.UNSIGNED), want, "%s tree %d" % (name, env))
        baked = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(baked))
        pts = np.concatenate([cen.reshape(-1, 3), np.full((cen.size // 3, 1), np.inf, np.float32)], 1).astype(np.float32)
        got = binding.nearest_points(gpu_lib, ses.scene, pts, binding.NEAREST_CLOSEST)
        asked = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(asked))
        assert got["prim"].tobytes() == want[1].tobytes(), "%d voxels' triangles are not the nearest query's" % int((got["prim"] != want[1].ravel()).sum())
        assert np.sqrt(got["dist2"]).tobytes() == want[0].tobytes(), "the magnitude is the exact root of the nearest query's dist2"
        assert baked.rays == asked.rays == len(pts) and baked.treeWidth == asked.treeWidth == width, (baked.as_dict(), asked.as_dict())
        assert (baked.nodesVisited, baked.trisTested) == (asked.nodesVisited, asked.trisTested) and baked.nodesVisited > 0, (baked.as_dict(), asked.as_dict())
    finally:
        ses.close()


def test_behind_a_multi_rank_frame_in_flight(gpu_lib, workdir):
    """tests/sdf_rank_child.py under three ranks on one device: Raylib_Render, then at once the bake (host entry and device entry).  The bake equals the
    oracle, and the frame equals the one-rank frame of this process."""
    import sdf_rank_child as child
    out = os.path.join(str(workdir), "sdf_rank.npz")
    env = dict(os.environ)
    for k in ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_QUERY_TREE"):
        env.pop(k, None)
    env.update(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0")
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(workdir), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    one = child.run(gpu_lib, workdir)
    assert int(got["ranks"]) == 3 and int(one["ranks"]) == 1
    for key in ("host_entry", "device_entry"):
        for part in ("_dist", "_prim"):
            assert got[key + part].tobytes() == got["oracle" + part].tobytes(), key + part
            assert got[key + part].tobytes() == one[key + part].tobytes(), key + part
    assert np.signbit(got["oracle_dist"]).any() and (got["oracle_prim"] >= 0).all()
    assert bool(helpers.same(got["frame"], one["frame"]).all()), "the frame in flight behind the bake is not the one-rank frame"
