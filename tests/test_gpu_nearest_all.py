"""The K nearest triangles and the count in range on the device (RaylibAMD_NearestPointsAll / RaylibAMD_NearestPointsAllDevice, csrc/rl_k_nearest_all.inl): rows
and counts equal the host oracle RaylibAMD_NearestPointsAllHost -- a loop over every triangle, itself held to a NumPy restatement by
tests/test_nearest_all_host.py -- BYTE FOR BYTE, with no tolerance, on every tree a scene carries, with and without the count, for every point count around the
chunk and wave edges, after the scene's triangles have moved and its trees were refitted or rebuilt, at the stacks' capacity edges, and behind a multi-rank
frame in flight.  The point sets take their radii from the oracle's own rows, so that rows are empty, part full, exactly full and overfull."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch    # before the library is loaded: the device entry is handed torch's tensors

import helpers
import move_cases as mc
import nearest_cases as nc
import nearest_all_cases as na
import stack_edges as se
from raylib_amd import binding

pytestmark = pytest.mark.gpu

MAX_HITS = (1, 3, 16)
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 513)
POISON = 0x5a5a5a5a


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


@pytest.fixture(scope="module")
def S(gpu_lib, workdir):
    out = na.make_sessions(gpu_lib, os.path.join(str(workdir), "nearest_all_gpu"))
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def base(S):
    """per scene: 520 points with maxDist +inf and the oracle's rows of 16 for them (computed once)"""
    return {name: na.base_points(S[name], 41 + k, 520) for k, name in enumerate(na.SCENES)}


def _device(lib, ses, pts, max_hits, count):
    """(rows, counts or None) through the host-memory entry"""
    r = binding.nearest_points_all(lib, ses.scene, pts, max_hits, count=count)
    return r if count else (r, None)


def _force(lib, monkeypatch, ses, tree):
    """RAYLIB_QUERY_TREE=tree (read per call); returns the width of the tree the planner then walks."""
    monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))
    rc, p = binding.plan_nearest_all(lib, ses.scene, 4)
    assert rc == 1
    return p["treeWidth"]


def _stats(lib):
    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
    return st


def _check(lib, ses, pts, max_hits, count, want, what):
    rows, counts = _device(lib, ses, pts, max_hits, count)
    na.same_rows(rows, want[0], what)
    if count:
        assert np.array_equal(counts, want[1]), (what, "counts differ at", np.nonzero(counts != want[1])[0][:8])


@pytest.mark.parametrize("name", na.SCENES)
def test_device_is_the_oracle_on_every_tree(gpu_lib, S, base, monkeypatch, name):
    ses = S[name]
    widths = set()
    for max_hits in MAX_HITS:
        pts = na.calibrated(base[name], max_hits)
        want = na.oracle(gpu_lib, ses, pts, max_hits)
        na.check_classes(want[1], max_hits, na.TWINS[name])
        for tree in (2, 4):
            width = _force(gpu_lib, monkeypatch, ses, tree)
            widths.add(width)
            for count in (False, True):
                _check(gpu_lib, ses, pts, max_hits, count, want, "%s, tree %d, maxHits %d, count %r" % (name, tree, max_hits, count))
                st = _stats(gpu_lib)
                assert st.rays == len(pts) and st.treeWidth == width and st.nodesVisited > 0 and st.kernelMs > 0, st.as_dict()
    assert widths == {2, 4}, "the scene carries both trees"


@pytest.mark.parametrize("n", COUNTS)
def test_counts_across_chunk_and_wave_edges(gpu_lib, S, base, n):
    ses, K = S["soup"], 3
    pts = np.ascontiguousarray(na.calibrated(base["soup"], K)[:n])
    want = na.oracle(gpu_lib, ses, pts, K)
    _check(gpu_lib, ses, pts, K, True, want, "n %d" % n)
    _check(gpu_lib, ses, pts, K, False, want, "n %d, no count" % n)
    # the device entry writes n * maxHits records and n counts, and nothing behind them
    dev = torch.from_numpy(pts).cuda()
    rows = torch.full((n * K + 4, 4), POISON, dtype=torch.int32, device="cuda")
    counts = torch.full((n + 4,), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert gpu_lib.RaylibAMD_NearestPointsAllDevice(ses.scene, C.c_void_p(dev.data_ptr()), n, K, C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()), None) == 1
    r, c = rows.cpu().numpy(), counts.cpu().numpy()
    assert r[:n * K].tobytes() == want[0].tobytes() and (r[n * K:] == POISON).all()
    assert np.array_equal(c[:n].view(np.uint32), want[1]) and (c[n:] == POISON).all()


@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_max_hits_1_without_the_count_is_closest_and_walks_the_same_records(gpu_lib, S, base, monkeypatch, name):
    """The walk and the bound are CLOSEST's, and a point's node and triangle records do not depend on the wave it rides in: the sums are equal exactly."""
    ses = S[name]
    pts = na.calibrated(base[name], 1)
    for tree in (2, 4):
        _force(gpu_lib, monkeypatch, ses, tree)
        closest = binding.nearest_points(gpu_lib, ses.scene, pts, nc.CLOSEST)
        a = _stats(gpu_lib)
        rows, _ = _device(gpu_lib, ses, pts, 1, False)
        b = _stats(gpu_lib)
        assert rows.tobytes() == closest.tobytes(), (name, tree)
        assert (b.rays, b.nodesVisited, b.trisTested) == (a.rays, a.nodesVisited, a.trisTested) and a.nodesVisited > 0 and a.trisTested > 0, (name, tree, a.as_dict(), b.as_dict())


def test_the_list_bound_prunes(gpu_lib, S, base, monkeypatch):
    """maxDist +inf on the 2000-triangle soup: with the count every node is in range; without it the walk culls with the list's last D."""
    ses, pts = S["soup"], base["soup"][0]
    for tree in (2, 4):
        _force(gpu_lib, monkeypatch, ses, tree)
        for max_hits in (1, 4, 16):
            want = na.oracle(gpu_lib, ses, pts, max_hits)
            assert (want[1] == 2000).all()
            _check(gpu_lib, ses, pts, max_hits, True, want, "with the count")
            full = _stats(gpu_lib)
            _check(gpu_lib, ses, pts, max_hits, False, want, "without the count")
            pruned = _stats(gpu_lib)
            assert full.trisTested == 2000 * len(pts), "the count visits every triangle"
            assert pruned.nodesVisited < full.nodesVisited and pruned.trisTested < full.trisTested, (tree, max_hits, pruned.as_dict(), full.as_dict())


def test_device_entry_on_torch_tensors(gpu_lib, S, base):
    ses, K = S["soup"], 5
    pts = np.ascontiguousarray(na.calibrated(base["soup"], K))
    n = len(pts)
    want = na.oracle(gpu_lib, ses, pts, K)
    # on a stream of the caller's, enqueued behind a kernel that writes the points
    src = torch.from_numpy(pts).cuda()
    dev = torch.zeros_like(src)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.add(src, 0.0, out=dev)
        rows, counts = binding.nearest_points_all(gpu_lib, ses.scene, dev, K, count=True)
        rows_only = binding.nearest_points_all(gpu_lib, ses.scene, dev, K)
    s.synchronize()
    assert rows.cpu().numpy().tobytes() == want[0].tobytes() and rows_only.cpu().numpy().tobytes() == want[0].tobytes()
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want[1])
    # the null stream: synchronous, with stats
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    f = gpu_lib.RaylibAMD_NearestPointsAllDevice
    out = torch.empty((n * K, 4), dtype=torch.int32, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert f(ses.scene, ptr(dev), n, K, ptr(out), ptr(cnt), None) == 1
    assert out.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(cnt.cpu().numpy().view(np.uint32), want[1])
    st = _stats(gpu_lib)
    assert st.rays == n and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    # refusals leave the outputs untouched: a host pointer, points off 16-byte alignment by 4 bytes, outputs off theirs
    out = torch.full((n * K + 1, 4), POISON, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + 1,), POISON, dtype=torch.int32, device="cuda")
    big = torch.zeros(n * 4 + 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert f(ses.scene, pts.ctypes.data, n, K, ptr(out), ptr(cnt), None) == 0
    assert f(ses.scene, ptr(big, 4), n, K, ptr(out), ptr(cnt), None) == 0
    assert f(ses.scene, ptr(dev), n, K, ptr(out, 4), ptr(cnt), None) == 0       # RaylibAMDNearestHit records need 16 bytes
    assert f(ses.scene, ptr(dev), n, K, ptr(out), ptr(cnt, 2), None) == 0       # counts need 4
    host_rows, host_cnt = np.zeros((n, K), binding.NEAREST_DTYPE), np.zeros(n, np.uint32)
    assert f(ses.scene, ptr(dev), n, K, host_rows.ctypes.data, ptr(cnt), None) == 0
    assert f(ses.scene, ptr(dev), n, K, ptr(out), host_cnt.ctypes.data, None) == 0
    assert f(ses.scene, ptr(dev), n, binding.MAX_NEAREST + 1, ptr(out), ptr(cnt), None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all() and (cnt.cpu().numpy() == POISON).all()
    assert f(ses.scene, ptr(dev), n, K, ptr(out), ptr(cnt, 4), None) == 1       # ... and 4 is enough for the counts
    assert gpu_lib.RaylibAMD_NearestPointsAll(ses.scene, None, 0, K, None, None) == 1


@pytest.mark.parametrize("device", [False, True], ids=["host-entry", "device-entry"])
def test_after_a_move_and_after_a_rebuild(gpu_lib, workdir, monkeypatch, device):
    """The 2000-triangle soup with a fifth of its vertices displaced by at most 0.05: the moved scene's query is the oracle's on the moved triangles and, byte for
    byte, the query on a scene built fresh from them -- on the refitted trees, and again on the trees RaylibAMD_SceneRebuild makes (K2: the order inside a tie
    follows the export index, so a rebuild changes nothing)."""
    d = os.path.join(str(workdir), "nearest_all_move_%d" % device); os.makedirs(d, exist_ok=True)
    obj = nc.write_soup(os.path.join(d, "soup.obj"), 2000)
    nv = 3 * 2000
    rng = np.random.RandomState(7)
    shift = rng.uniform(-0.05, 0.05, (nv, 3)).astype(np.float32)
    moved = rng.permutation(nv) < nv // 5
    moved_obj = mc.edit_obj(obj, os.path.join(d, "soup_moved.obj"), move_v=lambda k, p: p + shift[k] if moved[k] else p)
    ses, fresh = nc.session(gpu_lib, obj), nc.session(gpu_lib, moved_obj)
    K = 4
    try:
        pts = na.calibrated(na.base_points(fresh, 53, 400), K)
        want = na.oracle(gpu_lib, fresh, pts, K)
        na.check_classes(want[1], K)
        before = {}
        for tree in (2, 4):   # (the scene is on the device, both trees: the move refits them there)
            _force(gpu_lib, monkeypatch, ses, tree)
            before[tree] = _device(gpu_lib, ses, pts, K, True)
        monkeypatch.delenv("RAYLIB_QUERY_TREE")
        ok, first, end = mc.move_to(gpu_lib, ses, fresh, device=device)
        assert ok == 1 and end - first > 2000 // 8
        assert want[0].tobytes() != before[2][0].tobytes() and not np.array_equal(want[1], before[2][1]), "the move must change answers"
        for stage in ("refitted", "rebuilt"):
            if stage == "rebuilt":
                assert gpu_lib.RaylibAMD_SceneRebuild(ses.scene) == 1
            assert na.oracle(gpu_lib, ses, pts, K)[0].tobytes() == want[0].tobytes(), (stage, "the oracle reads the moved triangles")
            for tree in (2, 4):
                _force(gpu_lib, monkeypatch, ses, tree); _force(gpu_lib, monkeypatch, fresh, tree)
                for count in (False, True):
                    what = "%s, tree %d, count %r" % (stage, tree, count)
                    _check(gpu_lib, ses, pts, K, count, want, what)
                    _check(gpu_lib, fresh, pts, K, count, want, what + ": the fresh scene's query")
                assert _device(gpu_lib, ses, pts, K, False)[0].tobytes() != before[tree][0].tobytes()
    finally:
        ses.close(); fresh.close()


# the stacks' capacity edges (tests/stack_edges.py), as tests/test_gpu_nearest.py lists them: (scene, RAYLIB_QUERY_TREE, the tree and the stack the planner must pick)
EDGES = [("cone_d32", 2, 2, 32), ("cone_d33", 2, 2, 64), ("cone_d32", 4, 4, 32), ("cone_d33", 4, 4, 64), ("cone_n64", 4, 4, 64), ("cone_n65", 4, 2, 32),
         ("chain_l16", 2, 2, 32), ("chain_l17", 2, 2, 64)]


def _edge_points(spec):
    """On and around the axis: there every level's boxes are equally far (they all contain the axis), nothing is culled before the first leaf, and the far child is
    pushed at every level; then around every level's triangle, and from far outside."""
    rng = np.random.RandomState(3)
    if spec["kind"] == "cone":
        sc = np.asarray(se.cone_scales(spec["n"], spec["ratio"], spec["pace"], spec["size"]))
        z = np.concatenate([[0.0], sc, 0.5 * sc, 1.5 * sc, -sc, [4.0 * sc[0]]])
        axis = np.stack([np.zeros_like(z), np.zeros_like(z), z], 1)
        ring = np.concatenate([axis[1:1 + len(sc)] + sc[:, None] * np.asarray([f, g, 0.0]) for f, g in ((0.3, 0.0), (0.0, -0.4), (-0.9, 0.7), (1e-3, 1e-3))])
        pts = np.concatenate([axis, ring, axis + rng.uniform(-1, 1, axis.shape) * 1e-3 * sc[-1]])
    else:
        c = 2.0 ** -np.arange(1, spec["n_chain"] + 1)
        pts = np.concatenate([np.zeros((1, 3)), np.stack([c, np.zeros_like(c), np.zeros_like(c)], 1), np.stack([c, c / 4, c / 8], 1), np.stack([-c, c, c], 1),
                              rng.uniform(-2, 2, (200, 3))])
    return np.concatenate([pts, np.full((len(pts), 1), np.inf)], 1).astype(np.float32)


@pytest.mark.parametrize("name,env,width,stack", EDGES, ids=["%s-tree%d" % (e[0], e[1]) for e in EDGES])
def test_stack_capacity_edges(gpu_lib, workdir, monkeypatch, name, env, width, stack):
    """maxHits 4 with the count and maxDist +inf: nothing is culled, every far child is pushed.  The 64-deep instances carry 96 KB of stack beside the list."""
    spec = se.SCENES[name]
    ses, _ = se.make_session(gpu_lib, spec, os.path.join(str(workdir), "nearest_all_edges"), name)
    try:
        tn = se.tree_numbers(gpu_lib, ses.scene)
        assert (tn["depth"], tn["need4"]) == (spec["depth"], spec["need4"]), tn
        monkeypatch.setenv("RAYLIB_QUERY_TREE", str(env))
        rc, p = binding.plan_nearest_all(gpu_lib, ses.scene, 4, True)
        assert rc == 1 and (p["treeWidth"], p["stack"]) == (width, stack), p
        pts = _edge_points(spec)
        want = na.oracle(gpu_lib, ses, pts, 4)
        assert (want[1] == len(ses.export_flat()[0])).all() and (want[0]["prim"] >= 0).all(), "maxDist +inf: every triangle is in range"
        _check(gpu_lib, ses, pts, 4, True, want, "%s, tree %d: a dropped push shows as a difference from the oracle" % (name, env))
    finally:
        ses.close()


def test_behind_a_multi_rank_frame_in_flight(gpu_lib, workdir):
    """tests/nearest_all_rank_child.py under three ranks on one device: Raylib_Render, then at once the query (host entry and device entry).  The query equals
    the oracle, and the frame equals the one-rank frame of this process."""
    import nearest_all_rank_child as child
    out = os.path.join(str(workdir), "nearest_all_rank.npz")
    env = dict(os.environ)
    for k in ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_QUERY_TREE"):
        env.pop(k, None)
    env.update(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0")
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(workdir), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    one = child.run(gpu_lib, workdir)
    assert int(got["ranks"]) == 3 and int(one["ranks"]) == 1
    for key in ("rows_host_entry", "rows_device_entry", "rows_uncounted"):
        assert got[key].tobytes() == got["rows_oracle"].tobytes(), key
        assert got[key].tobytes() == np.asarray(one[key]).view(np.uint32).tobytes(), key
    for key in ("counts_host_entry", "counts_device_entry"):
        assert np.array_equal(got[key], got["counts_oracle"]) and np.array_equal(got[key], one[key]), key
    assert (got["counts_oracle"] > 0).any() and (got["counts_oracle"] == 0).any()
    assert bool(helpers.same(got["frame"], one["frame"]).all()), "the frame in flight behind the query is not the one-rank frame"
