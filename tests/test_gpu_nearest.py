"""Nearest-point queries on the device (RaylibAMD_NearestPoints / RaylibAMD_NearestPointsDevice, csrc/rl_k_nearest.inl): the result equals the host oracle
RaylibAMD_NearestPointsHost -- a loop over every triangle, itself held to a NumPy restatement by tests/test_nearest_host.py -- BYTE FOR BYTE, with no
tolerance, for both kinds, on every tree a scene carries, for every count around the chunk and wave edges, after the scene's triangles have moved and its
trees were refitted or rebuilt, at the stacks' capacity edges, and behind a multi-rank frame in flight."""
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
import nearest_cases as nc
import stack_edges as se
from raylib_amd import binding

pytestmark = pytest.mark.gpu

TREE_BVH2, TREE_GRID4 = 1, 3
KINDS = (nc.WITHIN, nc.CLOSEST)
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 513)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


@pytest.fixture(scope="module")
def nscenes(gpu_lib, workdir, mid_scene):
    d = os.path.join(str(workdir), "nearest_gpu"); os.makedirs(d, exist_ok=True)
    own = {"cornell": nc.session(gpu_lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
           "soup": nc.session(gpu_lib, scenes.soup(os.path.join(d, "soup.obj"), 10000)[0]),
           "doubled": nc.session(gpu_lib, nc.write_soup(os.path.join(d, "doubled.obj"), 500, seed=5, doubled=True))}
    out = dict(own); out["room"] = mid_scene[0]
    yield out
    for s in own.values():
        s.close()


def _oracle(lib, ses, pts, kind):
    return binding.nearest_points(lib, ses.scene, pts, kind, host=True)


def _device(lib, ses, pts, kind):
    return binding.nearest_points(lib, ses.scene, pts, kind)


def _force(lib, monkeypatch, ses, tree):
    """RAYLIB_QUERY_TREE=tree (read per call); returns the width of the tree the planner then walks."""
    monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))
    rc, p = binding.plan_nearest(lib, ses.scene, nc.CLOSEST)
    assert rc == 1
    return p["treeWidth"]


def _points_of(ses, seed, n=1200):
    """About 2000 points: random in 1.5 x the bounds, on surfaces, at vertices and on edges, 1e-4 off surfaces (maxDist +inf); far outside (1e6); and 600 of the
    first with maxDist 0, a quantile of the true distances, just below and just above the point's own sqrt(D), +inf."""
    tris, _ = ses.export_flat()
    rng = np.random.RandomState(seed)
    base = nc.point_set(rng, tris, n)
    far = np.concatenate([rng.choice([-1e6, 1e6], (40, 3)) + rng.uniform(-1, 1, (40, 3)), np.full((40, 1), np.inf)], 1).astype(np.float32)
    own = np.sqrt(_oracle(ses.lib, ses, base, nc.CLOSEST)["dist2"].astype(np.float64))
    pick = rng.permutation(len(base))[:600]
    q = float(np.quantile(own[own > 0], 0.4)) if (own > 0).any() else 0.0
    md = np.select([np.arange(600) % 5 == k for k in range(5)], [np.zeros(600), np.full(600, q), own[pick] * (1 - 1e-6), own[pick] * (1 + 1e-6), np.full(600, np.inf)])
    return np.concatenate([base, far, nc.with_max_dist(base[pick], md.astype(np.float32))])


@pytest.mark.parametrize("name", ["cornell", "soup", "room", "doubled"])
def test_device_is_the_oracle_on_every_tree(gpu_lib, nscenes, monkeypatch, name):
    ses = nscenes[name]
    pts = _points_of(ses, 41)
    want = {k: _oracle(gpu_lib, ses, pts, k) for k in KINDS}
    hits = (want[nc.CLOSEST]["prim"] >= 0)
    assert 0.5 < hits.mean() < 1.0 and np.array_equal(want[nc.WITHIN] == 1, hits), "the radii must cut: some points find a triangle, some do not"
    if name == "doubled":
        tris, _ = ses.export_flat()
        key = [t.tobytes() for t in np.stack([tris["v0"], tris["v1"], tris["v2"]], 1)]
        first = {}
        for k, b in enumerate(key):
            first.setdefault(b, k)
        assert all(first[key[p]] == p for p in want[nc.CLOSEST]["prim"][hits]), "every winner of a tie is the lower export index"
    widths = set()
    for tree in (2, 4):
        width = _force(gpu_lib, monkeypatch, ses, tree)
        widths.add(width)
        for k in KINDS:
            got = _device(gpu_lib, ses, pts, k)
            bad = np.nonzero(got.view(np.uint32).reshape(len(pts), -1) != want[k].view(np.uint32).reshape(len(pts), -1))[0]
            assert got.tobytes() == want[k].tobytes(), "%s, tree %d, kind %d: %d points differ, first %r got %r want %r" % (
                name, tree, k, len(set(bad)), pts[bad[0]], got[bad[0]], want[k][bad[0]])
        st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
        assert st.rays == len(pts) and st.treeWidth == width and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0, st.as_dict()
    assert widths == {2, 4}, "the scene carries both trees"


@pytest.mark.parametrize("tree", [2, 4])
def test_special_values(gpu_lib, nscenes, monkeypatch, tree):
    for name in ("cornell", "soup"):
        ses = nscenes[name]
        tris, _ = ses.export_flat()
        pts, what = nc.special_points(tris)
        _force(gpu_lib, monkeypatch, ses, tree)
        want = _oracle(gpu_lib, ses, pts, nc.CLOSEST)
        got = _device(gpu_lib, ses, pts, nc.CLOSEST)
        assert got.tobytes() == want.tobytes(), [(w, g, x) for w, g, x in zip(what, got, want) if g.tobytes() != x.tobytes()]
        assert np.array_equal(_device(gpu_lib, ses, pts, nc.WITHIN), _oracle(gpu_lib, ses, pts, nc.WITHIN))
        row = {w: got[i] for i, w in enumerate(what)}
        assert row["NaN x"]["prim"] == -1 and row["maxDist NaN"]["prim"] == -1 and row["maxDist -1"]["prim"] == -1
        assert row["maxDist -0.0 at a v0 vertex"]["prim"] >= 0 and row["maxDist -0.0 at a v0 vertex"]["dist2"] == 0.0
        assert row["1e25 away, maxDist +inf"]["prim"] == 0 and row["1e25 away, maxDist +inf"]["dist2"] == np.inf


@pytest.mark.parametrize("n", COUNTS)
def test_counts_across_chunk_and_wave_edges(gpu_lib, nscenes, n):
    ses = nscenes["soup"]
    pts = _points_of(ses, 43, n=600)[:n]
    for k in KINDS:
        out = _device(gpu_lib, ses, pts, k)
        assert out.tobytes() == _oracle(gpu_lib, ses, pts, k).tobytes(), (n, k)
    # the device entry writes n records and nothing behind them
    dev = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    out = torch.full((n + 4, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert gpu_lib.RaylibAMD_NearestPointsDevice(ses.scene, nc.CLOSEST, C.c_void_p(dev.data_ptr()), n, C.c_void_p(out.data_ptr()), None) == 1
    o = out.cpu().numpy()
    assert o[:n].tobytes() == _oracle(gpu_lib, ses, pts, nc.CLOSEST).tobytes() and (o[n:] == 0x5a5a5a5a).all()


def test_device_entry_on_torch_tensors(gpu_lib, nscenes):
    ses = nscenes["soup"]
    pts = np.ascontiguousarray(_points_of(ses, 47))
    n = len(pts)
    want = {k: _oracle(gpu_lib, ses, pts, k) for k in KINDS}
    # on a stream of the caller's, enqueued behind a kernel that writes the points
    src = torch.from_numpy(pts).cuda()
    dev = torch.zeros_like(src)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.add(src, 0.0, out=dev)
        outs = {k: binding.nearest_points(gpu_lib, ses.scene, dev, k) for k in KINDS}
    s.synchronize()
    assert outs[nc.CLOSEST].cpu().numpy().tobytes() == want[nc.CLOSEST].tobytes()
    assert np.array_equal(outs[nc.WITHIN].cpu().numpy().view(np.uint32), want[nc.WITHIN])
    # the null stream: synchronous, with stats
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert gpu_lib.RaylibAMD_NearestPointsDevice(ses.scene, nc.CLOSEST, ptr(dev), n, ptr(out), None) == 1
    assert out.cpu().numpy().tobytes() == want[nc.CLOSEST].tobytes()
    st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.rays == n and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    # refusals leave `out` untouched: a host pointer, points off 16-byte alignment by 4 bytes, outputs off theirs
    out = torch.full((n + 1, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    big = torch.zeros(n * 4 + 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    f = gpu_lib.RaylibAMD_NearestPointsDevice
    assert f(ses.scene, nc.CLOSEST, pts.ctypes.data, n, ptr(out), None) == 0
    assert f(ses.scene, nc.CLOSEST, ptr(big, 4), n, ptr(out), None) == 0
    assert f(ses.scene, nc.CLOSEST, ptr(dev), n, ptr(out, 4), None) == 0       # RaylibAMDNearestHit records need 16 bytes
    assert f(ses.scene, nc.WITHIN, ptr(dev), n, ptr(out, 2), None) == 0        # words need 4
    host_out = np.zeros(n, binding.NEAREST_DTYPE)
    assert f(ses.scene, nc.CLOSEST, ptr(dev), n, host_out.ctypes.data, None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5a5a5a5a).all()
    assert f(ses.scene, nc.WITHIN, ptr(dev), n, ptr(out, 4), None) == 1        # ... and 4 is enough for WITHIN
    assert gpu_lib.RaylibAMD_NearestPoints(ses.scene, nc.CLOSEST, None, 0, None) == 1


@pytest.mark.parametrize("device", [False, True], ids=["host-entry", "device-entry"])
def test_after_a_move_and_after_a_rebuild(gpu_lib, workdir, mid_scene, monkeypatch, device):
    """The room with the triangles of a fifth of its vertices displaced: the moved scene's query is the oracle's on the moved triangles and, byte for byte, the
    query on a scene built fresh from them -- on the refitted trees, and again on the trees RaylibAMD_SceneRebuild makes."""
    obj = mid_scene[1]
    d = os.path.join(str(workdir), "nearest_move"); os.makedirs(d, exist_ok=True)
    with open(obj) as f:
        nv = sum(1 for line in f if line.startswith("v "))
    shift = np.random.RandomState(7).uniform(-0.05, 0.05, (nv, 3)).astype(np.float32)
    moved_obj = mc.edit_obj(obj, os.path.join(os.path.dirname(obj), "mid_nearest_moved.obj"), move_v=lambda k, p: p + shift[k] if k < nv // 5 else p)
    ses, fresh = nc.session(gpu_lib, obj), nc.session(gpu_lib, moved_obj)
    try:
        pts = _points_of(fresh, 53)
        before = {k: _device(gpu_lib, ses, pts, k) for k in KINDS}      # (the scene is on the device, both trees: the move refits them there)
        _force(gpu_lib, monkeypatch, ses, 2)
        _device(gpu_lib, ses, pts[:64], nc.CLOSEST)
        monkeypatch.delenv("RAYLIB_QUERY_TREE")
        ok, first, end = mc.move_to(gpu_lib, ses, fresh, device=device)
        assert ok == 1 and end - first > len(ses.export_flat()[0]) // 8
        want = {k: _oracle(gpu_lib, fresh, pts, k) for k in KINDS}
        assert want[nc.CLOSEST].tobytes() != before[nc.CLOSEST].tobytes(), "the move must change answers"
        for stage in ("refitted", "rebuilt"):
            if stage == "rebuilt":
                assert gpu_lib.RaylibAMD_SceneRebuild(ses.scene) == 1
            for tree in (2, 4):
                _force(gpu_lib, monkeypatch, ses, tree); _force(gpu_lib, monkeypatch, fresh, tree)
                for k in KINDS:
                    got = _device(gpu_lib, ses, pts, k)
                    assert got.tobytes() == _oracle(gpu_lib, ses, pts, k).tobytes(), (stage, tree, k, "the oracle reads the moved triangles")
                    assert got.tobytes() == want[k].tobytes(), (stage, tree, k, "the fresh scene's oracle")
                    assert got.tobytes() == _device(gpu_lib, fresh, pts, k).tobytes(), (stage, tree, k, "the fresh scene's query")
    finally:
        ses.close(); fresh.close()


# the stacks' capacity edges (tests/stack_edges.py): (scene, RAYLIB_QUERY_TREE, the tree and the stack the planner must pick)
EDGES = [("cone_d32", 2, 2, 32), ("cone_d33", 2, 2, 64), ("cone_d32", 4, 4, 32), ("cone_d33", 4, 4, 64), ("cone_n64", 4, 4, 64), ("cone_n65", 4, 2, 32),
         ("chain_l16", 2, 2, 32), ("chain_l17", 2, 2, 64)]


def _edge_points(spec, tris):
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
    spec = se.SCENES[name]
    ses, _ = se.make_session(gpu_lib, spec, os.path.join(str(workdir), "nearest_edges"), name)
    try:
        tn = se.tree_numbers(gpu_lib, ses.scene)
        assert (tn["depth"], tn["need4"]) == (spec["depth"], spec["need4"]), tn
        monkeypatch.setenv("RAYLIB_QUERY_TREE", str(env))
        rc, p = binding.plan_nearest(gpu_lib, ses.scene, nc.CLOSEST)
        assert rc == 1 and (p["treeWidth"], p["stack"]) == (width, stack), p
        pts = _edge_points(spec, ses.export_flat()[0])
        for k in KINDS:
            got, want = _device(gpu_lib, ses, pts, k), _oracle(gpu_lib, ses, pts, k)
            assert got.tobytes() == want.tobytes(), (name, env, k, "a dropped push shows as a difference from the oracle")
            assert (want == 1).all() if k == nc.WITHIN else (want["prim"] >= 0).all(), "maxDist +inf: every point finds a triangle"
    finally:
        ses.close()


def test_behind_a_multi_rank_frame_in_flight(gpu_lib, workdir):
    """tests/nearest_rank_child.py under three ranks on one device: Raylib_Render, then at once the nearest query (host entry and device entry).  The query
    equals the oracle, and the frame equals the one-rank frame of this process."""
    import nearest_rank_child as child
    out = os.path.join(str(workdir), "nearest_rank.npz")
    env = dict(os.environ)
    for k in ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_QUERY_TREE"):
        env.pop(k, None)
    env.update(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0")
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(workdir), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    one = child.run(gpu_lib, workdir)
    assert int(got["ranks"]) == 3 and int(one["ranks"]) == 1
    for key in ("closest_host_entry", "closest_device_entry", "within_host_entry"):
        assert got[key].tobytes() == got[key.split("_")[0] + "_oracle"].tobytes(), key
        assert got[key].tobytes() == one[key].tobytes(), key
    assert (got["closest_oracle"].view(binding.NEAREST_DTYPE)["prim"] >= 0).any()
    assert bool(helpers.same(got["frame"], one["frame"]).all()), "the frame in flight behind the query is not the one-rank frame"
