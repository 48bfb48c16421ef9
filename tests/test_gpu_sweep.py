"""Swept-sphere queries on the device (RaylibAMD_SweepSpheres / RaylibAMD_SweepSpheresDevice, csrc/rl_k_sweep.inl): the result equals the host oracle
RaylibAMD_SweepSpheresHost -- a loop over every triangle, itself held to a NumPy restatement and to float64 geometry by tests/test_sweep_host.py -- BYTE FOR
BYTE, with no tolerance, for both kinds, on every tree a scene carries, for the special values, for every count around the chunk and wave edges, on torch
tensors and streams, after the scene's triangles have moved and its trees were refitted or rebuilt, at the stacks' capacity edges, and behind a multi-rank
frame in flight."""
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
import stack_edges as se
import sweep_cases as sc
from raylib_amd import binding

pytestmark = pytest.mark.gpu

KINDS = (sc.ANY, sc.CLOSEST)
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 513)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


@pytest.fixture(scope="module")
def sscenes(gpu_lib, workdir, mid_scene):
    d = os.path.join(str(workdir), "sweep_gpu"); os.makedirs(d, exist_ok=True)
    own = {"cornell": sc.session(gpu_lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
           "soup": sc.session(gpu_lib, scenes.soup(os.path.join(d, "soup.obj"), 10000)[0]),
           "doubled": sc.session(gpu_lib, sc.write_soup(os.path.join(d, "doubled.obj"), 500, seed=5, doubled=True))}
    out = dict(own); out["room"] = mid_scene[0]
    yield out
    for s in own.values():
        s.close()


def _oracle(lib, ses, q, kind):
    return binding.sweep_spheres(lib, ses.scene, q, kind, host=True)


def _device(lib, ses, q, kind):
    return binding.sweep_spheres(lib, ses.scene, q, kind)


def _force(lib, monkeypatch, ses, tree):
    """RAYLIB_QUERY_TREE=tree (read per call); returns the width of the tree the planner then walks."""
    monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))
    rc, p = binding.plan_sweep(lib, ses.scene, sc.CLOSEST)
    assert rc == 1
    return p["treeWidth"]


def _queries_of(ses, seed, n=2000):
    return sc.query_set(np.random.RandomState(seed), ses.export_flat()[0], n)


def _assert_same(got, want, q, what):
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint32).reshape(len(q), -1) != want.view(np.uint32).reshape(len(q), -1)).any(1))[0]
        raise AssertionError("%s: %d queries differ, first %r got %r want %r" % (what, len(bad), q[bad[0]], got[bad[0]], want[bad[0]]))


@pytest.mark.parametrize("name", ["cornell", "soup", "room", "doubled"])
def test_device_is_the_oracle_on_every_tree(gpu_lib, sscenes, monkeypatch, name):
    ses = sscenes[name]
    q = _queries_of(ses, 41)
    want = {k: _oracle(gpu_lib, ses, q, k) for k in KINDS}
    # the query set must cut (checked in the oracle, on the CPU)
    hit = want[sc.CLOSEST]["prim"] >= 0
    assert 0.2 < hit.mean() < 0.9 and np.array_equal(want[sc.ANY] == 1, hit), "between 20 %% and 90 %% of the queries must hit: %.2f" % hit.mean()
    seen = np.bincount(want[sc.CLOSEST]["feature"][hit], minlength=8)
    assert (seen > 0).all() and len(seen) == 8, "every feature 0..7 must occur: %r" % seen
    tris, _ = ses.export_flat()
    some = np.nonzero(hit)[0][:96]
    ties = sc.ties_near(q[some], tris)
    assert (ties >= 2).any(), "at least one tie on T must be decided by the index"
    if name == "doubled":
        key = [t.tobytes() for t in np.stack([tris["v0"], tris["v1"], tris["v2"]], 1)]
        first = {}
        for k, b in enumerate(key):
            first.setdefault(b, k)
        assert all(first[key[p]] == p for p in want[sc.CLOSEST]["prim"][hit]), "every winner of a tie is the lower export index"
    widths = set()
    for tree in (2, 4):
        width = _force(gpu_lib, monkeypatch, ses, tree)
        widths.add(width)
        for k in KINDS:
            _assert_same(_device(gpu_lib, ses, q, k), want[k], q, "%s, tree %d, kind %d" % (name, tree, k))
        st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
        assert st.rays == len(q) and st.treeWidth == width and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0, st.as_dict()
    assert widths == {2, 4}, "the scene carries both trees"


@pytest.mark.parametrize("tree", [2, 4])
def test_special_values(gpu_lib, sscenes, monkeypatch, tree):
    for name in ("cornell", "soup"):
        ses = sscenes[name]
        tris, _ = ses.export_flat()
        q, what = sc.special_queries(tris)
        q = np.concatenate([q, sc.ending_at_contact(gpu_lib, ses, tris)])
        assert len(q) > len(what)
        _force(gpu_lib, monkeypatch, ses, tree)
        want = _oracle(gpu_lib, ses, q, sc.CLOSEST)
        got = _device(gpu_lib, ses, q, sc.CLOSEST)
        assert got.tobytes() == want.tobytes(), [(w, g, x) for w, g, x in zip(what + ["ends at contact"] * len(q), got, want) if g.tobytes() != x.tobytes()]
        assert np.array_equal(_device(gpu_lib, ses, q, sc.ANY), _oracle(gpu_lib, ses, q, sc.ANY))
        row = {w: got[i] for i, w in enumerate(what)}
        assert row["NaN origin"]["prim"] == -1 and row["negative radius"]["prim"] == -1 and row["1e30 away"]["prim"] == -1
        assert row["origin exactly on a vertex"]["feature"] == 7 and row["origin exactly on a vertex"]["t"] == 0
        assert (got["t"][len(what):] == 1.0).all() and (got["prim"][len(what):] >= 0).all(), "a move that ends exactly at first contact hits"


@pytest.mark.parametrize("n", COUNTS)
def test_counts_across_chunk_and_wave_edges(gpu_lib, sscenes, n):
    ses = sscenes["soup"]
    q = _queries_of(ses, 43, n=600)[:n]
    for k in KINDS:
        assert _device(gpu_lib, ses, q, k).tobytes() == _oracle(gpu_lib, ses, q, k).tobytes(), (n, k)
    # the device entry writes n records and nothing behind them
    dev = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    out = torch.full((n + 4, 8), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert gpu_lib.RaylibAMD_SweepSpheresDevice(ses.scene, sc.CLOSEST, C.c_void_p(dev.data_ptr()), n, C.c_void_p(out.data_ptr()), None) == 1
    o = out.cpu().numpy()
    assert o[:n].tobytes() == _oracle(gpu_lib, ses, q, sc.CLOSEST).tobytes() and (o[n:] == 0x5a5a5a5a).all()


def test_device_entry_on_torch_tensors(gpu_lib, sscenes):
    ses = sscenes["soup"]
    q = np.ascontiguousarray(_queries_of(ses, 47))
    n = len(q)
    want = {k: _oracle(gpu_lib, ses, q, k) for k in KINDS}
    # on a stream of the caller's, enqueued behind a kernel that writes the queries
    src = torch.from_numpy(q).cuda()
    dev = torch.zeros_like(src)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.add(src, 0.0, out=dev)
        outs = {k: binding.sweep_spheres(gpu_lib, ses.scene, dev, k) for k in KINDS}
    s.synchronize()
    assert outs[sc.CLOSEST].cpu().numpy().tobytes() == want[sc.CLOSEST].tobytes()
    assert np.array_equal(outs[sc.ANY].cpu().numpy().view(np.uint32), want[sc.ANY])
    # torch's default stream: synchronous, with stats
    outs = {k: binding.sweep_spheres(gpu_lib, ses.scene, dev, k) for k in KINDS}
    assert outs[sc.CLOSEST].cpu().numpy().tobytes() == want[sc.CLOSEST].tobytes()
    assert np.array_equal(outs[sc.ANY].cpu().numpy().view(np.uint32), want[sc.ANY])
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    out = torch.full((n + 4, 8), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert gpu_lib.RaylibAMD_SweepSpheresDevice(ses.scene, sc.CLOSEST, ptr(dev), n, ptr(out), None) == 1
    o = out.cpu().numpy()
    assert o[:n].tobytes() == want[sc.CLOSEST].tobytes() and (o[n:] == 0x5a5a5a5a).all(), "the canaries behind the output stay"
    st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.rays == n and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    words = torch.full((n + 4,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert gpu_lib.RaylibAMD_SweepSpheresDevice(ses.scene, sc.ANY, ptr(dev), n, ptr(words), None) == 1
    w = words.cpu().numpy()
    assert np.array_equal(w[:n].view(np.uint32), want[sc.ANY]) and (w[n:] == 0x5a5a5a5a).all()
    # refusals leave `out` untouched: a host pointer, queries off 16-byte alignment by 4 bytes, outputs off theirs
    out = torch.full((n + 1, 8), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    big = torch.zeros(n * 8 + 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    f = gpu_lib.RaylibAMD_SweepSpheresDevice
    assert f(ses.scene, sc.CLOSEST, q.ctypes.data, n, ptr(out), None) == 0
    assert f(ses.scene, sc.CLOSEST, ptr(big, 4), n, ptr(out), None) == 0
    assert f(ses.scene, sc.CLOSEST, ptr(dev), n, ptr(out, 4), None) == 0       # RaylibAMDSweepHit records need 16 bytes
    assert f(ses.scene, sc.ANY, ptr(dev), n, ptr(out, 2), None) == 0           # words need 4
    host_out = np.zeros(n, binding.SWEEP_HIT_DTYPE)
    assert f(ses.scene, sc.CLOSEST, ptr(dev), n, host_out.ctypes.data, None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5a5a5a5a).all()
    assert f(ses.scene, sc.ANY, ptr(dev), n, ptr(out, 4), None) == 1           # ... and 4 is enough for ANY
    assert gpu_lib.RaylibAMD_SweepSpheres(ses.scene, sc.CLOSEST, None, 0, None) == 1


@pytest.mark.parametrize("device", [False, True], ids=["host-entry", "device-entry"])
def test_after_a_move_and_after_a_rebuild(gpu_lib, workdir, mid_scene, monkeypatch, device):
    """The room with the triangles of a fifth of its vertices displaced: the moved scene's query is the oracle's on the moved triangles and, byte for byte, the
    query on a scene built fresh from them -- on the refitted trees, and again on the trees RaylibAMD_SceneRebuild makes."""
    obj = mid_scene[1]
    with open(obj) as f:
        nv = sum(1 for line in f if line.startswith("v "))
    shift = np.random.RandomState(7).uniform(-0.05, 0.05, (nv, 3)).astype(np.float32)
    moved_obj = mc.edit_obj(obj, os.path.join(os.path.dirname(obj), "mid_sweep_moved.obj"), move_v=lambda k, p: p + shift[k] if k < nv // 5 else p)
    ses, fresh = sc.session(gpu_lib, obj), sc.session(gpu_lib, moved_obj)
    try:
        q = _queries_of(fresh, 53, n=800)
        before = {k: _device(gpu_lib, ses, q, k) for k in KINDS}      # (the scene is on the device, both trees: the move refits them there)
        _force(gpu_lib, monkeypatch, ses, 2)
        _device(gpu_lib, ses, q[:64], sc.CLOSEST)
        monkeypatch.delenv("RAYLIB_QUERY_TREE")
        ok, first, end = mc.move_to(gpu_lib, ses, fresh, device=device)
        assert ok == 1 and end - first > len(ses.export_flat()[0]) // 8
        want = {k: _oracle(gpu_lib, fresh, q, k) for k in KINDS}
        assert want[sc.CLOSEST].tobytes() != before[sc.CLOSEST].tobytes(), "the move must change answers"
        for stage in ("refitted", "rebuilt"):
            if stage == "rebuilt":
                assert gpu_lib.RaylibAMD_SceneRebuild(ses.scene) == 1
            own = {k: _oracle(gpu_lib, ses, q, k) for k in KINDS}   # (the oracle walks no tree: once per stage)
            for tree in (2, 4):
                _force(gpu_lib, monkeypatch, ses, tree); _force(gpu_lib, monkeypatch, fresh, tree)
                for k in KINDS:
                    got = _device(gpu_lib, ses, q, k)
                    assert got.tobytes() == own[k].tobytes(), (stage, tree, k, "the oracle reads the moved triangles")
                    assert got.tobytes() == want[k].tobytes(), (stage, tree, k, "the fresh scene's oracle")
                    assert got.tobytes() == _device(gpu_lib, fresh, q, k).tobytes(), (stage, tree, k, "the fresh scene's query")
    finally:
        ses.close(); fresh.close()


# the stacks' capacity edges (tests/stack_edges.py): (scene, RAYLIB_QUERY_TREE, the tree and the stack the planner must pick)
EDGES = [("cone_d32", 2, 2, 32), ("cone_d33", 2, 2, 64), ("cone_d32", 4, 4, 32), ("cone_d33", 4, 4, 64), ("cone_n64", 4, 4, 64), ("cone_n65", 4, 2, 32),
         ("chain_l16", 2, 2, 32), ("chain_l17", 2, 2, 64)]


def _edge_queries(spec):
    """Moves on and around the axis: there every level's boxes contain the path from its start (they all contain the axis), so their time bounds are all 0,
    nothing is culled before the first leaf and the far child is pushed at every level; then moves around every level's triangle, and from far outside."""
    rng = np.random.RandomState(3)
    if spec["kind"] == "cone":
        scales = np.asarray(se.cone_scales(spec["n"], spec["ratio"], spec["pace"], spec["size"]))
        z = np.concatenate([[0.0], scales, 0.5 * scales, 1.5 * scales, -scales, [4.0 * scales[0]]])
        axis = np.stack([np.zeros_like(z), np.zeros_like(z), z], 1)
        ring = np.concatenate([axis[1:1 + len(scales)] + scales[:, None] * np.asarray([f, g, 0.0]) for f, g in ((0.3, 0.0), (0.0, -0.4), (-0.9, 0.7), (1e-3, 1e-3))])
        org = np.concatenate([axis, ring, axis + rng.uniform(-1, 1, axis.shape) * 1e-3 * scales[-1]])
        size = np.concatenate([np.abs(z) + scales[-1], np.tile(scales, 4), np.abs(z) + scales[-1]])
    else:
        c = 2.0 ** -np.arange(1, spec["n_chain"] + 1)
        org = np.concatenate([np.zeros((1, 3)), np.stack([c, np.zeros_like(c), np.zeros_like(c)], 1), np.stack([c, c / 4, c / 8], 1), np.stack([-c, c, c], 1),
                              rng.uniform(-2, 2, (200, 3))])
        size = np.concatenate([[1.0], c, c, c, np.ones(200)])
    n = len(org)
    q = np.zeros((n, 8), np.float32)
    q[:, 0:3] = org
    q[:, 3] = size * np.where(np.arange(n) % 3 == 0, 0.0, rng.uniform(1e-3, 0.3, n))
    away = rng.normal(size=(n, 3)) * size[:, None]
    q[:, 4:7] = np.where((np.arange(n) % 4 == 0)[:, None], -org, np.where((np.arange(n) % 4 == 1)[:, None], org * 0.5, away))   # to the apex, outwards, anywhere
    return q


@pytest.mark.parametrize("name,env,width,stack", EDGES, ids=["%s-tree%d" % (e[0], e[1]) for e in EDGES])
def test_stack_capacity_edges(gpu_lib, workdir, monkeypatch, name, env, width, stack):
    spec = se.SCENES[name]
    ses, _ = se.make_session(gpu_lib, spec, os.path.join(str(workdir), "sweep_edges"), name)
    try:
        tn = se.tree_numbers(gpu_lib, ses.scene)
        assert (tn["depth"], tn["need4"]) == (spec["depth"], spec["need4"]), tn
        monkeypatch.setenv("RAYLIB_QUERY_TREE", str(env))
        rc, p = binding.plan_sweep(gpu_lib, ses.scene, sc.CLOSEST)
        assert rc == 1 and (p["treeWidth"], p["stack"]) == (width, stack), p
        q = _edge_queries(spec)
        for k in KINDS:
            got, want = _device(gpu_lib, ses, q, k), _oracle(gpu_lib, ses, q, k)
            assert got.tobytes() == want.tobytes(), (name, env, k, "a dropped push shows as a difference from the oracle")
        hit = want["prim"] >= 0
        assert 0.1 < hit.mean() < 1.0, hit.mean()
        st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
        assert st.rays == len(q) and st.nodesVisited > len(q) * spec["depth"] // 8, st.as_dict()
    finally:
        ses.close()


def test_behind_a_multi_rank_frame_in_flight(gpu_lib, workdir):
    """tests/sweep_rank_child.py under three ranks on one device: Raylib_Render, then at once the sweep (host entry and device entry).  The sweep equals the
    oracle, and the frame equals the one-rank frame of this process."""
    import sweep_rank_child as child
    out = os.path.join(str(workdir), "sweep_rank.npz")
    env = dict(os.environ)
    for k in ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_QUERY_TREE"):
        env.pop(k, None)
    env.update(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0")
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(workdir), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    one = child.run(gpu_lib, workdir)
    assert int(got["ranks"]) == 3 and int(one["ranks"]) == 1
    for key in ("closest_host_entry", "closest_device_entry", "any_host_entry"):
        assert got[key].tobytes() == got[key.split("_")[0] + "_oracle"].tobytes(), key
        assert got[key].tobytes() == np.asarray(one[key]).view(got[key].dtype).tobytes(), key
    prim = got["closest_oracle"].view(binding.SWEEP_HIT_DTYPE)["prim"]
    assert (prim >= 0).any() and (prim < 0).any()
    assert bool(helpers.same(got["frame"], one["frame"]).all()), "the frame in flight behind the sweep is not the one-rank frame"
