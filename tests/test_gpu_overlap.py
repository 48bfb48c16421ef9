"""Triangle-overlap queries on the device (RaylibAMD_OverlapTriangles / RaylibAMD_OverlapTrianglesDevice, csrc/rl_k_overlap.inl): the result equals the host
oracle RaylibAMD_OverlapTrianglesHost -- a loop over every triangle, itself held to a NumPy restatement by tests/test_overlap_host.py -- BYTE FOR BYTE, with no
tolerance, for both kinds, with and without the shared-vertex flag, for maxHits 1, 4 and 16 with and without the count, on every tree a scene carries, for
every count around the chunk and wave edges, after the scene's triangles have moved and its trees were refitted or rebuilt, at the stacks' capacity edges, and
behind a multi-rank frame in flight."""
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
import overlap_cases as oc
import stack_edges as se
from raylib_amd import binding

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 513)
MAX_HITS = (1, 4, 16)
FLAGS = (0, oc.SKIP_SHARED)
CANARY = 0x5a5a5a5a


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


@pytest.fixture(scope="module")
def oscenes(gpu_lib, workdir, mid_scene):
    d = os.path.join(str(workdir), "overlap_gpu"); os.makedirs(d, exist_ok=True)
    own = {"cornell": oc.session(gpu_lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
           "soup": oc.session(gpu_lib, scenes.soup(os.path.join(d, "soup.obj"), 10000)[0]),
           "doubled": oc.session(gpu_lib, oc.write_soup(os.path.join(d, "doubled.obj"), 500, seed=5, doubled=True))}
    out = dict(own); out["room"] = mid_scene[0]
    yield out
    for s in own.values():
        s.close()


def _oracle(lib, ses, q, kind, flags=0, k=16):
    return binding.overlap_triangles(lib, ses.scene, q, kind, flags, k, host=True)


def _device(lib, ses, q, kind, flags=0, k=16, count=True):
    return binding.overlap_triangles(lib, ses.scene, q, kind, flags, k, count=count)


def _force(lib, monkeypatch, ses, tree):
    """RAYLIB_QUERY_TREE=tree (read per call); returns the width of the tree the planner then walks."""
    monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))
    rc, p = binding.plan_overlap(lib, ses.scene, oc.LIST)
    assert rc == 1
    return p["treeWidth"]


def _queries_of(ses, seed, n=2000):
    """About n queries: the scene's own triangles, those jittered, random triangles from 0.01 to 2 times the extent, the specials."""
    return oc.query_set(np.random.RandomState(seed), ses.export_flat()[0], n)


def _same(lib, ses, q, what, stats_width=None):
    """Every kind, flag value and maxHits, with and without the count, against the oracle; returns the flag-less counts."""
    plain = None
    for flags in FLAGS:
        want_any = _oracle(lib, ses, q, oc.ANY, flags)
        assert _device(lib, ses, q, oc.ANY, flags).tobytes() == want_any.tobytes(), (what, "ANY", flags)
        for k in MAX_HITS:
            want_rows, want_counts = _oracle(lib, ses, q, oc.LIST, flags, k)
            rows, counts = _device(lib, ses, q, oc.LIST, flags, k)
            bad = np.nonzero((rows != want_rows).any(1) | (counts != want_counts))[0]
            assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), "%s, flags %d, maxHits %d: %d queries differ, first %d got %r %d want %r %d" % (
                what, flags, k, len(bad), bad[0], rows[bad[0]], counts[bad[0]], want_rows[bad[0]], want_counts[bad[0]])
            assert _device(lib, ses, q, oc.LIST, flags, k, count=False).tobytes() == want_rows.tobytes(), (what, "no count", flags, k)
            assert np.array_equal(want_any, (want_counts > 0).astype(np.uint32))
        if flags == 0:
            plain = want_counts
    if stats_width is not None:
        st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
        assert st.rays == len(q) and st.treeWidth == stats_width and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0, st.as_dict()
    return plain


@pytest.mark.parametrize("name", ["cornell", "soup", "room", "doubled"])
def test_device_is_the_oracle_on_every_tree(gpu_lib, oscenes, monkeypatch, name):
    ses = oscenes[name]
    q = _queries_of(ses, 41)
    widths = set()
    for tree in (2, 4):
        width = _force(gpu_lib, monkeypatch, ses, tree)
        widths.add(width)
        counts = _same(gpu_lib, ses, q, "%s, tree %d" % (name, tree), stats_width=width)
    assert widths == {2, 4}, "the scene carries both trees"
    share = (counts > 0).mean()
    assert 0.2 < share < 0.95 and (counts > 16).any(), "the set must cut: %.3f of the queries meet a triangle, the most %d" % (share, counts.max())
    assert (_oracle(gpu_lib, ses, q, oc.LIST, oc.SKIP_SHARED)[1] < counts).any(), "the flag must change answers"


@pytest.mark.parametrize("tree", [2, 4])
def test_special_values(gpu_lib, oscenes, monkeypatch, tree):
    for name in ("cornell", "soup"):
        ses = oscenes[name]
        tris, _ = ses.export_flat()
        q, what = oc.specials(tris)
        _force(gpu_lib, monkeypatch, ses, tree)
        for flags in FLAGS:
            rows, counts = _device(gpu_lib, ses, q, oc.LIST, flags)
            want_rows, want_counts = _oracle(gpu_lib, ses, q, oc.LIST, flags)
            assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), [(w, g, x) for w, g, x in zip(what, counts, want_counts) if g != x]
            hits = _device(gpu_lib, ses, q, oc.ANY, flags)
            assert hits.tobytes() == _oracle(gpu_lib, ses, q, oc.ANY, flags).tobytes()
            got = dict(zip(what, zip(counts, hits)))
            for w in ("a NaN vertex", "an inf vertex", "a -inf vertex", "a query far outside", "a point 1e30 away"):
                assert got[w] == (0, 0), (w, got[w])
            assert got["a query that contains the whole scene"] == (len(tris), 1)
            if flags == 0:
                assert got["a point-sized query at a scene vertex"][0] >= 1 and got["a 1e30 vertex"][0] >= 1


@pytest.mark.parametrize("n", COUNTS)
def test_counts_across_chunk_and_wave_edges(gpu_lib, oscenes, n):
    ses = oscenes["soup"]
    q = np.ascontiguousarray(_queries_of(ses, 43, n=600)[-n:])    # (the specials are at the end)
    for flags in FLAGS:
        assert _device(gpu_lib, ses, q, oc.ANY, flags).tobytes() == _oracle(gpu_lib, ses, q, oc.ANY, flags).tobytes(), (n, flags)
        rows, counts = _device(gpu_lib, ses, q, oc.LIST, flags, 4)
        want_rows, want_counts = _oracle(gpu_lib, ses, q, oc.LIST, flags, 4)
        assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), (n, flags)
    # the device entry writes n rows and n counts and nothing behind them
    dev = torch.from_numpy(q.view(np.float32).reshape(n, 12)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for k in (1, 3, 16):
        out = torch.full((n * k + 8,), CANARY, dtype=torch.int32, device="cuda")
        cnt = torch.full((n + 8,), CANARY, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert gpu_lib.RaylibAMD_OverlapTrianglesDevice(ses.scene, oc.LIST, 0, ptr(dev), n, k, ptr(out), ptr(cnt), None) == 1
        o, c = out.cpu().numpy(), cnt.cpu().numpy()
        want_rows, want_counts = _oracle(gpu_lib, ses, q, oc.LIST, 0, k)
        assert o[:n * k].tobytes() == want_rows.tobytes() and (o[n * k:] == CANARY).all(), (n, k)
        assert c[:n].tobytes() == want_counts.tobytes() and (c[n:] == CANARY).all(), (n, k)
    out = torch.full((n + 8,), CANARY, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert gpu_lib.RaylibAMD_OverlapTrianglesDevice(ses.scene, oc.ANY, 0, ptr(dev), n, 0, ptr(out), None, None) == 1
    o = out.cpu().numpy()
    assert o[:n].tobytes() == _oracle(gpu_lib, ses, q, oc.ANY).tobytes() and (o[n:] == CANARY).all()


def test_device_entry_on_torch_tensors(gpu_lib, oscenes):
    ses = oscenes["soup"]
    q = np.ascontiguousarray(_queries_of(ses, 47))
    n = len(q)
    words = q.view(np.float32).reshape(n, 12)
    want_any = _oracle(gpu_lib, ses, q, oc.ANY, oc.SKIP_SHARED)
    want_rows, want_counts = _oracle(gpu_lib, ses, q, oc.LIST, oc.SKIP_SHARED, 4)
    # on a stream of the caller's, enqueued behind a kernel that writes the queries
    src = torch.from_numpy(words).cuda()
    dev = torch.zeros_like(src)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev.copy_(src)
        got_any = binding.overlap_triangles(gpu_lib, ses.scene, dev, oc.ANY, oc.SKIP_SHARED)
        got_rows, got_counts = binding.overlap_triangles(gpu_lib, ses.scene, dev, oc.LIST, oc.SKIP_SHARED, 4)
    s.synchronize()
    assert np.array_equal(got_any.cpu().numpy().view(np.uint32), want_any)
    assert got_rows.cpu().numpy().tobytes() == want_rows.tobytes() and got_counts.cpu().numpy().tobytes() == want_counts.tobytes()
    # the null stream: synchronous, with stats
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    f = gpu_lib.RaylibAMD_OverlapTrianglesDevice
    assert f(ses.scene, oc.LIST, oc.SKIP_SHARED, ptr(dev), n, 4, ptr(out), ptr(cnt), None) == 1
    assert out.cpu().numpy().tobytes() == want_rows.tobytes() and cnt.cpu().numpy().tobytes() == want_counts.tobytes()
    st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.rays == n and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    # refusals leave the outputs untouched: a host pointer, queries off 16-byte alignment by 4 bytes, outputs off theirs
    out = torch.full((n + 1, 4), CANARY, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + 1,), CANARY, dtype=torch.int32, device="cuda")
    big = torch.zeros(n * 12 + 4, dtype=torch.float32, device="cuda")
    host_out, host_cnt = np.zeros((n, 4), np.int32), np.zeros(n, np.uint32)
    torch.cuda.synchronize()
    assert f(ses.scene, oc.LIST, 0, q.ctypes.data, n, 4, ptr(out), ptr(cnt), None) == 0
    assert f(ses.scene, oc.LIST, 0, ptr(big, 4), n, 4, ptr(out), ptr(cnt), None) == 0
    assert f(ses.scene, oc.LIST, 0, ptr(dev), n, 4, ptr(out, 2), ptr(cnt), None) == 0
    assert f(ses.scene, oc.LIST, 0, ptr(dev), n, 4, ptr(out), ptr(cnt, 2), None) == 0
    assert f(ses.scene, oc.ANY, 0, ptr(dev), n, 4, ptr(out, 1), None, None) == 0
    assert f(ses.scene, oc.LIST, 0, ptr(dev), n, 4, host_out.ctypes.data, ptr(cnt), None) == 0
    assert f(ses.scene, oc.LIST, 0, ptr(dev), n, 4, ptr(out), host_cnt.ctypes.data, None) == 0
    assert f(ses.scene, oc.ANY, 0, ptr(dev), n, 4, ptr(out), ptr(cnt), None) == 0          # outCount belongs to LIST
    assert f(ses.scene, oc.LIST, 2, ptr(dev), n, 4, ptr(out), ptr(cnt), None) == 0
    assert f(ses.scene, oc.LIST, 0, ptr(dev), n, 17, ptr(out), ptr(cnt), None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all() and (cnt.cpu().numpy() == CANARY).all()
    assert f(ses.scene, oc.LIST, 0, ptr(dev), n, 4, ptr(out, 4), ptr(cnt, 4), None) == 1    # ... and 4 bytes are enough for both
    assert gpu_lib.RaylibAMD_OverlapTriangles(ses.scene, oc.LIST, 0, None, 0, 4, None, None) == 1
    assert gpu_lib.RaylibAMD_OverlapTrianglesDevice(ses.scene, oc.ANY, 0, None, 0, 0, None, None, None) == 1


@pytest.mark.parametrize("device", [False, True], ids=["host-entry", "device-entry"])
def test_after_a_move_and_after_a_rebuild(gpu_lib, workdir, mid_scene, monkeypatch, device):
    """The room with the triangles of a fifth of its vertices displaced: the moved scene's query is the oracle's on the moved triangles and, byte for byte, the
    query on a scene built fresh from them -- on the refitted trees, and again on the trees RaylibAMD_SceneRebuild makes."""
    obj = mid_scene[1]
    with open(obj) as f:
        nv = sum(1 for line in f if line.startswith("v "))
    shift = np.random.RandomState(7).uniform(-0.05, 0.05, (nv, 3)).astype(np.float32)
    moved_obj = mc.edit_obj(obj, os.path.join(os.path.dirname(obj), "mid_overlap_moved.obj"), move_v=lambda k, p: p + shift[k] if k < nv // 5 else p)
    ses, fresh = oc.session(gpu_lib, obj), oc.session(gpu_lib, moved_obj)
    try:
        q = _queries_of(fresh, 53, n=1200)
        k = 4
        before = _device(gpu_lib, ses, q, oc.LIST, 0, k)      # (the scene is on the device, both trees: the move refits them there)
        _force(gpu_lib, monkeypatch, ses, 2)
        _device(gpu_lib, ses, q[:64], oc.ANY)
        monkeypatch.delenv("RAYLIB_QUERY_TREE")
        ok, first, end = mc.move_to(gpu_lib, ses, fresh, device=device)
        assert ok == 1 and end - first > len(ses.export_flat()[0]) // 8
        want = {(kind, flags): _oracle(gpu_lib, fresh, q, kind, flags, k) for kind in (oc.ANY, oc.LIST) for flags in FLAGS}
        assert want[(oc.LIST, 0)][1].tobytes() != before[1].tobytes(), "the move must change answers"
        flat = lambda r: r.tobytes() if isinstance(r, np.ndarray) else r[0].tobytes() + r[1].tobytes()
        for stage in ("refitted", "rebuilt"):
            if stage == "rebuilt":
                assert gpu_lib.RaylibAMD_SceneRebuild(ses.scene) == 1
            for tree in (2, 4):
                _force(gpu_lib, monkeypatch, ses, tree); _force(gpu_lib, monkeypatch, fresh, tree)
                for (kind, flags), w in want.items():
                    got = flat(_device(gpu_lib, ses, q, kind, flags, k))
                    assert got == flat(_oracle(gpu_lib, ses, q, kind, flags, k)), (stage, tree, kind, flags, "the oracle reads the moved triangles")
                    assert got == flat(w), (stage, tree, kind, flags, "the fresh scene's oracle")
                    assert got == flat(_device(gpu_lib, fresh, q, kind, flags, k)), (stage, tree, kind, flags, "the fresh scene's query")
    finally:
        ses.close(); fresh.close()


# the stacks' capacity edges (tests/stack_edges.py): (scene, RAYLIB_QUERY_TREE, the tree and the stack the planner must pick)
EDGES = [("cone_d32", 2, 2, 32), ("cone_d33", 2, 2, 64), ("cone_d32", 4, 4, 32), ("cone_d33", 4, 4, 64), ("cone_n64", 4, 4, 64), ("cone_n65", 4, 2, 32),
         ("chain_l16", 2, 2, 32), ("chain_l17", 2, 2, 64)]


def _edge_queries(tris):
    """The walk pushes most where a query's box meets every box of the tree: a query whose box contains the scene pushes the other child (the other three) at
    every level of the deepest path.  Then the query that contains the whole scene, the scene's own triangles, and each of them jittered."""
    sp, what = oc.specials(tris)
    keep = [what.index("a query whose box contains the scene"), what.index("a query that contains the whole scene")]
    T = oc.tri_array(tris)
    rng = np.random.RandomState(3)
    return np.concatenate([sp[keep], oc.as_queries(T), oc.as_queries(oc.own_triangles(rng, tris, len(T), jitter=0.3))])


@pytest.mark.parametrize("name,env,width,stack", EDGES, ids=["%s-tree%d" % (e[0], e[1]) for e in EDGES])
def test_stack_capacity_edges(gpu_lib, workdir, monkeypatch, name, env, width, stack):
    spec = se.SCENES[name]
    ses, _ = se.make_session(gpu_lib, spec, os.path.join(str(workdir), "overlap_edges"), name)
    try:
        tn = se.tree_numbers(gpu_lib, ses.scene)
        assert (tn["depth"], tn["need4"]) == (spec["depth"], spec["need4"]), tn
        monkeypatch.setenv("RAYLIB_QUERY_TREE", str(env))
        rc, p = binding.plan_overlap(gpu_lib, ses.scene, oc.LIST)
        assert rc == 1 and (p["treeWidth"], p["stack"]) == (width, stack), p
        tris, _ = ses.export_flat()
        q = _edge_queries(tris)
        for flags in FLAGS:
            rows, counts = _device(gpu_lib, ses, q, oc.LIST, flags)
            want_rows, want_counts = _oracle(gpu_lib, ses, q, oc.LIST, flags)
            assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), (name, env, flags, "a dropped push shows as a difference from the oracle")
            assert _device(gpu_lib, ses, q, oc.ANY, flags).tobytes() == _oracle(gpu_lib, ses, q, oc.ANY, flags).tobytes(), (name, env, flags)
        assert _oracle(gpu_lib, ses, q, oc.LIST, 0)[1][1] == len(tris), "the query that contains the whole scene meets every triangle: nothing of the tree is left out"
    finally:
        ses.close()


def test_behind_a_multi_rank_frame_in_flight(gpu_lib, workdir):
    """tests/overlap_rank_child.py under three ranks on one device: Raylib_Render, then at once the overlap query (host entry and device entry).  The query
    equals the oracle, and the frame equals the one-rank frame of this process."""
    import overlap_rank_child as child
    out = os.path.join(str(workdir), "overlap_rank.npz")
    env = dict(os.environ)
    for k in ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_QUERY_TREE"):
        env.pop(k, None)
    env.update(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0")
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(workdir), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    one = child.run(gpu_lib, workdir)
    assert int(got["ranks"]) == 3 and int(one["ranks"]) == 1
    for key in ("rows_host_entry", "rows_device_entry", "counts_host_entry", "counts_device_entry", "any_host_entry"):
        assert got[key].tobytes() == got[key.split("_")[0] + "_oracle"].tobytes(), key
        assert got[key].tobytes() == one[key].tobytes(), key
    assert (got["counts_oracle"] > 0).any() and (got["counts_oracle"] == 0).any()
    assert bool(helpers.same(got["frame"], one["frame"]).all()), "the frame in flight behind the query is not the one-rank frame"
