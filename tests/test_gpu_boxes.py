"""Oriented-box range queries on the device (RaylibAMD_OverlapBoxes / RaylibAMD_OverlapBoxesDevice, csrc/rl_k_overlap_box.inl): the result equals the host oracle
RaylibAMD_OverlapBoxesHost -- a loop over every triangle, itself held to a NumPy restatement by tests/test_box_host.py -- BYTE FOR BYTE, with no tolerance, for
all three kinds, for maxHits 1, 4 and 16 with and without the count, on every tree a scene carries, for every count around the chunk and wave edges, for masks
around the word edges, after the scene's triangles have moved and its trees were refitted or rebuilt, at the stacks' capacity edges, and behind a multi-rank
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
import box_cases as bc
import stack_edges as se
from raylib_amd import binding

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 513)
MAX_HITS = (1, 4, 16)
CANARY = 0x5a5a5a5a


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


@pytest.fixture(scope="module")
def bscenes(gpu_lib, workdir, mid_scene):
    d = os.path.join(str(workdir), "boxes_gpu"); os.makedirs(d, exist_ok=True)
    own = {"cornell": bc.session(gpu_lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
           "soup": bc.session(gpu_lib, scenes.soup(os.path.join(d, "soup.obj"), 10000)[0]),
           "doubled": bc.session(gpu_lib, bc.write_soup(os.path.join(d, "doubled.obj"), 500, seed=5, doubled=True))}
    out = dict(own); out["room"] = mid_scene[0]
    yield out
    for s in own.values():
        s.close()


def _oracle(lib, ses, q, kind, k=16):
    return binding.overlap_boxes(lib, ses.scene, q, kind, k, host=True)


def _device(lib, ses, q, kind, k=16, count=True):
    return binding.overlap_boxes(lib, ses.scene, q, kind, k, count=count)


def _force(lib, monkeypatch, ses, tree):
    """RAYLIB_QUERY_TREE=tree (read per call); returns the width of the tree the planner then walks."""
    monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))
    rc, p = binding.plan_overlap_boxes(lib, ses.scene, bc.LIST)
    assert rc == 1
    return p["treeWidth"]


def _queries_of(ses, seed, n=1200):
    return np.ascontiguousarray(bc.query_set(np.random.RandomState(seed), ses.export_flat()[0], n))


def _stats(lib, n, width):
    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.rays == n and st.treeWidth == width and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0, st.as_dict()


def _same(lib, ses, q, what, stats_width=None):
    """Every kind and maxHits, with and without the count, against the oracle; returns the oracle's counts and mask."""
    want_any = _oracle(lib, ses, q, bc.ANY)
    assert _device(lib, ses, q, bc.ANY).tobytes() == want_any.tobytes(), (what, "ANY")
    if stats_width is not None:
        _stats(lib, len(q), stats_width)
    for k in MAX_HITS:
        want_rows, want_counts = _oracle(lib, ses, q, bc.LIST, k)
        rows, counts = _device(lib, ses, q, bc.LIST, k)
        bad = np.nonzero((rows != want_rows).any(1) | (counts != want_counts))[0]
        assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), "%s, maxHits %d: %d queries differ, first %d got %r %d want %r %d" % (
            what, k, len(bad), bad[0], rows[bad[0]], counts[bad[0]], want_rows[bad[0]], want_counts[bad[0]])
        assert _device(lib, ses, q, bc.LIST, k, count=False).tobytes() == want_rows.tobytes(), (what, "no count", k)
        assert np.array_equal(want_any, (want_counts > 0).astype(np.uint32))
    if stats_width is not None:
        _stats(lib, len(q), stats_width)
    want_mask = _oracle(lib, ses, q, bc.MARK)
    mask = _device(lib, ses, q, bc.MARK)
    assert mask.tobytes() == want_mask.tobytes(), (what, "MARK", np.nonzero(mask != want_mask)[0][:8])
    if stats_width is not None:
        _stats(lib, len(q), stats_width)
    return want_counts, want_mask


@pytest.mark.parametrize("name", ["cornell", "soup", "room", "doubled"])
def test_device_is_the_oracle_on_every_tree(gpu_lib, bscenes, monkeypatch, name):
    ses = bscenes[name]
    n = 1200
    q = _queries_of(ses, 41, n)
    m = gpu_lib.RaylibAMD_SceneNumTriangles(ses.scene)
    widths = set()
    for tree in (2, 4):
        width = _force(gpu_lib, monkeypatch, ses, tree)
        widths.add(width)
        counts, mask = _same(gpu_lib, ses, q, "%s, tree %d" % (name, tree), stats_width=width)
        lead = np.ascontiguousarray(q[:bc.LEAD])
        part = _device(gpu_lib, ses, lead, bc.MARK)
        assert part.tobytes() == _oracle(gpu_lib, ses, lead, bc.MARK).tobytes()
    assert widths == {2, 4}, "the scene carries both trees"
    core = bc.core_count(n)
    share = (counts[:core] > 0).mean()
    assert 0.2 < share < 0.95 and (counts > 16).any(), "the set must cut: %.3f of the queries meet a triangle, the most %d" % (share, counts.max())
    bits = int(np.unpackbits(part.view(np.uint8)).sum())
    assert 0 < bits < m, "a mask that is neither empty nor full: %d of %d" % (bits, m)
    assert int(np.unpackbits(mask.view(np.uint8)).sum()) == m, "with the boxes that hold the scene every triangle is marked"


@pytest.mark.parametrize("tree", [2, 4])
def test_special_values(gpu_lib, bscenes, monkeypatch, tree):
    for name in ("cornell", "soup"):
        ses = bscenes[name]
        tris, _ = ses.export_flat()
        q, what = bc.specials(tris)
        _force(gpu_lib, monkeypatch, ses, tree)
        rows, counts = _device(gpu_lib, ses, q, bc.LIST)
        want_rows, want_counts = _oracle(gpu_lib, ses, q, bc.LIST)
        assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), [(w, g, x) for w, g, x in zip(what, counts, want_counts) if g != x]
        hits = _device(gpu_lib, ses, q, bc.ANY)
        assert hits.tobytes() == _oracle(gpu_lib, ses, q, bc.ANY).tobytes()
        got = dict(zip(what, zip(counts, hits)))
        for i, w in enumerate(what):
            one = np.ascontiguousarray(q[i:i + 1])
            mask = _device(gpu_lib, ses, one, bc.MARK)
            assert mask.tobytes() == _oracle(gpu_lib, ses, one, bc.MARK).tobytes(), w
            if "NaN" in w or "inf" in w or w in ("a negative half extent", "a box 1e30 away"):
                assert got[w] == (0, 0) and not mask.any(), (w, got[w])
        assert got["a half extent of 1e30"] == (len(tris), 1)
        assert got["a triangle strictly inside the box"][0] >= 1 and got["zeroed axes"][0] >= 1 and got["a -0.0 half extent"][0] >= 1


@pytest.mark.parametrize("n", COUNTS)
def test_counts_across_chunk_and_wave_edges(gpu_lib, bscenes, n):
    ses = bscenes["soup"]
    q = np.ascontiguousarray(_queries_of(ses, 43, n=600)[-n:])    # (the specials are at the end)
    assert _device(gpu_lib, ses, q, bc.ANY).tobytes() == _oracle(gpu_lib, ses, q, bc.ANY).tobytes(), n
    rows, counts = _device(gpu_lib, ses, q, bc.LIST, 4)
    want_rows, want_counts = _oracle(gpu_lib, ses, q, bc.LIST, 4)
    assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), n
    assert _device(gpu_lib, ses, q, bc.MARK).tobytes() == _oracle(gpu_lib, ses, q, bc.MARK).tobytes(), n
    # the device entry writes n rows and n counts and nothing behind them
    dev = torch.from_numpy(q.view(np.float32).reshape(n, 16)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for k in (1, 3, 16):
        out = torch.full((n * k + 8,), CANARY, dtype=torch.int32, device="cuda")
        cnt = torch.full((n + 8,), CANARY, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert gpu_lib.RaylibAMD_OverlapBoxesDevice(ses.scene, bc.LIST, ptr(dev), n, k, ptr(out), ptr(cnt), None) == 1
        o, c = out.cpu().numpy(), cnt.cpu().numpy()
        want_rows, want_counts = _oracle(gpu_lib, ses, q, bc.LIST, k)
        assert o[:n * k].tobytes() == want_rows.tobytes() and (o[n * k:] == CANARY).all(), (n, k)
        assert c[:n].tobytes() == want_counts.tobytes() and (c[n:] == CANARY).all(), (n, k)
    out = torch.full((n + 8,), CANARY, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert gpu_lib.RaylibAMD_OverlapBoxesDevice(ses.scene, bc.ANY, ptr(dev), n, 0, ptr(out), None, None) == 1
    o = out.cpu().numpy()
    assert o[:n].tobytes() == _oracle(gpu_lib, ses, q, bc.ANY).tobytes() and (o[n:] == CANARY).all()


@pytest.mark.parametrize("m", [31, 32, 33, 65])
def test_mark_around_the_word_edges(gpu_lib, workdir, monkeypatch, m):
    """Scenes of m triangles: the last word's spare bits are 0, a canary word behind the mask is untouched, and a mask pre-filled with ones comes back as the
    answer -- the call clears it."""
    d = os.path.join(str(workdir), "boxes_gpu"); os.makedirs(d, exist_ok=True)
    ses = bc.session(gpu_lib, bc.write_soup(os.path.join(d, "soup_%d.obj" % m), m, seed=m))
    try:
        assert gpu_lib.RaylibAMD_SceneNumTriangles(ses.scene) == m
        words = (m + 31) // 32
        q = _queries_of(ses, 59, n=200)
        n = len(q)
        core = np.ascontiguousarray(q[:40])
        ptr = lambda t: C.c_void_p(t.data_ptr())
        for tree in (2, 4):
            monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))
            for qs in (q, core):
                want = _oracle(gpu_lib, ses, qs, bc.MARK)
                assert len(want) == words and not np.unpackbits(want.view(np.uint8), bitorder="little")[m:].any()
                assert _device(gpu_lib, ses, qs, bc.MARK).tobytes() == want.tobytes(), (m, tree)
                dev = torch.from_numpy(qs.view(np.float32).reshape(len(qs), 16)).cuda()
                out = torch.full((words + 4,), -1, dtype=torch.int32, device="cuda")    # all ones, and behind the mask too
                torch.cuda.synchronize()
                assert gpu_lib.RaylibAMD_OverlapBoxesDevice(ses.scene, bc.MARK, ptr(dev), len(qs), 0, ptr(out), None, None) == 1
                o = out.cpu().numpy().view(np.uint32)
                assert o[:words].tobytes() == want.tobytes() and (o[words:] == 0xffffffff).all(), (m, tree)
            assert int(np.unpackbits(_oracle(gpu_lib, ses, q, bc.MARK).view(np.uint8)).sum()) == m
            part = int(np.unpackbits(_oracle(gpu_lib, ses, core, bc.MARK).view(np.uint8)).sum())
            assert 0 < part < m, part
        # n == 0: the whole mask, all zero; through the host entry and the device entry
        host = np.full(words + 1, CANARY, np.uint32)
        assert gpu_lib.RaylibAMD_OverlapBoxes(ses.scene, bc.MARK, None, 0, 0, host.ctypes.data, None) == 1
        assert not host[:words].any() and host[words] == CANARY
        out = torch.full((words + 1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert gpu_lib.RaylibAMD_OverlapBoxesDevice(ses.scene, bc.MARK, None, 0, 0, ptr(out), None, None) == 1
        o = out.cpu().numpy()
        assert not o[:words].any() and o[words] == -1
    finally:
        ses.close()


def test_mark_is_an_or_whatever_the_cut(gpu_lib, bscenes):
    """The whole mask equals the oracle's; it is identical with the same queries in reversed order, and one call of 513 equals the OR of 513 calls of one."""
    ses = bscenes["soup"]
    q = np.ascontiguousarray(_queries_of(ses, 67, n=600)[:513])
    want = _oracle(gpu_lib, ses, q, bc.MARK)
    assert _device(gpu_lib, ses, q, bc.MARK).tobytes() == want.tobytes()
    assert _device(gpu_lib, ses, np.ascontiguousarray(q[::-1]), bc.MARK).tobytes() == want.tobytes()
    ored = np.zeros_like(want)
    for i in range(len(q)):
        ored |= _device(gpu_lib, ses, q[i:i + 1], bc.MARK)
    assert ored.tobytes() == want.tobytes()
    bits = int(np.unpackbits(want.view(np.uint8)).sum())
    assert 0 < bits < gpu_lib.RaylibAMD_SceneNumTriangles(ses.scene)


def test_device_entry_on_torch_tensors(gpu_lib, bscenes):
    ses = bscenes["soup"]
    q = _queries_of(ses, 47)
    n = len(q)
    words16 = q.view(np.float32).reshape(n, 16)
    m = gpu_lib.RaylibAMD_SceneNumTriangles(ses.scene)
    words = (m + 31) // 32
    want_any = _oracle(gpu_lib, ses, q, bc.ANY)
    want_rows, want_counts = _oracle(gpu_lib, ses, q, bc.LIST, 4)
    lead = np.ascontiguousarray(q[:200])
    want_mask = _oracle(gpu_lib, ses, lead, bc.MARK)
    # on a stream of the caller's, enqueued behind a kernel that writes the queries
    src = torch.from_numpy(words16).cuda()
    dev = torch.zeros_like(src)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev.copy_(src)
        got_any = binding.overlap_boxes(gpu_lib, ses.scene, dev, bc.ANY)
        got_rows, got_counts = binding.overlap_boxes(gpu_lib, ses.scene, dev, bc.LIST, 4)
        got_mask = binding.overlap_boxes(gpu_lib, ses.scene, dev[:200], bc.MARK)
    s.synchronize()
    assert np.array_equal(got_any.cpu().numpy().view(np.uint32), want_any)
    assert got_rows.cpu().numpy().tobytes() == want_rows.tobytes() and got_counts.cpu().numpy().tobytes() == want_counts.tobytes()
    assert got_mask.cpu().numpy().tobytes() == want_mask.tobytes()
    # the null stream: synchronous, with stats
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    f = gpu_lib.RaylibAMD_OverlapBoxesDevice
    assert f(ses.scene, bc.LIST, ptr(dev), n, 4, ptr(out), ptr(cnt), None) == 1
    assert out.cpu().numpy().tobytes() == want_rows.tobytes() and cnt.cpu().numpy().tobytes() == want_counts.tobytes()
    st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.rays == n and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    # refusals leave the outputs untouched: a host pointer, queries off 16-byte alignment by 4 bytes, outputs off theirs; a refused MARK does not clear
    out = torch.full((n + 1, 4), CANARY, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + 1,), CANARY, dtype=torch.int32, device="cuda")
    mask = torch.full((words + 1,), CANARY, dtype=torch.int32, device="cuda")
    big = torch.zeros(n * 16 + 4, dtype=torch.float32, device="cuda")
    host_out, host_cnt, host_mask = np.zeros((n, 4), np.int32), np.zeros(n, np.uint32), np.full(words, CANARY, np.uint32)
    torch.cuda.synchronize()
    assert f(ses.scene, bc.LIST, q.ctypes.data, n, 4, ptr(out), ptr(cnt), None) == 0
    assert f(ses.scene, bc.LIST, ptr(big, 4), n, 4, ptr(out), ptr(cnt), None) == 0
    assert f(ses.scene, bc.LIST, ptr(dev), n, 4, ptr(out, 2), ptr(cnt), None) == 0
    assert f(ses.scene, bc.LIST, ptr(dev), n, 4, ptr(out), ptr(cnt, 2), None) == 0
    assert f(ses.scene, bc.ANY, ptr(dev), n, 4, ptr(out, 1), None, None) == 0
    assert f(ses.scene, bc.LIST, ptr(dev), n, 4, host_out.ctypes.data, ptr(cnt), None) == 0
    assert f(ses.scene, bc.LIST, ptr(dev), n, 4, ptr(out), host_cnt.ctypes.data, None) == 0
    assert f(ses.scene, bc.ANY, ptr(dev), n, 4, ptr(out), ptr(cnt), None) == 0           # outCount belongs to LIST
    assert f(ses.scene, bc.LIST, ptr(dev), n, 17, ptr(out), ptr(cnt), None) == 0
    assert f(ses.scene, 3, ptr(dev), n, 4, ptr(out), None, None) == 0
    assert f(ses.scene, bc.MARK, ptr(dev), n, 4, ptr(mask), ptr(cnt), None) == 0          # ... nor to MARK
    assert f(ses.scene, bc.MARK, q.ctypes.data, n, 4, ptr(mask), None, None) == 0
    assert f(ses.scene, bc.MARK, ptr(big, 4), n, 4, ptr(mask), None, None) == 0
    assert f(ses.scene, bc.MARK, ptr(dev), n, 4, ptr(mask, 2), None, None) == 0
    assert f(ses.scene, bc.MARK, ptr(dev), n, 4, host_mask.ctypes.data, None, None) == 0
    assert f(ses.scene, bc.MARK, None, 0, 4, ptr(mask, 2), None, None) == 0
    assert f(ses.scene, bc.MARK, None, 0, 4, host_mask.ctypes.data, None, None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all() and (cnt.cpu().numpy() == CANARY).all()
    assert (mask.cpu().numpy() == CANARY).all() and (host_mask == CANARY).all(), "a refused MARK does not clear"
    assert f(ses.scene, bc.LIST, ptr(dev), n, 4, ptr(out, 4), ptr(cnt, 4), None) == 1    # ... and 4 bytes are enough for both
    assert gpu_lib.RaylibAMD_OverlapBoxes(ses.scene, bc.LIST, None, 0, 4, None, None) == 1
    assert gpu_lib.RaylibAMD_OverlapBoxesDevice(ses.scene, bc.ANY, None, 0, 0, None, None, None) == 1


@pytest.mark.parametrize("device", [False, True], ids=["host-entry", "device-entry"])
def test_after_a_move_and_after_a_rebuild(gpu_lib, workdir, mid_scene, monkeypatch, device):
    """The room with the triangles of a fifth of its vertices displaced: the moved scene's query is the oracle's on the moved triangles and, byte for byte, the
    query on a scene built fresh from them -- on the refitted trees, and again on the trees RaylibAMD_SceneRebuild makes."""
    obj = mid_scene[1]
    with open(obj) as f:
        nv = sum(1 for line in f if line.startswith("v "))
    shift = np.random.RandomState(7).uniform(-0.05, 0.05, (nv, 3)).astype(np.float32)
    moved_obj = mc.edit_obj(obj, os.path.join(os.path.dirname(obj), "mid_boxes_moved.obj"), move_v=lambda k, p: p + shift[k] if k < nv // 5 else p)
    ses, fresh = bc.session(gpu_lib, obj), bc.session(gpu_lib, moved_obj)
    try:
        q = np.ascontiguousarray(_queries_of(fresh, 53, n=600)[:bc.core_count(600)])
        k = 4
        before = _device(gpu_lib, ses, q, bc.LIST, k)      # (the scene is on the device, both trees: the move refits them there)
        _force(gpu_lib, monkeypatch, ses, 2)
        _device(gpu_lib, ses, q[:64], bc.ANY)
        monkeypatch.delenv("RAYLIB_QUERY_TREE")
        ok, first, end = mc.move_to(gpu_lib, ses, fresh, device=device)
        assert ok == 1 and end - first > len(ses.export_flat()[0]) // 8
        want = {kind: _oracle(gpu_lib, fresh, q, kind, k) for kind in (bc.ANY, bc.LIST, bc.MARK)}
        assert want[bc.LIST][1].tobytes() != before[1].tobytes(), "the move must change answers"
        flat = lambda r: r.tobytes() if isinstance(r, np.ndarray) else r[0].tobytes() + r[1].tobytes()
        for stage in ("refitted", "rebuilt"):
            if stage == "rebuilt":
                assert gpu_lib.RaylibAMD_SceneRebuild(ses.scene) == 1
            for tree in (2, 4):
                _force(gpu_lib, monkeypatch, ses, tree); _force(gpu_lib, monkeypatch, fresh, tree)
                for kind, w in want.items():
                    got = flat(_device(gpu_lib, ses, q, kind, k))
                    assert got == flat(_oracle(gpu_lib, ses, q, kind, k)), (stage, tree, kind, "the oracle reads the moved triangles")
                    assert got == flat(w), (stage, tree, kind, "the fresh scene's oracle")
                    assert got == flat(_device(gpu_lib, fresh, q, kind, k)), (stage, tree, kind, "the fresh scene's query")
    finally:
        ses.close(); fresh.close()


# the stacks' capacity edges (tests/stack_edges.py): (scene, RAYLIB_QUERY_TREE, the tree and the stack the planner must pick)
EDGES = [("cone_d32", 2, 2, 32), ("cone_d33", 2, 2, 64), ("cone_d32", 4, 4, 32), ("cone_d33", 4, 4, 64), ("cone_n64", 4, 4, 64), ("cone_n65", 4, 2, 32),
         ("chain_l16", 2, 2, 32), ("chain_l17", 2, 2, 64)]


@pytest.mark.parametrize("name,env,width,stack", EDGES, ids=["%s-tree%d" % (e[0], e[1]) for e in EDGES])
def test_stack_capacity_edges(gpu_lib, workdir, monkeypatch, name, env, width, stack):
    """A box that holds the whole scene meets every box of the tree: the walk pushes the other child (the other three) at every level of the deepest path."""
    spec = se.SCENES[name]
    ses, _ = se.make_session(gpu_lib, spec, os.path.join(str(workdir), "boxes_edges"), name)
    try:
        tn = se.tree_numbers(gpu_lib, ses.scene)
        assert (tn["depth"], tn["need4"]) == (spec["depth"], spec["need4"]), tn
        monkeypatch.setenv("RAYLIB_QUERY_TREE", str(env))
        rc, p = binding.plan_overlap_boxes(gpu_lib, ses.scene, bc.LIST)
        assert rc == 1 and (p["treeWidth"], p["stack"]) == (width, stack), p
        tris, _ = ses.export_flat()
        rng = np.random.RandomState(3)
        q = np.ascontiguousarray(np.concatenate([bc.enclosing_boxes(rng, tris, 2), bc.own_boxes(rng, tris, 64), bc.own_boxes(rng, tris, 64, jitter=0.5)]))
        rows, counts = _device(gpu_lib, ses, q, bc.LIST)
        want_rows, want_counts = _oracle(gpu_lib, ses, q, bc.LIST)
        assert rows.tobytes() == want_rows.tobytes() and counts.tobytes() == want_counts.tobytes(), (name, env, "a dropped push shows as a difference from the oracle")
        assert _device(gpu_lib, ses, q, bc.ANY).tobytes() == _oracle(gpu_lib, ses, q, bc.ANY).tobytes(), (name, env)
        one = np.ascontiguousarray(q[:1])
        mask = _device(gpu_lib, ses, one, bc.MARK)
        assert mask.tobytes() == _oracle(gpu_lib, ses, one, bc.MARK).tobytes(), (name, env)
        assert want_counts[0] == len(tris) and int(np.unpackbits(mask.view(np.uint8)).sum()) == len(tris), "the box that holds the scene meets every triangle: nothing of the tree is left out"
    finally:
        ses.close()


def test_behind_a_multi_rank_frame_in_flight(gpu_lib, workdir):
    """tests/box_rank_child.py under three ranks on one device: Raylib_Render, then at once the box queries (host entry and device entry).  The queries equal
    the oracle, and the frame equals the one-rank frame of this process."""
    import box_rank_child as child
    out = os.path.join(str(workdir), "box_rank.npz")
    env = dict(os.environ)
    for k in ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_QUERY_TREE"):
        env.pop(k, None)
    env.update(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0")
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(workdir), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    one = child.run(gpu_lib, workdir)
    assert int(got["ranks"]) == 3 and int(one["ranks"]) == 1
    for key in ("rows_host_entry", "rows_device_entry", "counts_host_entry", "counts_device_entry", "any_host_entry", "mark_host_entry", "mark_device_entry"):
        assert got[key].tobytes() == got[key.split("_")[0] + "_oracle"].tobytes(), key
        assert got[key].tobytes() == one[key].tobytes(), key
    assert (got["counts_oracle"] > 0).any() and (got["counts_oracle"] == 0).any() and got["mark_oracle"].any()
    assert bool(helpers.same(got["frame"], one["frame"]).all()), "the frame in flight behind the query is not the one-rank frame"
