"""Contact segments on the device (RaylibAMD_OverlapContacts / RaylibAMD_OverlapContactsDevice, k_overlap_contacts of csrc/rl_k_overlap.inl): index rows, records
and counts equal the host oracle RaylibAMD_OverlapContactsHost -- a loop over every triangle, itself held to a NumPy restatement by
tests/test_contact_host.py -- BYTE FOR BYTE, with no tolerance: on every tree a scene carries, with and without the shared-vertex flag, for maxHits 1 and 16
with and without the count, for every count around the chunk and wave edges, on the special values, the exact cases and the edge-touching set, through the
device entry on torch tensors, after the scene's triangles have moved and its trees were refitted or rebuilt, at the stacks' capacity edges, and behind a
multi-rank frame in flight."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch    # before the library is loaded: the device entry is handed torch's tensors

import helpers
from helpers import scenes
import contact_cases as cc
import move_cases as mc
import overlap_cases as oc
import stack_edges as se
from raylib_amd import binding

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 513)    # tests/test_gpu_overlap.py COUNTS
MAX_HITS = (1, 16)
FLAGS = (0, oc.SKIP_SHARED)
CANARY = 0x5a5a5a5a


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


@pytest.fixture(scope="module")
def oscenes(gpu_lib, workdir, mid_scene):
    d = os.path.join(str(workdir), "contact_gpu"); os.makedirs(d, exist_ok=True)
    own = {"cornell": oc.session(gpu_lib, scenes.cornell(os.path.join(d, "cornell.obj"))[0]),
           "soup": oc.session(gpu_lib, scenes.soup(os.path.join(d, "soup.obj"), 10000)[0]),
           "doubled": oc.session(gpu_lib, oc.write_soup(os.path.join(d, "doubled.obj"), 500, seed=5, doubled=True))}
    out = dict(own); out["room"] = mid_scene[0]
    yield out
    for s in own.values():
        s.close()


def _oracle(lib, ses, q, flags=0, k=16):
    return binding.overlap_contacts(lib, ses.scene, q, flags, k, host=True)


def _device(lib, ses, q, flags=0, k=16, count=True):
    return binding.overlap_contacts(lib, ses.scene, q, flags, k, count=count)


def _force(lib, monkeypatch, ses, tree):
    """RAYLIB_QUERY_TREE=tree (read per call); returns the width of the tree the planner then walks."""
    monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))
    rc, p = binding.plan_overlap_contacts(lib, ses.scene)
    assert rc == 1
    return p["treeWidth"]


def _queries_of(ses, seed, n=2000):
    return oc.query_set(np.random.RandomState(seed), ses.export_flat()[0], n)


def _equal(got, want, what):
    rows, recs, counts = got
    want_rows, want_recs, want_counts = want
    assert rows.tobytes() == want_rows.tobytes(), (what, "rows")
    if want_counts is not None and counts is not None:
        assert counts.tobytes() == want_counts.tobytes(), (what, "counts")
    bad = np.argwhere(recs != want_recs)
    assert recs.tobytes() == want_recs.tobytes(), "%s: %d records differ, first at %r: got %r, want %r" % (
        what, len(bad), bad[0], recs[tuple(bad[0])], want_recs[tuple(bad[0])])


def _same(lib, ses, q, what, stats_width=None):
    """Both flag values and every maxHits, with and without the count, against the oracle; returns the flag-less (records, counts) at maxHits 16."""
    plain = None
    for flags in FLAGS:
        for k in MAX_HITS:
            want = _oracle(lib, ses, q, flags, k)
            _equal(_device(lib, ses, q, flags, k), want, "%s, flags %d, maxHits %d" % (what, flags, k))
            _equal(_device(lib, ses, q, flags, k, count=False), want, "%s, flags %d, maxHits %d, no count" % (what, flags, k))
            assert cc.rows_are_pairs(want[0], want[1])
        if flags == 0:
            plain = want[1], want[2]
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
        recs, counts = _same(gpu_lib, ses, q, "%s, tree %d" % (name, tree), stats_width=width)
    assert widths == {2, 4}, "the scene carries both trees"
    assert (counts > 16).any() and (counts == 0).any()
    assert {cc.NONE, cc.SEGMENT, cc.NO_CROSSING} <= set(np.unique(recs["kind"]).tolist())
    monkeypatch.delenv("RAYLIB_QUERY_TREE")
    rows, list_counts = binding.overlap_triangles(gpu_lib, ses.scene, q, oc.LIST, 0, 16)
    got = _device(gpu_lib, ses, q, 0, 16)
    assert got[0].tobytes() == rows.tobytes() and got[2].tobytes() == list_counts.tobytes(), "the rows and counts are LIST's"


def test_self_contacts_of_the_doubled_soup(gpu_lib, oscenes):
    """The scene's own triangles as queries with SKIP_SHARED: a triangle reports neither itself nor its twin; where the count exceeds maxHits the row is cut and
    the count complete, and the records behind a short row are NONE."""
    ses = oscenes["doubled"]
    tris, _ = ses.export_flat()
    q = oc.as_queries(oc.tri_array(tris))
    for k in (1, 4):
        want = _oracle(gpu_lib, ses, q, oc.SKIP_SHARED, k)
        got = _device(gpu_lib, ses, q, oc.SKIP_SHARED, k)
        _equal(got, want, "self-contacts, maxHits %d" % k)
        rows, recs, counts = got
        assert (counts > 1).any() and (counts < k).any(), "the set must hold rows cut at maxHits 1 and short rows"   # (whatever meets one copy meets its twin: counts are even)
        listed = (rows >= 0).sum(1)
        assert np.array_equal(listed, np.minimum(counts, k))
        assert cc.rows_are_pairs(rows, recs)
        assert not (rows == np.arange(len(q))[:, None]).any(), "no triangle meets itself under the flag"
        assert (recs["kind"][rows >= 0] == cc.SEGMENT).mean() > 0.9, "soup triangles that meet cross"


@pytest.mark.parametrize("n", COUNTS)
def test_counts_across_chunk_and_wave_edges(gpu_lib, oscenes, n):
    ses = oscenes["soup"]
    q = np.ascontiguousarray(_queries_of(ses, 43, n=600)[-n:])    # (the specials are at the end)
    for flags in FLAGS:
        _equal(_device(gpu_lib, ses, q, flags, 4), _oracle(gpu_lib, ses, q, flags, 4), (n, flags))
    # the device entry writes n rows, n * maxHits records and n counts and nothing behind them
    dev = torch.from_numpy(q.view(np.float32).reshape(n, 12)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for k in (1, 3, 16):
        out = torch.full((n * k + 8,), CANARY, dtype=torch.int32, device="cuda")
        rec = torch.full((n * k * 8 + 8,), CANARY, dtype=torch.int32, device="cuda")
        cnt = torch.full((n + 8,), CANARY, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert gpu_lib.RaylibAMD_OverlapContactsDevice(ses.scene, 0, ptr(dev), n, k, ptr(out), ptr(rec), ptr(cnt), None) == 1
        o, r, c = out.cpu().numpy(), rec.cpu().numpy(), cnt.cpu().numpy()
        want_rows, want_recs, want_counts = _oracle(gpu_lib, ses, q, 0, k)
        assert o[:n * k].tobytes() == want_rows.tobytes() and (o[n * k:] == CANARY).all(), (n, k)
        assert r[:n * k * 8].tobytes() == want_recs.tobytes() and (r[n * k * 8:] == CANARY).all(), (n, k)
        assert c[:n].tobytes() == want_counts.tobytes() and (c[n:] == CANARY).all(), (n, k)


@pytest.mark.parametrize("tree", [2, 4])
def test_special_values(gpu_lib, oscenes, workdir, monkeypatch, tree):
    """A query with a NaN or an infinity: a row of -1, count 0, records NONE.  The exact cases.  The edge-touching set, each pair in a cell of its own: the kinds
    are the oracle's, and both SEGMENT and GAP are among them."""
    for name in ("cornell", "soup"):
        ses = oscenes[name]
        q, what = oc.specials(ses.export_flat()[0])
        _force(gpu_lib, monkeypatch, ses, tree)
        for flags in FLAGS:
            got = _device(gpu_lib, ses, q, flags)
            _equal(got, _oracle(gpu_lib, ses, q, flags), (name, flags))
            for w in ("a NaN vertex", "an inf vertex", "a -inf vertex"):
                i = what.index(w)
                assert (got[0][i] == -1).all() and got[2][i] == 0 and got[1][i].tobytes() == bytes(32 * 16), w
    d = os.path.join(str(workdir), "contact_gpu")
    T, Q = cc.exact_scene_and_queries()
    Qt, Tt = cc.edge_touching_pairs(np.random.RandomState(11), 4000, spacing=4.0)
    for label, tris, queries in (("exact", T, Q), ("touching", Tt, Qt)):
        ses = oc.session(gpu_lib, oc.write_triangles(os.path.join(d, "%s_%d.obj" % (label, tree)), tris))
        try:
            _force(gpu_lib, monkeypatch, ses, tree)
            want = _oracle(gpu_lib, ses, oc.as_queries(queries), 0, 2)
            got = _device(gpu_lib, ses, oc.as_queries(queries), 0, 2)
            _equal(got, want, label)
            assert np.array_equal(got[1]["kind"], want[1]["kind"])
            if label == "exact":
                assert got[1]["kind"][:, 0].tolist() == [c[4] for c in cc.EXACT]
            else:
                kinds = got[1]["kind"][:, 0]
                assert (kinds == cc.SEGMENT).sum() >= 100 and (kinds == cc.GAP).sum() >= 1, np.unique(kinds, return_counts=True)
        finally:
            ses.close()


def test_device_entry_on_torch_tensors(gpu_lib, oscenes):
    ses = oscenes["soup"]
    q = np.ascontiguousarray(_queries_of(ses, 47))
    n = len(q)
    words = q.view(np.float32).reshape(n, 12)
    want_rows, want_recs, want_counts = _oracle(gpu_lib, ses, q, oc.SKIP_SHARED, 4)
    # on a stream of the caller's, enqueued behind a kernel that writes the queries; the stats are left alone
    src = torch.from_numpy(words).cuda()
    dev = torch.zeros_like(src)
    _device(gpu_lib, ses, q[:100], 0, 4)
    before = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(before))
    assert before.rays == 100
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev.copy_(src)
        got_rows, got_recs, got_counts = binding.overlap_contacts(gpu_lib, ses.scene, dev, oc.SKIP_SHARED, 4)
    s.synchronize()
    assert got_rows.cpu().numpy().tobytes() == want_rows.tobytes() and got_counts.cpu().numpy().tobytes() == want_counts.tobytes()
    assert got_recs.cpu().numpy().tobytes() == want_recs.tobytes()
    after = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(after))
    assert (after.rays, after.nodesVisited, after.trisTested, after.kernelMs) == (before.rays, before.nodesVisited, before.trisTested, before.kernelMs), "a call on a stream leaves the stats alone"
    # the null stream: synchronous, with stats
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    rec = torch.empty((n, 4, 8), dtype=torch.float32, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    f = gpu_lib.RaylibAMD_OverlapContactsDevice
    assert f(ses.scene, oc.SKIP_SHARED, ptr(dev), n, 4, ptr(out), ptr(rec), ptr(cnt), None) == 1
    assert out.cpu().numpy().tobytes() == want_rows.tobytes() and cnt.cpu().numpy().tobytes() == want_counts.tobytes() and rec.cpu().numpy().tobytes() == want_recs.tobytes()
    st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.rays == n and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    # refusals leave the outputs untouched: a host pointer for each argument, the queries and the records off 16-byte alignment, rows and counts off theirs
    out = torch.full((n + 1, 4), CANARY, dtype=torch.int32, device="cuda")
    rec = torch.full((n + 1, 4, 8), CANARY, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + 1,), CANARY, dtype=torch.int32, device="cuda")
    big = torch.zeros(n * 12 + 4, dtype=torch.float32, device="cuda")
    host_out, host_rec, host_cnt = np.zeros((n, 4), np.int32), np.zeros((n, 4), cc.DTYPE), np.zeros(n, np.uint32)
    torch.cuda.synchronize()
    assert f(ses.scene, 0, q.ctypes.data, n, 4, ptr(out), ptr(rec), ptr(cnt), None) == 0
    assert f(ses.scene, 0, ptr(big, 4), n, 4, ptr(out), ptr(rec), ptr(cnt), None) == 0
    assert f(ses.scene, 0, ptr(dev), n, 4, ptr(out, 2), ptr(rec), ptr(cnt), None) == 0
    assert f(ses.scene, 0, ptr(dev), n, 4, ptr(out), ptr(rec), ptr(cnt, 2), None) == 0
    for off in (4, 8, 12):
        assert f(ses.scene, 0, ptr(dev), n, 4, ptr(out), ptr(rec, off), ptr(cnt), None) == 0, "outContact %d bytes off 16-byte alignment" % off
    assert f(ses.scene, 0, ptr(dev), n, 4, host_out.ctypes.data, ptr(rec), ptr(cnt), None) == 0
    assert f(ses.scene, 0, ptr(dev), n, 4, ptr(out), host_rec.ctypes.data, ptr(cnt), None) == 0
    assert f(ses.scene, 0, ptr(dev), n, 4, ptr(out), ptr(rec), host_cnt.ctypes.data, None) == 0
    assert f(ses.scene, 0, ptr(dev), n, 4, ptr(out), None, ptr(cnt), None) == 0
    assert f(ses.scene, 2, ptr(dev), n, 4, ptr(out), ptr(rec), ptr(cnt), None) == 0
    assert f(ses.scene, 0, ptr(dev), n, 17, ptr(out), ptr(rec), ptr(cnt), None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all() and (rec.cpu().numpy() == CANARY).all() and (cnt.cpu().numpy() == CANARY).all()
    assert f(ses.scene, 0, ptr(dev), n, 4, ptr(out, 4), ptr(rec, 16), ptr(cnt, 4), None) == 1    # ... 4, 16 and 4 bytes are enough
    assert gpu_lib.RaylibAMD_OverlapContacts(ses.scene, 0, None, 0, 4, None, None, None) == 1
    assert f(ses.scene, 0, None, 0, 4, None, None, None, None) == 1


@pytest.mark.parametrize("device", [False, True], ids=["host-entry", "device-entry"])
def test_after_a_move_and_after_a_rebuild(gpu_lib, workdir, mid_scene, monkeypatch, device):
    """The room with the triangles of a fifth of its vertices displaced: the moved scene's contacts are the oracle's on the moved triangles and, byte for byte,
    those of a scene built fresh from them -- on the refitted trees, and again on the trees RaylibAMD_SceneRebuild makes; through the host entry and the device
    entry alike."""
    obj = mid_scene[1]
    with open(obj) as f:
        nv = sum(1 for line in f if line.startswith("v "))
    shift = np.random.RandomState(7).uniform(-0.05, 0.05, (nv, 3)).astype(np.float32)
    moved_obj = mc.edit_obj(obj, os.path.join(os.path.dirname(obj), "mid_contact_moved.obj"), move_v=lambda k, p: p + shift[k] if k < nv // 5 else p)
    ses, fresh = oc.session(gpu_lib, obj), oc.session(gpu_lib, moved_obj)
    try:
        q = np.ascontiguousarray(_queries_of(fresh, 53, n=1200))
        dev = torch.from_numpy(q.view(np.float32).reshape(len(q), 12)).cuda()
        k = 4

        def on_torch(s, flags):
            rows, recs, counts = binding.overlap_contacts(gpu_lib, s.scene, dev, flags, k)
            torch.cuda.synchronize()
            return rows.cpu().numpy(), recs.cpu().numpy().view(cc.DTYPE).reshape(len(q), k), counts.cpu().numpy().view(np.uint32)

        before = _device(gpu_lib, ses, q, 0, k)      # (the scene is on the device, both trees and the slot tables: the move refits and keeps them)
        _force(gpu_lib, monkeypatch, ses, 2)
        _device(gpu_lib, ses, q[:64], 0, k)
        monkeypatch.delenv("RAYLIB_QUERY_TREE")
        ok, first, end = mc.move_to(gpu_lib, ses, fresh, device=device)
        assert ok == 1 and end - first > len(ses.export_flat()[0]) // 8
        want = {flags: _oracle(gpu_lib, fresh, q, flags, k) for flags in FLAGS}
        assert want[0][1].tobytes() != before[1].tobytes(), "the move must change the records"
        for stage in ("refitted", "rebuilt"):
            if stage == "rebuilt":
                assert gpu_lib.RaylibAMD_SceneRebuild(ses.scene) == 1
            for tree in (2, 4):
                _force(gpu_lib, monkeypatch, ses, tree); _force(gpu_lib, monkeypatch, fresh, tree)
                for flags, w in want.items():
                    got = _device(gpu_lib, ses, q, flags, k)
                    _equal(got, _oracle(gpu_lib, ses, q, flags, k), (stage, tree, flags, "the oracle reads the moved triangles"))
                    _equal(got, w, (stage, tree, flags, "the fresh scene's oracle"))
                    _equal(on_torch(ses, flags), w, (stage, tree, flags, "the device entry"))
                    _equal(_device(gpu_lib, fresh, q, flags, k), w, (stage, tree, flags, "the fresh scene's query"))
    finally:
        ses.close(); fresh.close()


# the stacks' capacity edges (tests/stack_edges.py): (scene, RAYLIB_QUERY_TREE, the tree and the stack the planner must pick) -- tests/test_gpu_overlap.py EDGES
EDGES = [("cone_d32", 2, 2, 32), ("cone_d33", 2, 2, 64), ("cone_d32", 4, 4, 32), ("cone_d33", 4, 4, 64), ("cone_n64", 4, 4, 64), ("cone_n65", 4, 2, 32),
         ("chain_l16", 2, 2, 32), ("chain_l17", 2, 2, 64)]


def _edge_queries(tris):
    """tests/test_gpu_overlap.py _edge_queries: a query whose box contains the scene pushes the other child (the other three) at every level of the deepest
    path; then the query that contains the whole scene, the scene's own triangles, and each of them jittered."""
    sp, what = oc.specials(tris)
    keep = [what.index("a query whose box contains the scene"), what.index("a query that contains the whole scene")]
    T = oc.tri_array(tris)
    rng = np.random.RandomState(3)
    return np.concatenate([sp[keep], oc.as_queries(T), oc.as_queries(oc.own_triangles(rng, tris, len(T), jitter=0.3))])


@pytest.mark.parametrize("name,env,width,stack", EDGES, ids=["%s-tree%d" % (e[0], e[1]) for e in EDGES])
def test_stack_capacity_edges(gpu_lib, workdir, monkeypatch, name, env, width, stack):
    spec = se.SCENES[name]
    ses, _ = se.make_session(gpu_lib, spec, os.path.join(str(workdir), "contact_edges"), name)
    try:
        tn = se.tree_numbers(gpu_lib, ses.scene)
        assert (tn["depth"], tn["need4"]) == (spec["depth"], spec["need4"]), tn
        monkeypatch.setenv("RAYLIB_QUERY_TREE", str(env))
        rc, p = binding.plan_overlap_contacts(gpu_lib, ses.scene)
        assert rc == 1 and (p["treeWidth"], p["stack"]) == (width, stack), p
        tris, _ = ses.export_flat()
        q = _edge_queries(tris)
        for flags in FLAGS:
            _equal(_device(gpu_lib, ses, q, flags), _oracle(gpu_lib, ses, q, flags), (name, env, flags, "a dropped push shows as a difference from the oracle"))
        assert _oracle(gpu_lib, ses, q, 0)[2][1] == len(tris), "the query that contains the whole scene meets every triangle: nothing of the tree is left out"
    finally:
        ses.close()


def test_behind_a_multi_rank_frame_in_flight(gpu_lib, workdir):
    """tests/contact_rank_child.py under three ranks on one device: Raylib_Render, then at once the contacts query (host entry and device entry).  The query
    equals the oracle, and the frame equals the one-rank frame of this process."""
    import contact_rank_child as child
    out = os.path.join(str(workdir), "contact_rank.npz")
    env = dict(os.environ)
    for k in ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_QUERY_TREE"):
        env.pop(k, None)
    env.update(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0")
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(workdir), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    one = child.run(gpu_lib, workdir)
    assert int(got["ranks"]) == 3 and int(one["ranks"]) == 1
    for key in ("rows_host_entry", "rows_device_entry", "records_host_entry", "records_device_entry", "counts_host_entry", "counts_device_entry"):
        assert got[key].tobytes() == got[key.split("_")[0] + "_oracle"].tobytes(), key
        assert got[key].tobytes() == one[key].tobytes(), key
    assert (got["counts_oracle"] > 0).any() and (got["counts_oracle"] == 0).any()
    assert bool(helpers.same(got["frame"], one["frame"]).all()), "the frame in flight behind the query is not the one-rank frame"
