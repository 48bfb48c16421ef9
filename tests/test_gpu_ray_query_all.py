"""Ordered multi-hit ray queries on the device (RaylibAMD_TraceRaysAll / RaylibAMD_TraceRaysAllDevice, csrc/rl_k_multihit.inl; include/raylib_amd.h statements
M1 to M5): against the peeled brute-force oracle of oracle/ (tests/ray_query_all_cases.py) and against RaylibAMD_TraceRaysAllHost byte for byte, on every tree
the planner offers, with and without the count; the first record against RaylibAMD_TraceRays(CLOSEST); intervals that start and end at peeled surfaces;
special bounds; ray counts around the chunk and refill edges; the device entry on a caller's stream; after a move; behind a three-rank frame in flight."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
from helpers import bits, with_interval
import ray_query_all_cases as rc
from raylib_amd import binding

pytestmark = pytest.mark.gpu

FLT_MAX = helpers.F32_MAX
SCENES = ["soup", "room", "cutout8", "cornell", "stack"]
TREES_OF = {"soup": (2, 8), "room": (2, 8), "cutout8": (2, 8), "cornell": (2,), "stack": (2,)}


@pytest.fixture(scope="module")
def cases(gpu_lib, oracle, workdir):
    S = rc.make_cases(gpu_lib, oracle, workdir, SCENES)   # (the excused cap is asserted in there, from the oracle alone)
    yield S
    for c in S.values():
        oracle.scene_destroy(c.osc)
        c.ses.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _force(lib, monkeypatch, ses, tree):
    monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))
    r, p = binding.plan_ray_query_all(lib, ses.scene, 4)
    assert r == 1 and p["treeWidth"] == tree, (tree, p)


def _host(lib, ses, rays, k, count=True):
    return binding.trace_rays_all(lib, ses.scene, rays, k, count=count, host=True)


def _dev(lib, ses, rays, k, count=True):
    return binding.trace_rays_all(lib, ses.scene, rays, k, count=count)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _first_difference(a, b):
    d = (a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(1)
    i = int(np.argmax(d))
    return "%d of %d rows differ, first %d: %s against %s" % (d.sum(), len(a), i, a[i].tolist(), b[i].tolist())


@pytest.mark.parametrize("name", SCENES)
def test_device_equals_the_peeled_oracle_and_the_host_oracle(gpu_lib, cases, monkeypatch, name):
    c, problems = cases[name], []
    assert (c.P.total >= 2).mean() > 0.05 and c.P.total.max() >= 3
    assert TREES_OF[name][-1] == (8 if binding.plan_ray_query_all(gpu_lib, c.ses.scene, 4)[1]["treeWidth"] == 8 else 2), "every tree the plan offers"
    for k in rc.MAX_HITS:
        want_h, want_c = _host(gpu_lib, c.ses, c.rays, k)
        per_tree = {}
        for tree in TREES_OF[name]:
            _force(gpu_lib, monkeypatch, c.ses, tree)
            hits, counts = _dev(gpu_lib, c.ses, c.rays, k)
            st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
            assert st.rays == len(c.rays) and st.treeWidth == tree and st.trisTested > 0, st.as_dict()
            rc.check("%s tree %d with count" % (name, tree), c.rays, c.tris, c.P, k, hits, counts, problems)
            assert hits.tobytes() == want_h.tobytes(), (name, tree, k, "with count", _first_difference(hits, want_h))
            assert np.array_equal(counts, want_c), (name, tree, k)
            plain = _dev(gpu_lib, c.ses, c.rays, k, count=False)
            assert plain.tobytes() == want_h.tobytes(), (name, tree, k, "without count", _first_difference(plain, want_h))
            per_tree[tree] = hits
            closest = binding.trace_rays(gpu_lib, c.ses.scene, c.rays, binding.QUERY_CLOSEST)
            assert closest.tobytes() == np.ascontiguousarray(hits[:, 0]).tobytes(), (name, tree, k, "hits[:, 0] is CLOSEST's record")
        first = per_tree[TREES_OF[name][0]]
        for tree in TREES_OF[name][1:]:
            assert per_tree[tree].tobytes() == first.tobytes(), (name, k, "two trees, ties included")
    assert not problems, "\n".join(problems[:20])


def test_stack_tie_groups_in_slot_order(gpu_lib, cases):
    c = cases["stack"]
    order = rc.tri_order(gpu_lib, c.ses)
    slot_of = np.zeros(30, np.int64); slot_of[order] = np.arange(30)
    group = np.where(c.rays[:, 0] == c.rays[:, 1], 6, 3)
    for k in range(1, 17):
        hits, counts = _dev(gpu_lib, c.ses, c.rays, k)
        assert np.array_equal(counts, 5 * group), k
        assert _dev(gpu_lib, c.ses, c.rays, k, count=False).tobytes() == hits.tobytes()
        for i in range(len(c.rays)):
            nh = min(k, 5 * group[i])
            assert np.array_equal(hits["t"][i, :nh], (np.arange(nh) // group[i] + 1).astype(np.float32)) and (hits["prim"][i, nh:] == -1).all(), (k, i)
            slots = slot_of[hits["prim"][i, :nh]]
            assert all((np.diff(slots[g:g + group[i]]) > 0).all() for g in range(0, nh, group[i])), (k, i, slots)


@pytest.mark.parametrize("name", ["soup", "room"])
def test_intervals_between_peeled_surfaces(gpu_lib, cases, monkeypatch, name):
    """[t_2, t_4] returns layers 2 to 4 and [t_3, t_3] the third alone (rays that are not excused and whose first four layers hold one triangle each)."""
    c = cases[name]
    T, P = c.P.T, c.P
    sel = np.isfinite(T[3]) & ~P.excused & (P.count[:4] == 1).all(0)
    assert sel.sum() >= 10, sel.sum()
    rays, T = c.rays[sel], T[:, sel]
    # (which layers lie in [t_2, t_4]: 2, 3 and 4 -- and nothing else, since the layers are every accepted t in order)
    span = with_interval(rays, T[1], T[3])
    point = with_interval(rays, T[2], T[2])
    full = _host(gpu_lib, c.ses, rays, 4)[0]
    for tree in TREES_OF[name]:
        _force(gpu_lib, monkeypatch, c.ses, tree)
        for count in (True, False):
            h = binding.trace_rays_all(gpu_lib, c.ses.scene, span, 4, count=count)
            hits, cnt = h if count else (h, None)
            assert np.array_equal(bits(hits["t"][:, :3]), bits(T[1:4].T)) and (hits["prim"][:, 3] == -1).all(), (name, tree, count)
            assert np.array_equal(hits["prim"][:, :3], full["prim"][:, 1:4])
            assert cnt is None or (cnt == 3).all()
            h = binding.trace_rays_all(gpu_lib, c.ses.scene, point, 4, count=count)
            hits, cnt = h if count else (h, None)
            assert np.array_equal(bits(hits["t"][:, 0]), bits(T[2])) and (hits["prim"][:, 1:] == -1).all(), (name, tree, count)
            assert np.array_equal(hits["prim"][:, 0], full["prim"][:, 2]) and (cnt is None or (cnt == 1).all())
        assert _same(_dev(gpu_lib, c.ses, span, 4), _host(gpu_lib, c.ses, span, 4)) and _same(_dev(gpu_lib, c.ses, point, 4), _host(gpu_lib, c.ses, point, 4))


@pytest.mark.parametrize("name", ["soup", "cornell"])
def test_special_bounds(gpu_lib, cases, monkeypatch, name):
    c = cases[name]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for tree in TREES_OF[name]:
        _force(gpu_lib, monkeypatch, c.ses, tree)
        for tmin, tmax in ((nan, FLT_MAX), (0.0, nan), (nan, nan), (5.0, 1.0), (inf, inf), (0.0, -1.0)):
            for count in (True, False):
                h = binding.trace_rays_all(gpu_lib, c.ses.scene, with_interval(c.rays, tmin, tmax), 4, count=count)
                hits, cnt = h if count else (h, None)
                assert (hits["prim"] == -1).all() and not hits.view(np.uint32)[..., [0, 2, 3]].any() and (cnt is None or not cnt.any()), (tree, tmin, tmax)
        for tmin, tmax in ((-inf, FLT_MAX), (-1.0, inf), (np.float32(-0.0), 3.0), (0.0, inf)):
            r = with_interval(c.rays, tmin, tmax)
            got, want = _dev(gpu_lib, c.ses, r, 8), _host(gpu_lib, c.ses, r, 8)
            assert _same(got, want), (name, tree, tmin, tmax, _first_difference(got[0], want[0]))
            assert _dev(gpu_lib, c.ses, r, 8, count=False).tobytes() == want[0].tobytes()
            assert tmax < FLT_MAX or (want[0]["prim"][:, 0] >= 0).sum() > len(r) // 10
        raised = _host(gpu_lib, c.ses, with_interval(c.rays, 0.0, None), 8)
        assert _same(_dev(gpu_lib, c.ses, with_interval(c.rays, -inf, None), 8), raised)          # tMin < 0 is read as +0


@pytest.mark.parametrize("name", ["soup", "cutout8"])
def test_small_ray_counts(gpu_lib, cases, monkeypatch, name):
    """n around a wave, a chunk and the 8-wide schedule's refill; row n of the output is not written."""
    c = cases[name]
    for tree in TREES_OF[name]:
        _force(gpu_lib, monkeypatch, c.ses, tree)
        for n in (1, 63, 64, 65, 513):
            rays = np.ascontiguousarray(np.resize(c.rays, (n, 8)))
            for k in (1, 4, 16):
                got, want = _dev(gpu_lib, c.ses, rays, k), _host(gpu_lib, c.ses, rays, k)
                assert _same(got, want), (name, tree, n, k)
                assert _dev(gpu_lib, c.ses, rays, k, count=False).tobytes() == want[0].tobytes(), (name, tree, n, k)
    assert gpu_lib.RaylibAMD_TraceRaysAll(c.ses.scene, None, 0, 0.0, 4, None, None) == 1
    assert gpu_lib.RaylibAMD_TraceRaysAllDevice(c.ses.scene, None, 0, 0.0, 4, None, None, None) == 1


def test_deep_tree_takes_the_64_entry_stack(gpu_lib, workdir, monkeypatch):
    """A binary tree deeper than 32 levels: the 64-entry instance, whose 64 KB stack shares the workgroup's LDS with the list (32 KB at 16 hits)."""
    import test_ray_query_host as qh
    d = os.path.join(str(workdir), "ray_query_all_deep"); os.makedirs(d, exist_ok=True)
    ses = binding.SceneSession(gpu_lib, qh._write_soup(os.path.join(d, "deep.obj"), 1000, 72), (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    try:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", "2")
        r, p = binding.plan_ray_query_all(gpu_lib, ses.scene, 16)
        assert r == 1 and (p["treeWidth"], p["stack"]) == (2, 64), p
        rng = np.random.RandomState(4)
        o = rng.uniform(-2.0, 2.0, (600, 3)).astype(np.float32)
        tgt = np.stack([2.0 ** -rng.uniform(1.0, 24.0, 600), 2.0 ** -rng.uniform(3.0, 26.0, 600), np.zeros(600)], 1)   # into the chain (tests/stack_edges.py)
        rays = helpers.rays8(o, (tgt - o).astype(np.float32), 0.0, FLT_MAX)
        for k in (1, 4, 16):
            got, want = _dev(gpu_lib, ses, rays, k), _host(gpu_lib, ses, rays, k)
            assert _same(got, want), (k, _first_difference(got[0], want[0]))
            assert _dev(gpu_lib, ses, rays, k, count=False).tobytes() == want[0].tobytes(), k
        assert (want[1] >= 3).mean() > 0.1
    finally:
        ses.close()


def test_device_entry_on_torch_tensors(gpu_lib, cases):
    c = cases["soup"]
    rays = np.ascontiguousarray(c.rays[:257])
    n, k = len(rays), 4
    want_h, want_c = _host(gpu_lib, c.ses, rays, k)
    # on a stream of the caller's, enqueued behind a kernel that writes the rays
    src = torch.from_numpy(rays).cuda()
    dev = torch.zeros_like(src)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.add(src, 0.0, out=dev)
        hits, counts = binding.trace_rays_all(gpu_lib, c.ses.scene, dev, k, count=True)
        plain = binding.trace_rays_all(gpu_lib, c.ses.scene, dev, k)
    s.synchronize()
    assert hits.cpu().numpy().tobytes() == want_h.tobytes() and plain.cpu().numpy().tobytes() == want_h.tobytes()
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want_c)
    # the null stream: synchronous, with stats; a NumPy array through the device entry
    got = binding.trace_rays_all(gpu_lib, c.ses.scene, rays, k, count=True, device=True)
    assert _same(got, (want_h, want_c))
    st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.rays == n and st.nodesVisited > 0 and st.trisTested > 0 and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    # refusals leave the outputs untouched: host pointers, rays and records off 16-byte alignment, counts off 4-byte alignment
    ray_p = lambda t, off=0: C.cast(C.c_void_p(t.data_ptr() + off), C.POINTER(binding.Ray))
    hit_p = lambda t, off=0: C.cast(C.c_void_p(t.data_ptr() + off), C.POINTER(binding.HitT))
    cnt_p = lambda t, off=0: C.cast(C.c_void_p(t.data_ptr() + off), C.POINTER(C.c_uint32))
    out = torch.full((n * k + 1, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + 1,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    big = torch.zeros(n * 8 + 4, dtype=torch.float32, device="cuda")
    host_hits = np.full((n, k), 0, binding.HITT_DTYPE); host_cnt = np.zeros(n, np.uint32)
    torch.cuda.synchronize()
    f = gpu_lib.RaylibAMD_TraceRaysAllDevice
    assert f(c.ses.scene, rays.ctypes.data_as(C.POINTER(binding.Ray)), n, 0.0, k, hit_p(out), cnt_p(cnt), None) == 0
    assert f(c.ses.scene, ray_p(big, 4), n, 0.0, k, hit_p(out), cnt_p(cnt), None) == 0
    assert f(c.ses.scene, ray_p(dev), n, 0.0, k, hit_p(out, 4), cnt_p(cnt), None) == 0
    assert f(c.ses.scene, ray_p(dev), n, 0.0, k, hit_p(out), cnt_p(cnt, 2), None) == 0
    assert f(c.ses.scene, ray_p(dev), n, 0.0, k, C.cast(C.c_void_p(host_hits.ctypes.data), C.POINTER(binding.HitT)), cnt_p(cnt), None) == 0
    assert f(c.ses.scene, ray_p(dev), n, 0.0, k, hit_p(out), host_cnt.ctypes.data_as(C.POINTER(C.c_uint32)), None) == 0
    if torch.cuda.device_count() > 1:      # a pointer off rank 0's device
        other = torch.zeros((n * k, 4), dtype=torch.int32, device="cuda:1")
        assert f(c.ses.scene, ray_p(dev), n, 0.0, k, hit_p(other), None, None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5a5a5a5a).all() and (cnt.cpu().numpy() == 0x5a5a5a5a).all() and not host_cnt.any()
    assert f(c.ses.scene, ray_p(dev), n, 0.0, k, hit_p(out, 16), cnt_p(cnt, 4), None) == 1       # ... and those alignments are enough
    o = out.cpu().numpy()
    assert o[1:].tobytes() == want_h.tobytes() and (o[0] == 0x5a5a5a5a).all()
    assert np.array_equal(cnt.cpu().numpy()[1:].view(np.uint32), want_c)


def test_after_a_move(gpu_lib, cases, monkeypatch):
    """RaylibAMD_SceneMoveTriangles on the soup: the device on the refitted trees equals the host oracle, which reads the moved triangles."""
    c = cases["soup"]
    rays = c.rays
    for tree in TREES_OF["soup"]:            # both trees on the device: the move refits them there
        _force(gpu_lib, monkeypatch, c.ses, tree)
        before = _dev(gpu_lib, c.ses, rays, 8)
    tris = c.ses.export_flat()[0]
    m = len(tris) // 3
    pos = np.ascontiguousarray(np.concatenate([tris["v0"][:m], tris["v1"][:m], tris["v2"][:m]], 1), np.float32)
    pos += np.random.RandomState(5).uniform(-0.3, 0.3, (m, 1, 3)).astype(np.float32).repeat(3, 1).reshape(m, 9)
    assert binding.move_triangles(gpu_lib, c.ses.scene, 0, pos) == 1
    try:
        want = _host(gpu_lib, c.ses, rays, 8)
        assert not _same(want, before), "the move must change answers"
        for tree in TREES_OF["soup"]:
            _force(gpu_lib, monkeypatch, c.ses, tree)
            got = _dev(gpu_lib, c.ses, rays, 8)
            assert _same(got, want), (tree, _first_difference(got[0], want[0]))
            assert _dev(gpu_lib, c.ses, rays, 8, count=False).tobytes() == want[0].tobytes(), tree
    finally:
        back = np.ascontiguousarray(np.concatenate([tris["v0"][:m], tris["v1"][:m], tris["v2"][:m]], 1), np.float32)
        assert binding.move_triangles(gpu_lib, c.ses.scene, 0, back) == 1
    monkeypatch.delenv("RAYLIB_QUERY_TREE")
    assert _same(_dev(gpu_lib, c.ses, rays, 8), _host(gpu_lib, c.ses, rays, 8))


def test_behind_a_multi_rank_frame_in_flight(gpu_lib, workdir):
    """tests/ray_query_all_rank_child.py under three ranks on one device: Raylib_Render, then at once the multi-hit query (host entry and device entry).  The
    query equals the oracle and reports its own stats, and the frame equals the one-rank frame of this process."""
    import ray_query_all_rank_child as child
    out = os.path.join(str(workdir), "ray_query_all_rank.npz")
    env = dict(os.environ)
    for k in ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_QUERY_TREE"):
        env.pop(k, None)
    env.update(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0")
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(workdir), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    one = child.run(gpu_lib, workdir)
    assert int(got["ranks"]) == 3 and int(one["ranks"]) == 1
    for key in ("hits_host_entry", "hits_device_entry", "counts_host_entry", "counts_device_entry"):
        assert got[key].tobytes() == got[key.split("_")[0] + "_oracle"].tobytes(), key
        assert got[key].tobytes() == np.ascontiguousarray(one[key]).view(np.uint32).tobytes(), key
    assert (got["counts_oracle"] >= 2).any()
    assert bool(helpers.same(got["frame"], one["frame"]).all()), "the frame in flight behind the query is not the one-rank frame"
