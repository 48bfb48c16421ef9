"""The adaptive gather on the device (RaylibAMD_GatherAdaptive, include/raylib_amd.h statements A1 to A5).  The per-sample keys come from the route of
tests/test_gpu_gather.py -- the NumPy direction with the device's sincos, RaylibAMD_TraceRadiance along it, the NumPy product --, the decision from the NumPy
restatement (tests/gather_adaptive_cases.py) and from the host oracle, and the result from RaylibAMD_Gather at the count a point stopped with: every comparison
is bit for bit, on every point.  Cap 24, passes of 4, minSamples 4."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch    # before the library is loaded: the device entries take torch's tensors, and both must run on one HIP runtime

import helpers
import radiance_cases as rc
import gather_cases as gc
import gather_adaptive_cases as ga
import lightmap_cases as lc

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(helpers.ROOT, "software-raytracing_amd", "csrc")
with open(os.path.join(_CSRC, "rl_kernels.h")) as _f:
    _text = _f.read()
    QUERY_CHUNK = int(re.search(r"^#define RL_QUERY_CHUNK (\d+)u$", _text, re.M).group(1))
    COMPACT_PER = int(re.search(r"^#define RL_GATHER_COMPACT_PER (\d+)$", _text, re.M).group(1))
    COMPACT_SCAN_BLOCK = int(re.search(r"^#define RL_GATHER_COMPACT_SCAN_BLOCK (\d+)$", _text, re.M).group(1))
with open(os.path.join(_CSRC, "rl_device.h")) as _f:
    RL_BLOCK = int(re.search(r"^#define RL_BLOCK (\d+)\b", _f.read(), re.M).group(1))
COMPACT_TILE = RL_BLOCK * COMPACT_PER
F = np.float32
# test_decision_and_result's scenes: those whose reference decision, at the threshold the test computes, spreads over at least three counts with the cap among them.
# On the Cornell room, on the cut-out scene under the sky and on the glass-and-sun scene every point has stopped by 12 or 16 samples at that threshold: y = lum /
# (1 + lum) is bounded, and where most points see the sky or a strong sun the errors after 8 samples lie within a factor of two of their median.  The spread needs
# a scene that is dim at most points and bright at a few: the microfacet room, whose light only some points see -- and, for the scene with a sun, that room under
# a sun so dim (DIM_SUN) that the rays which leave the room add little beside the lamp.
SCENES = ["pbr_maps", "pbr_maps_dim_sun"]
DIM_SUN = (0.05, 0.05, 0.05)
OTHER = "cutout_sky"          # the scene of the tests that need no such spread
KINDS = [gc.IRRADIANCE, gc.SH9]
MIN_POINTS = 2 * QUERY_CHUNK + 2
CAP, PASS, MIN_SAMPLES = 24, 4, 4
CHILD_KILL_SECONDS = 300     # a kill limit; the child takes seconds


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    eq = helpers.same(got, want).reshape(len(got), -1).all(-1)
    assert eq.all(), "%s: %d of %d records differ (first at %d: %s against %s)" % (what, (~eq).sum(), len(eq), np.nonzero(~eq)[0][0],
                                                                                   got[~eq][0].tolist(), want[~eq][0].tolist())


def _stats(lib):
    from raylib_amd import binding
    st = binding.Stats()
    lib.RaylibAMD_GetLastStats(C.byref(st))
    return st


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    monkeypatch.delenv("RAYLIB_GATHER_BATCH", raising=False)


def surface_points(lib, ses):
    """tests/test_gpu_gather.py `cases`: the surface points a 16 x 12 frame of the session's camera rays meets, with the hits' normals, repeated on further streams up
    to MIN_POINTS points -- a wave's and a chunk's tails."""
    from raylib_amd import binding
    rays = rc.frame_rays(lib, ses, 16, 12)
    hits = binding.trace_rays(lib, ses.scene, helpers.rays8(rays[:, 0:3], rays[:, 4:7]), binding.QUERY_SURFACE)
    ok = hits["hit"] != 0
    assert ok.sum() >= 32, int(ok.sum())
    pos, nrm, time = hits["p"][ok], hits["n"][ok], rays[ok, 3]
    reps = -(-MIN_POINTS // len(pos))
    pts = gc.points(np.tile(pos, (reps, 1)), np.tile(nrm, (reps, 1)), np.tile(time, reps))
    assert len(pts) >= MIN_POINTS and np.isfinite(pts[:, :7]).all()
    return np.ascontiguousarray(pts)


@pytest.fixture(scope="module")
def cases(gpu_lib, sessions, workdir):
    from raylib_amd import binding
    obj, c = helpers.build_case("pbr_maps", workdir)
    sunny = binding.SceneSession(gpu_lib, obj, c["origin"], c["look_at"], c["fov"], c["aspect"], sun=DIM_SUN, sun_dir=helpers.CASES["cutout_sky"]["sun_dir"],
                                 aperture=c["aperture"], focal=c["focal"], shutter=c["shutter"])
    ses = {"pbr_maps": sessions["pbr_maps"], "pbr_maps_dim_sun": sunny, OTHER: sessions[OTHER]}
    yield {name: (v, surface_points(gpu_lib, v)) for name, v in ses.items()}
    sunny.close()


@pytest.fixture(scope="module")
def reference(gpu_lib, cases):
    """(name, kind) -> dict(keys (n, CAP, 3): statement A2's key of every sample; rays (n-point calls' ray counts are not per point, so:) a function
    rays_of(live, s) -> the rays RaylibAMD_TraceRadiance traces for sample s of the points `live`).  Computed once per key and shared, never changed."""
    from raylib_amd import binding
    sincos = gc.device_sincos(gpu_lib)
    seed = gpu_lib.RaylibAMD_GetSeed()
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            ses, pts = cases[name]
            keys = np.zeros((len(pts), CAP, 3), F)
            wis = []
            for s in range(CAP):
                wi = gc.directions(seed, pts, kind, s, 0, sincos)
                L = binding.trace_radiance(gpu_lib, ses.scene, gc.path_rays(pts, wi), sample_first=s, sample_count=1, skip_draws=2)
                keys[:, s] = gc.sample_values(L, pts, wi, kind) if kind == gc.IRRADIANCE else L[:, :3]      # SH9: L itself, not its products with Y_j
                wis.append(wi)
            keys.setflags(write=False)
            ray_cache = {}

            def rays_of(live, s):
                k = (live.tobytes(), s)
                if k not in ray_cache:
                    binding.trace_radiance(gpu_lib, ses.scene, gc.path_rays(pts[live], wis[s][live]), sample_first=s, sample_count=1, skip_draws=2)
                    ray_cache[k] = int(_stats(gpu_lib).rays)
                return ray_cache[k]
            cache[(name, kind)] = dict(keys=keys, rays_of=rays_of)
        return cache[(name, kind)]
    return get


def median_threshold(keys):
    """The midpoint between two distinct neighbouring errors after 8 samples, at the median: about half of the points may stop by then."""
    s1, s2 = ga.moments(keys[:, :8])
    e = ga.error(s1[:, 7], s2[:, 7], 8)
    u = np.unique(e[np.isfinite(e)])
    assert len(u) >= 2, u
    i = max(1, len(u) // 2)
    t = F((np.float64(u[i - 1]) + np.float64(u[i])) / 2)
    assert u[i - 1] <= t <= u[i] and t > 0
    return float(t)


def _adaptive(lib, ses, pts, kind, threshold, **kw):
    from raylib_amd import binding
    kw = dict(dict(min_samples=MIN_SAMPLES, pass_samples=PASS, sample_count=CAP), **kw)
    return binding.gather_adaptive(lib, ses.scene, pts, kind, threshold, **kw)


def _check_result(lib, ses, pts, kind, values, counts, what, **gather_kw):
    """A4: for every distinct n, the points that stopped with n hold RaylibAMD_Gather's bits at sampleCount = n on the same records."""
    from raylib_amd import binding
    for n in np.unique(counts):
        sel = counts == n
        want = binding.gather(lib, ses.scene, np.ascontiguousarray(pts[sel]), kind, sample_count=int(n), **gather_kw)
        _same_bits(values[sel], want, "%s: the %d points that stopped with %d samples" % (what, sel.sum(), n))


# ---- 1. decision and result ----
@pytest.mark.parametrize("kind", KINDS, ids=["irradiance", "sh9"])
@pytest.mark.parametrize("name", SCENES)
def test_decision_and_result(gpu_lib, cases, reference, name, kind):
    from raylib_amd import binding
    ses, pts = cases[name]
    keys = reference(name, kind)["keys"]
    threshold = median_threshold(keys)
    want = ga.decide(keys, threshold, MIN_SAMPLES, PASS)
    distinct = set(want.tolist())
    print("%s kind %d: threshold %.9g, reference counts %s" % (name, kind, threshold, {n: int((want == n).sum()) for n in sorted(distinct)}))
    assert len(distinct) >= 3 and CAP in distinct and min(distinct) < CAP, distinct          # the reference decision itself is not trivial
    host = binding.gather_adaptive_decide_host(gpu_lib, keys, threshold, MIN_SAMPLES, PASS)
    assert host.tolist() == want.tolist()
    values, counts = _adaptive(gpu_lib, ses, pts, kind, threshold)
    assert counts.dtype == np.uint32 and counts.tolist() == want.tolist(), np.nonzero(counts != want)[0][:8]
    _check_result(gpu_lib, ses, pts, kind, values, counts, "%s kind %d" % (name, kind))
    if kind == gc.IRRADIANCE:
        assert (values[:, 3] == 1).all()
    assert (values[:, :3] != 0).any()
    # outSamples may be null: the values are the same
    v2, none = _adaptive(gpu_lib, ses, pts, kind, threshold, want_samples=False)
    assert none is None
    _same_bits(v2, values, "without outSamples")


# ---- 2. degenerate settings ----
@pytest.mark.parametrize("kind", KINDS, ids=["irradiance", "sh9"])
def test_degenerate_settings_are_the_plain_gather(gpu_lib, cases, reference, kind):
    from raylib_amd import binding
    ses, pts = cases["cutout_sky"]
    threshold = median_threshold(reference("cutout_sky", kind)["keys"])
    plain = {n: binding.gather(gpu_lib, ses.scene, pts, kind, sample_count=n) for n in (23, 24)}
    for what, kw, t, n in (("threshold 0", {}, 0.0, 24), ("minSamples 25", dict(min_samples=25), threshold, 24), ("passSamples 24", dict(pass_samples=24), threshold, 24),
                           ("passSamples 32", dict(pass_samples=32), threshold, 24), ("cap 23, threshold 0", dict(sample_count=23), 0.0, 23),
                           ("cap 23, minSamples 25", dict(sample_count=23, min_samples=25), threshold, 23)):
        values, counts = _adaptive(gpu_lib, ses, pts, kind, t, **kw)
        assert (counts == n).all(), (what, np.unique(counts))
        _same_bits(values, plain[n], what)
        assert _stats(gpu_lib).cameraSamples == n * len(pts)
    # cap 23 in passes of 4 with a live rule, on the scene where points reach the cap: the last pass is 3 samples short, and a point that goes to the end holds the
    # plain gather's 23 samples
    ses, pts = cases["pbr_maps"]
    keys = reference("pbr_maps", kind)["keys"]
    threshold = median_threshold(keys)
    values, counts = _adaptive(gpu_lib, ses, pts, kind, threshold, sample_count=23)
    want = ga.decide(keys, threshold, MIN_SAMPLES, PASS, cap=23)
    assert counts.tolist() == want.tolist() and 23 in set(counts.tolist())
    _check_result(gpu_lib, ses, pts, kind, values, counts, "cap 23")


# ---- 3. independence ----
@pytest.mark.parametrize("kind", KINDS, ids=["irradiance", "sh9"])
def test_independence(gpu_lib, cases, reference, monkeypatch, kind):
    """A5: RAYLIB_GATHER_BATCH of two samples of every point cuts the first pass (4 samples of every point) into two sample ranges, 37 and 1 cut it into point
    ranges of one sample each -- and the later passes, of fewer points, otherwise; the trees; the points in another order, and half of them alone."""
    ses, pts = cases["cutout_sky"]
    assert len(pts) > 37
    threshold = median_threshold(reference("cutout_sky", kind)["keys"])
    values, counts = _adaptive(gpu_lib, ses, pts, kind, threshold)
    passes = _stats(gpu_lib).traceLaunches                            # one launch per pass that ran
    assert passes == len(ga.pass_counts(int(counts.max()), PASS))
    for batch in (2 * len(pts), 37, 1):
        monkeypatch.setenv("RAYLIB_GATHER_BATCH", str(batch))
        v, c = _adaptive(gpu_lib, ses, pts, kind, threshold)
        assert _stats(gpu_lib).traceLaunches > passes
        assert c.tolist() == counts.tolist(), batch
        _same_bits(v, values, "RAYLIB_GATHER_BATCH=%d" % batch)
    monkeypatch.delenv("RAYLIB_GATHER_BATCH")
    for tree in ("2", "4"):
        monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
        v, c = _adaptive(gpu_lib, ses, pts, kind, threshold)
        assert c.tolist() == counts.tolist(), tree
        _same_bits(v, values, "RAYLIB_QUERY_TREE=%s" % tree)
    monkeypatch.delenv("RAYLIB_QUERY_TREE")
    perm = np.random.RandomState(5).permutation(len(pts))
    v, c = _adaptive(gpu_lib, ses, np.ascontiguousarray(pts[perm]), kind, threshold)
    assert c.tolist() == counts[perm].tolist()
    _same_bits(v, values[perm], "the points permuted")
    half = np.sort(perm[:len(pts) // 2])
    v, c = _adaptive(gpu_lib, ses, np.ascontiguousarray(pts[half]), kind, threshold)
    assert c.tolist() == counts[half].tolist()
    _same_bits(v, values[half], "half of the points alone")


# ---- 4. the compaction ----
def _compact_case(lib, num_live, mode, seed):
    from raylib_amd import binding
    rng = np.random.RandomState(seed)
    num_points = num_live + 7
    live = np.sort(rng.permutation(num_points)[:num_live]).astype(np.uint32)
    stopped = {"random": rng.choice(np.array([0, 0, 1, 200], np.uint8), num_points), "none": np.zeros(num_points, np.uint8),
               "all": np.ones(num_points, np.uint8)}[mode]
    if mode == "none":
        stopped[np.setdiff1d(np.arange(num_points), live)] = 1          # (points outside the list do not matter)
    points = rng.randint(0, 2 ** 32, (num_points, 8), dtype=np.uint64).astype(np.uint32).view(F)
    r, out_live, out_points, count = binding.gather_compact_test(lib, live, stopped, points)
    assert r == 1
    want = live[stopped[live] == 0]
    assert count[0] == len(want), (num_live, mode, count[0], len(want))
    assert np.array_equal(out_live[:len(want)], want)
    assert np.array_equal(out_points[:len(want)], points.view(np.uint32)[want])
    assert (out_live[len(want):] == binding.COMPACT_SENTINEL).all() and (out_points[len(want):] == binding.COMPACT_SENTINEL).all()      # nothing past the count


@pytest.mark.parametrize("num_live", [1, 63, 64, 65, RL_BLOCK - 1, RL_BLOCK, RL_BLOCK + 1, COMPACT_TILE - 1, COMPACT_TILE, COMPACT_TILE + 1, 100003])
def test_compaction(gpu_lib, num_live):
    for k, mode in enumerate(("random", "none", "all")):
        _compact_case(gpu_lib, num_live, mode, num_live * 3 + k)


def test_compaction_past_one_round_of_the_tile_scan(gpu_lib):
    """More tiles than the scan's workgroup has threads: its loop over the tiles' counts runs a second round, carrying the first's total."""
    _compact_case(gpu_lib, COMPACT_SCAN_BLOCK * COMPACT_TILE + COMPACT_TILE + 5, "random", 77)


def test_compaction_refusals(gpu_lib):
    from raylib_amd import binding
    pts = np.zeros((4, 8), F)
    for live in ([0, 2, 2], [2, 0, 3], [0, 1, 4], [0, 1, 2, 3, 3]):
        r, out_live, out_points, count = binding.gather_compact_test(gpu_lib, np.array(live, np.uint32), np.zeros(4, np.uint8), pts)
        assert r == 0 and (out_live == binding.COMPACT_SENTINEL).all() and (out_points == binding.COMPACT_SENTINEL).all() and count[0] == binding.COMPACT_SENTINEL
    r, out_live, out_points, count = binding.gather_compact_test(gpu_lib, np.zeros(0, np.uint32), np.zeros(4, np.uint8), pts)       # an empty list: count 0
    assert r == 1 and count[0] == 0 and (out_live == binding.COMPACT_SENTINEL).all()


# ---- 5. the device entry ----
def test_device_entry(gpu_lib, cases, reference):
    from raylib_amd import binding
    ses, pts = cases["cutout_sky"]
    n = len(pts)
    dev = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    for kind in KINDS:
        threshold = median_threshold(reference("cutout_sky", kind)["keys"])
        values, counts = _adaptive(gpu_lib, ses, pts, kind, threshold)
        before = _stats(gpu_lib).as_dict()
        assert before["cameraSamples"] == counts.sum()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            v, c = _adaptive(gpu_lib, ses, dev, kind, threshold)
        # the call returned with the last pass complete: no wait here
        assert v.cpu().numpy().tobytes() == values.tobytes() and c.cpu().numpy().astype(np.uint32).tolist() == counts.tolist()
        assert _stats(gpu_lib).as_dict() == before                       # a caller's stream: the stats of the call before are left alone
        v, c = _adaptive(gpu_lib, ses, dev, kind, threshold)             # torch's default stream: the library's stream, synchronous, with stats
        assert v.cpu().numpy().tobytes() == values.tobytes() and c.cpu().numpy().astype(np.uint32).tolist() == counts.tolist()
        assert _stats(gpu_lib).cameraSamples == counts.sum()
    # refusals: outSamples misaligned or in host memory, with nothing written
    out = torch.full((n * 4,), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((n + 2,), 7, dtype=torch.int32, device="cuda")
    host_cnt = np.full(n, 7, np.uint32)
    torch.cuda.synchronize()
    prm = binding.GatherParams(gc.IRRADIANCE, 5, 1e-4, 0, CAP, 0, 0.0, 1.0)
    ada = binding.GatherAdaptiveParams(0.01, MIN_SAMPLES, PASS)
    fn = gpu_lib.RaylibAMD_GatherAdaptiveDevice
    pp = C.cast(C.c_void_p(dev.data_ptr()), C.POINTER(binding.GatherPoint))
    op = C.cast(C.c_void_p(out.data_ptr()), C.POINTER(C.c_float))
    u32 = C.POINTER(C.c_uint32)
    assert fn(ses.scene, C.byref(prm), C.byref(ada), pp, n, op, C.cast(C.c_void_p(cnt.data_ptr() + 2), u32), None) == 0
    assert fn(ses.scene, C.byref(prm), C.byref(ada), pp, n, op, host_cnt.ctypes.data_as(u32), None) == 0
    assert fn(ses.scene, C.byref(prm), C.byref(ada), pp, n, C.cast(C.c_void_p(out.data_ptr() + 4), C.POINTER(C.c_float)), C.cast(C.c_void_p(cnt.data_ptr()), u32), None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all() and (cnt.cpu().numpy() == 7).all() and (host_cnt == 7).all()
    assert fn(ses.scene, C.byref(prm), C.byref(ada), pp, n, op, C.cast(C.c_void_p(cnt.data_ptr() + 4), u32), None) == 1      # (4-byte aligned is enough)
    want_v, want_c = _adaptive(gpu_lib, ses, pts, gc.IRRADIANCE, 0.01)
    assert out.cpu().numpy().tobytes() == want_v.tobytes() and cnt[1:1 + n].cpu().numpy().astype(np.uint32).tolist() == want_c.tolist()


# ---- 6. the stats ----
@pytest.mark.parametrize("batch", [None, 37])
def test_stats(gpu_lib, cases, reference, monkeypatch, batch):
    from raylib_amd import binding
    name = "cutout_sky"
    ses, pts = cases[name]
    for kind in KINDS:
        ref = reference(name, kind)
        threshold = median_threshold(ref["keys"])
        want = ga.decide(ref["keys"], threshold, MIN_SAMPLES, PASS)
        # the reference route's rays over the samples actually taken: pass by pass, the live points' samples (before the batch is set: the route is one launch each)
        rays, live_sizes = 0, []
        for p, n_p in enumerate(ga.pass_counts(CAP, PASS)):
            live = np.nonzero(want > p * PASS)[0]
            if not len(live):
                break
            live_sizes.append((len(live), n_p - p * PASS))
            rays += sum(ref["rays_of"](live, s) for s in range(p * PASS, n_p))
        if batch:
            monkeypatch.setenv("RAYLIB_GATHER_BATCH", str(batch))
        values, counts = _adaptive(gpu_lib, ses, pts, kind, threshold)
        st = _stats(gpu_lib)
        launches = sum(binding.plan_gather_cut(gpu_lib, kind, m, take)["launches"] for m, take in live_sizes)
        monkeypatch.delenv("RAYLIB_GATHER_BATCH", raising=False)
        assert counts.tolist() == want.tolist()
        assert st.cameraSamples == counts.sum() == sum(m * take for m, take in live_sizes), st.as_dict()
        assert st.rays == rays, (st.rays, rays)
        assert st.traceLaunches == launches and (launches > len(live_sizes)) == bool(batch), (st.traceLaunches, launches, live_sizes)
        assert st.ranks == 1 and st.nodesVisited > 0 and st.trisTested > 0 and st.shadedHits > 0
        assert 0 < st.traceKernelMs <= st.kernelMs <= st.wallMs


@pytest.mark.parametrize("count", [33, 41])
def test_timing_of_many_launches(gpu_lib, cases, monkeypatch, count):
    """One pass of `count` samples at threshold 0, cut by RAYLIB_GATHER_BATCH=1 into 100 x count launches.  Up to RL_GATHER_TIMED = 4096 of them the trace launches
    are timed apart, and their sum lies below the whole call's time; a call that goes past the limit reports the whole span as its trace time."""
    ses, pts = cases[OTHER]
    pts = np.ascontiguousarray(pts[:100])
    want_v, want_c = _adaptive(gpu_lib, ses, pts, gc.IRRADIANCE, 0.0, pass_samples=count, sample_count=count)
    assert _stats(gpu_lib).traceLaunches == 1 and (want_c == count).all()
    monkeypatch.setenv("RAYLIB_GATHER_BATCH", "1")
    values, counts = _adaptive(gpu_lib, ses, pts, gc.IRRADIANCE, 0.0, pass_samples=count, sample_count=count)
    st = _stats(gpu_lib)
    print("count %d: traceLaunches %d, traceKernelMs %.6f, kernelMs %.6f, wallMs %.6f" % (count, st.traceLaunches, st.traceKernelMs, st.kernelMs, st.wallMs))
    assert counts.tolist() == want_c.tolist()
    _same_bits(values, want_v, "%d samples, one pair per launch" % count)
    assert st.traceLaunches == 100 * count and st.cameraSamples == 100 * count
    if 100 * count <= 4096:
        assert 0 < st.traceKernelMs < st.kernelMs <= st.wallMs
    else:
        assert st.traceKernelMs == st.kernelMs > 0


# ---- 7. the lightmap ----
LM_W = LM_H = 32


@pytest.mark.parametrize("kind", KINDS, ids=["irradiance", "sh9"])
def test_lightmap(gpu_lib, sessions, kind):
    """A 32 x 32 atlas of the Cornell room's floor and back wall (triangles 0 .. 5: floor, ceiling, back wall; the ceiling's pair gets a degenerate uv and is skipped)."""
    from raylib_amd import binding
    ses = sessions["cornell"]
    uv = lc.grid_uv(6)
    uv[2:4] = 0.0
    pts, tex, n = binding.lightmap_points(gpu_lib, ses.scene, LM_W, LM_H, uv, tri_first=0, tri_count=6)
    assert n == len(tex) and 200 < n < LM_W * LM_H
    # y lies in [0, 1), so a point's error after n samples is at most 1 / (2 sqrt(n - 1)): 0.29 at 4 samples, 0.10 at 24.  0.02 lies inside that range; that it
    # splits the texels is asserted on the counts below, and the decision itself is test_decision_and_result's subject
    threshold = 0.02
    values, counts = binding.gather_adaptive(gpu_lib, ses.scene, pts, kind, threshold, MIN_SAMPLES, PASS, sample_count=CAP)
    assert len(np.unique(counts)) >= 2
    cov_want = np.zeros(LM_W * LM_H, np.uint8); cov_want[tex] = 1
    cnt_want = np.zeros(LM_W * LM_H, np.uint32); cnt_want[tex] = counts
    atlas, cov, cnt = binding.bake_lightmap_adaptive(gpu_lib, ses.scene, LM_W, LM_H, threshold, MIN_SAMPLES, PASS, uv, kind, tri_first=0, tri_count=6, sample_count=CAP)
    st = _stats(gpu_lib)
    assert st.pixels == n and st.cameraSamples == counts.sum() and st.kernelMs > 0
    want_atlas, _ = lc.scatter(values, tex, LM_W, LM_H)
    assert np.array_equal(cov.reshape(-1), cov_want) and np.array_equal(cnt.reshape(-1), cnt_want)
    assert lc.same_bits(atlas, want_atlas)
    assert (helpers.bits(atlas.reshape(LM_W * LM_H, -1)[cov_want == 0]) == 0).all()                    # +0 where nothing is covered
    # dilate 2: the values and the coverage are dilated, the counts are not
    atlas2, cov2, cnt2 = binding.bake_lightmap_adaptive(gpu_lib, ses.scene, LM_W, LM_H, threshold, MIN_SAMPLES, PASS, uv, kind, tri_first=0, tri_count=6, dilate=2,
                                                        sample_count=CAP)
    want2, want_cov2 = lc.dilate(want_atlas, cov_want.reshape(LM_H, LM_W), 2)
    assert np.array_equal(cov2, want_cov2) and (cov2 > 1).any() and lc.same_bits(atlas2, want2)
    assert np.array_equal(cnt2.reshape(-1), cnt_want)
    # outSamples may be null
    atlas3, cov3, none = binding.bake_lightmap_adaptive(gpu_lib, ses.scene, LM_W, LM_H, threshold, MIN_SAMPLES, PASS, uv, kind, tri_first=0, tri_count=6,
                                                        sample_count=CAP, want_samples=False)
    assert none is None and lc.same_bits(atlas3, atlas) and np.array_equal(cov3, cov)
    # the device entry on a stream of torch's
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a4, c4, n4 = binding.bake_lightmap_adaptive(gpu_lib, ses.scene, LM_W, LM_H, threshold, MIN_SAMPLES, PASS, torch.from_numpy(uv).cuda(), kind, tri_first=0, tri_count=6,
                                                    sample_count=CAP)
    s.synchronize()
    assert lc.same_bits(a4.cpu().numpy(), atlas) and np.array_equal(c4.cpu().numpy(), cov) and np.array_equal(n4.cpu().numpy().astype(np.uint32), cnt)
    # the intended pipeline: the raw adaptive atlas through RaylibAMD_FilterLightmap is the host filter on it, scattered
    filt = (3, 0.8, 0.5, 0.05)
    got, got_cov = binding.filter_lightmap(gpu_lib, ses.scene, LM_W, LM_H, atlas, filt, uv, kind, tri_first=0, tri_count=6)
    host_pts, host_tex, _ = binding.lightmap_points(gpu_lib, ses.scene, LM_W, LM_H, uv, tri_first=0, tri_count=6, host=True)
    assert np.array_equal(host_tex, tex)
    filtered = binding.filter_lightmap_host(gpu_lib, LM_W, LM_H, kind, filt, host_pts, host_tex, values)
    want_f, want_f_cov = lc.scatter(filtered, tex, LM_W, LM_H)
    assert np.array_equal(got_cov, want_f_cov) and lc.same_bits(got, want_f)


# ---- 8. behind a multi-rank frame in flight ----
def test_behind_a_multi_rank_frame(gpu_lib, cases, reference, workdir):
    """A fresh process with two ranks on the one device: gather_adaptive straight behind a Raylib_Render whose frame is still in flight gives the one-rank bits,
    reports its own stats, and leaves the frame alone."""
    ses, pts = cases["cutout_sky"]
    kind = gc.IRRADIANCE
    threshold = median_threshold(reference("cutout_sky", kind)["keys"])
    values, counts = _adaptive(gpu_lib, ses, pts, kind, threshold)
    src = os.path.join(str(workdir), "gather_adaptive_child_in.npz")
    dst = os.path.join(str(workdir), "gather_adaptive_child_out.npz")
    np.savez(src, points=pts, threshold=np.float64(threshold), kind=kind, cap=CAP, pass_samples=PASS, min_samples=MIN_SAMPLES)
    env = dict(os.environ)
    for k in ("RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_DEVICE", "RAYLIB_POOL", "RAYLIB_LIB", "RAYLIB_GATHER_BATCH", "RAYLIB_QUERY_TREE"):
        env.pop(k, None)
    env.update(RAYLIB_NUM_GPUS="2", RAYLIB_GPU_MAP="0,0")
    cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gather_adaptive_child.py"), str(workdir), src, dst]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_KILL_SECONDS)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(dst)
    assert got["counts"].tolist() == counts.tolist()
    _same_bits(got["values"], values, "behind the frame in flight")
    ranks, camera_samples = got["stats"]
    assert ranks == 1 and camera_samples == counts.sum()                  # the gather's own numbers, not the frame's
    assert got["control_ranks"] == 2                                       # the two-rank path really ran
    assert got["frame_pixels_differing"] == 0
