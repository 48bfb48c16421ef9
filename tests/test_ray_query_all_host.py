"""Ordered multi-hit ray queries (RaylibAMD_TraceRaysAll, include/raylib_amd.h statements M1 to M5) without a device: the host oracle
RaylibAMD_TraceRaysAllHost against peeling through the brute-force oracle of oracle/ (tests/ray_query_all_cases.py), a stack of coincident quads whose answers
are known exactly, the refusals, the planner's choice of tree, and the oracle's first record against the host restatement of the device walks.
tests/test_gpu_ray_query_all.py holds the device to the same truth and to this oracle byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from helpers import bits
import ray_query_all_cases as rc
import test_ray_query_host as qh

TREE_BVH2, TREE_WIDE8 = 1, 4
POOL8_MAXLEVELS = 16


@pytest.fixture(scope="module")
def cases(lib, oracle, workdir):
    S = rc.make_cases(lib, oracle, workdir, ["soup", "cutout8", "cornell", "stack"])
    yield S
    for c in S.values():
        oracle.scene_destroy(c.osc)
        c.ses.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


def _host(lib, ses, rays, k, count):
    from raylib_amd import binding
    return binding.trace_rays_all(lib, ses.scene, rays, k, count=count, host=True)


@pytest.mark.parametrize("name", ["soup", "cutout8", "cornell"])
def test_host_oracle_equals_the_peeled_brute_force(lib, cases, name):
    c, problems = cases[name], []
    assert (c.P.total >= 2).mean() > 0.05 and c.P.total.max() >= 3, "the rays must have something behind their first surface"
    for k in rc.MAX_HITS:
        hits, counts = _host(lib, c.ses, c.rays, k, True)
        rc.check(name + " with count", c.rays, c.tris, c.P, k, hits, counts, problems)
        plain = _host(lib, c.ses, c.rays, k, False)
        assert plain.tobytes() == hits.tobytes(), (name, k, "the records depend on whether the count is asked for")
        rc.check(name, c.rays, c.tris, c.P, k, plain, None, problems)
    assert not problems, "\n".join(problems[:20])


def test_stack_of_coincident_quads(lib, cases):
    """t = 1, 2, 3, 4, 5 exactly; tie groups of 3 (6 on the diagonal) in ascending slot order; every maxHits cuts inside and between them."""
    c = cases["stack"]
    assert len(c.tris) == 30
    order = rc.tri_order(lib, c.ses)
    slot_of = np.zeros(30, np.int64); slot_of[order] = np.arange(30)
    diag = c.rays[:, 0] == c.rays[:, 1]
    assert diag.sum() == 7 and len(c.rays) == 49
    group = np.where(diag, 6, 3)
    assert np.array_equal(c.P.total, 5 * group) and not c.P.excused.any()
    problems = []
    for k in range(1, 17):
        hits, counts = _host(lib, c.ses, c.rays, k, True)
        rc.check("stack", c.rays, c.tris, c.P, k, hits, counts, problems)
        assert np.array_equal(counts, 5 * group), (k, counts)
        for i in range(len(c.rays)):
            nh = min(k, 5 * group[i])
            assert (hits["prim"][i, :nh] >= 0).all() and (hits["prim"][i, nh:] == -1).all()
            assert np.array_equal(hits["t"][i, :nh], (np.arange(nh) // group[i] + 1).astype(np.float32)), (k, i, hits["t"][i])
            slots = slot_of[hits["prim"][i, :nh]]
            for g in range(0, nh, group[i]):
                s = slots[g:g + group[i]]
                assert (np.diff(s) > 0).all(), (k, i, g, s)
            assert len(set(hits["prim"][i, :nh].tolist())) == nh
        assert _host(lib, c.ses, c.rays, k, False).tobytes() == hits.tobytes()
    assert not problems, "\n".join(problems[:20])


def test_first_record_is_the_walks_closest_hit(lib, cases):
    """hits[:, 0] of the oracle against WalkStackHost's outT over [tMin, FLT_MAX] (the device walks' host restatement, binary tree at its full stack)"""
    for name in ("soup", "cornell"):
        c = cases[name]
        r6 = np.ascontiguousarray(np.concatenate([c.rays[:, 0:3], c.rays[:, 4:7]], axis=1), np.float32)
        out_t = np.zeros(len(r6), np.float32)
        tmin = float(c.rays[0, 3])
        assert (c.rays[:, 3] == c.rays[0, 3]).all() and (c.rays[:, 7] == helpers.F32_MAX).all()
        assert lib.RaylibAMD_SceneWalkStackHost(c.ses.scene, 2, r6.ctypes.data_as(C.POINTER(C.c_float)), len(r6), tmin, 64, out_t.ctypes.data_as(C.POINTER(C.c_float)), None) == 1
        hits = _host(lib, c.ses, c.rays, 1, False)
        hit = hits["prim"][:, 0] >= 0
        assert np.array_equal(hit, np.isfinite(out_t)), name
        assert np.array_equal(bits(hits["t"][hit, 0]), bits(out_t[hit])), name
        assert hit.sum() > len(r6) // 10


def test_special_bounds_give_the_empty_set(lib, cases):
    c = cases["soup"]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for tmin, tmax in ((nan, helpers.F32_MAX), (0.0, nan), (nan, nan), (5.0, 1.0), (inf, inf), (0.0, -1.0)):
        hits, counts = _host(lib, c.ses, helpers.with_interval(c.rays, tmin, tmax), 4, True)
        assert (hits["prim"] == -1).all() and not hits.view(np.uint32)[..., [0, 2, 3]].any() and not counts.any(), (tmin, tmax)
    # tMin < 0 is read as +0
    a = _host(lib, c.ses, helpers.with_interval(c.rays, -np.inf, None), 4, True)
    b = _host(lib, c.ses, helpers.with_interval(c.rays, 0.0, None), 4, True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_record_layout_and_exports(lib):
    from raylib_amd import binding
    assert binding.MAX_HITS == 16
    for name in ("RaylibAMD_TraceRaysAll", "RaylibAMD_TraceRaysAllDevice", "RaylibAMD_TraceRaysAllHost", "RaylibAMD_PlanRayQueryAll", "RaylibAMD_SceneExportTriOrder"):
        assert name in binding.RAYLIB_AMD_H_EXPORTS and hasattr(lib, name)


def _entries(lib):
    return ((lib.RaylibAMD_TraceRaysAll, ()), (lib.RaylibAMD_TraceRaysAllDevice, (None,)), (lib.RaylibAMD_TraceRaysAllHost, ()))


def test_refusals_leave_the_outputs_untouched(lib, cases, workdir):
    """Statement M5, whether or not there is a device: every entry, nothing written.  (A BVH deeper than 64 levels cannot be had from the builder, whose own
    bound is 61 -- tests/stack_edges.py deepest_triangles --, so that refusal, which every query entry carries, is not reachable from here.)"""
    from raylib_amd import binding
    ses = cases["soup"].ses
    rays = np.ascontiguousarray(cases["soup"].rays[:4])
    rp = rays.ctypes.data_as(C.POINTER(binding.Ray))
    out = np.full(4 * 16 * 16, 0x5a, np.uint8)
    cnt = np.full(4, 0x5a5a5a5a, np.uint32)
    op = C.cast(C.c_void_p(out.ctypes.data), C.POINTER(binding.HitT))
    cp = cnt.ctypes.data_as(C.POINTER(C.c_uint32))
    mats = np.zeros(1, helpers.ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    spheres = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)], [])
    cubes = binding.ProceduralSession(lib, mats, [], [dict(minBounds=(1, 0, 0), maxBounds=(1.5, 0.5, 0.5), timeStartMove=0.0, velocity=(0.0, 0.0, 0.0), material=0)])
    try:
        for fn, extra in _entries(lib):
            assert fn(ses.scene, None, 4, 0.0, 4, op, cp, *extra) == 0
            assert fn(ses.scene, rp, 4, 0.0, 4, None, cp, *extra) == 0
            assert fn(ses.scene, rp, -1, 0.0, 4, op, cp, *extra) == 0
            for k in (0, -1, 17, 1 << 20):
                assert fn(ses.scene, rp, 4, 0.0, k, op, cp, *extra) == 0
            for t in (float("nan"), float("inf"), float("-inf")):
                assert fn(ses.scene, rp, 4, t, 4, op, cp, *extra) == 0
            assert fn(None, rp, 4, 0.0, 4, op, cp, *extra) == 0
            unfinished = lib.Raylib_CreateScene()
            assert fn(unfinished, rp, 4, 0.0, 4, op, cp, *extra) == 0
            lib.Raylib_DestroyScene(unfinished)
            assert fn(spheres.scene, rp, 4, 0.0, 4, op, cp, *extra) == 0
            assert fn(cubes.scene, rp, 4, 0.0, 4, op, cp, *extra) == 0
            assert fn(ses.scene, rp, (1 << 31) - 1, 0.0, 2, op, cp, *extra) == 0          # n * maxHits above 2^31 - 1
            assert fn(ses.scene, rp, 134217728, 0.0, 16, op, cp, *extra) == 0             # = 2^31 exactly
        assert (out == 0x5a).all() and (cnt == 0x5a5a5a5a).all()
        # n == 0 returns 1 where nothing else stands in the way (the host entry needs no device), and writes nothing
        assert lib.RaylibAMD_TraceRaysAllHost(ses.scene, None, 0, 0.0, 4, None, None) == 1
        assert lib.RaylibAMD_TraceRaysAllHost(ses.scene, rp, 0, 0.0, 4, op, cp) == 1
        assert (out == 0x5a).all() and (cnt == 0x5a5a5a5a).all()
        with pytest.raises(RuntimeError):
            binding.trace_rays_all(lib, ses.scene, rays, 17, host=True)
    finally:
        spheres.close(); cubes.close()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-device path: this machine may have a GPU")
def test_without_a_device_the_plain_and_device_entries_return_0(lib, cases):
    from raylib_amd import binding
    ses = cases["soup"].ses
    rays = np.ascontiguousarray(cases["soup"].rays[:4])
    rp = rays.ctypes.data_as(C.POINTER(binding.Ray))
    out = np.full(4 * 4 * 16, 0x5a, np.uint8)
    op = C.cast(C.c_void_p(out.ctypes.data), C.POINTER(binding.HitT))
    assert lib.RaylibAMD_TraceRaysAll(ses.scene, rp, 4, 0.0, 4, op, None) == 0
    assert lib.RaylibAMD_TraceRaysAllDevice(ses.scene, rp, 4, 0.0, 4, op, None, None) == 0
    assert lib.RaylibAMD_TraceRaysAll(ses.scene, rp, 0, 0.0, 4, op, None) == 0
    assert (out == 0x5a).all()
    with pytest.raises(RuntimeError):
        binding.trace_rays_all(lib, ses.scene, rays, 4)
    assert binding.trace_rays_all(lib, ses.scene, rays, 4, host=True).shape == (4, 4)


def test_plan(lib, cases, workdir, monkeypatch):
    """The tree chosen (8-wide, else binary: no grid-4 instance), RAYLIB_QUERY_TREE honoured, the 64-entry stack for a BVH deeper than 32 levels, 0 for what M5
    refuses.  (-1, a BVH deeper than 64 levels, is not reachable: the builder stops at 61.)"""
    from raylib_amd import binding

    def plan(ses, k=4, count=False):
        r, p = binding.plan_ray_query_all(lib, ses.scene, k, count)
        assert r == 1, r
        return p

    soup, cornell = cases["soup"].ses, cases["cornell"].ses
    b = qh._bvh(lib, soup)
    assert b["has8"] and b["levels8"] <= POOL8_MAXLEVELS and b["depth"] <= 32, b
    for k in (1, 16):
        for count in (False, True):
            p = plan(soup, k, count)
            assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"], p["prims"], p["early"]) == (TREE_WIDE8, 8, 80, 2 * POOL8_MAXLEVELS, 0, 0), p
    assert not qh._bvh(lib, cornell)["has8"]
    p = plan(cornell)
    assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"]) == (TREE_BVH2, 2, 64, 32), p      # PlanRayQuery would take the grid-4 tree here
    for v, want in (("2", TREE_BVH2), ("4", TREE_BVH2), ("8", TREE_WIDE8), ("5", TREE_WIDE8)):
        monkeypatch.setenv("RAYLIB_QUERY_TREE", v)
        assert plan(soup)["tree"] == want, v
        assert plan(cornell)["tree"] == TREE_BVH2
    monkeypatch.delenv("RAYLIB_QUERY_TREE")
    d = os.path.join(str(workdir), "ray_query_all_plan"); os.makedirs(d, exist_ok=True)
    deep = binding.SceneSession(lib, qh._write_soup(os.path.join(d, "deep.obj"), 1000, 72), (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    try:
        b = qh._bvh(lib, deep)
        assert 32 < b["depth"] <= 64 and b["levels8"] <= POOL8_MAXLEVELS, b
        assert plan(deep)["tree"] == TREE_WIDE8
        monkeypatch.setenv("RAYLIB_QUERY_TREE", "2")
        assert (plan(deep)["tree"], plan(deep)["stack"]) == (TREE_BVH2, 64)
        monkeypatch.delenv("RAYLIB_QUERY_TREE")
        q = binding.QueryPlan()
        for k in (0, 17, -3):
            assert lib.RaylibAMD_PlanRayQueryAll(soup.scene, k, 0, C.byref(q)) == 0
        assert lib.RaylibAMD_PlanRayQueryAll(soup.scene, 4, 0, None) == 0
        assert lib.RaylibAMD_PlanRayQueryAll(None, 4, 0, C.byref(q)) == 0
        unfinished = lib.Raylib_CreateScene()
        assert lib.RaylibAMD_PlanRayQueryAll(unfinished, 4, 0, C.byref(q)) == 0
        lib.Raylib_DestroyScene(unfinished)
    finally:
        deep.close()
