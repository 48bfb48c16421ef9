"""The choice of the megakernel instance, its tree and its job layout (csrc/rl_plan.cc), through RaylibAMD_PlanRender: every row of the choice table and
every per-render switch of INTEGRATION.md, on the scenes the suite renders.  No device needed; tests/test_gpu_* check that a launch reports what the plan said --
the rows with the 64-deep stacks in tests/test_gpu_stack_edges.py, on the scenes of tests/stack_edges.py."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import scenes, ffi

TREE_NONE, TREE_BVH2, TREE_BOX4, TREE_GRID4, TREE_WIDE8 = range(5)
POOL_SHORT_LSTACK, POOL8_LSTACK, POOL8_MAXLEVELS, MAX_HEADS, BLOCK = 18, 16, 16, 8, 256
SWITCHES = ("RAYLIB_POOL", "RAYLIB_POOL_MIN_TRIS", "RAYLIB_POOL_SHORT_STACK", "RAYLIB_BVH4", "RAYLIB_BVH8", "RAYLIB_LDS_SCENE", "RAYLIB_LEAF_LIST",
            "RAYLIB_PLAIN_KERNEL", "RAYLIB_SAMPLE_BATCH", "RAYLIB_SAMPLE_BUFFER_GIB", "RAYLIB_JOB_CHUNK", "RAYLIB_JOB_HEADS", "RAYLIB_GUIDED",
            "RAYLIB_BLOCKS_PER_CU", "RAYLIB_CULL_CELLS")


def plan(lib, ses, w=64, h=64, spp=4, tmin=1e-4, mode=0, sky=False, cus=256, per_cu=4):
    from raylib_amd import binding
    st = binding.RendererSettings(w, h, spp, 5, tmin, mode)
    out = binding.RenderPlan()
    rc = lib.RaylibAMD_PlanRender(ses.scene, C.byref(st), int(sky), cus, per_cu, C.byref(out))
    assert rc == 1, rc
    return out.as_dict()


def _write_soup(path, n_soup, n_chain):
    """n_soup triangles of about the scene's size (rays expected to take many node steps), then a chain of n_chain triangles, each half the size of the
    last and next to it, which the SAH builder peels off a few at a time: a BVH2 as deep as the chain is long."""
    rng = np.random.RandomState(3)
    lines, k = ["o soup\n"], 0
    tris = [c + rng.uniform(-1.0, 1.0, (3, 3)) for c in rng.uniform(-1.0, 1.0, (n_soup, 3))]
    for j in range(1, n_chain + 1):
        c = 2.0 ** -j
        tris.append(np.array([[c, 0, 0], [c + c / 2, 0, 0], [c, c / 2, 0]]))
    for p in tris:
        for q in p:
            lines.append("v %.9g %.9g %.9g\n" % tuple(q))
        lines.append("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))
        k += 1
    with open(path, "w") as f:
        f.write("".join(lines))
    return path


def _bvh(lib, ses):
    n, d, s = C.c_uint32(), C.c_uint32(), C.c_float()
    lib.RaylibAMD_SceneBVHInfo(ses.scene, C.byref(n), C.byref(d), C.byref(s))
    n4, st4 = C.c_uint32(), C.c_uint32()
    lib.RaylibAMD_SceneBVH4Info(ses.scene, C.byref(n4), C.byref(st4))
    n8, lv, s4, s8 = C.c_uint32(0), C.c_uint32(0), C.c_float(0), C.c_float(0)
    lib.RaylibAMD_SceneBVH8Info(ses.scene, C.byref(n8), C.byref(lv), C.byref(s4), C.byref(s8))
    return dict(depth=d.value, stack4=st4.value, levels8=lv.value, steps4=s4.value)


@pytest.fixture(scope="module")
def plan_scenes(lib, workdir):
    from raylib_amd import binding
    d = os.path.join(str(workdir), "plan_host"); os.makedirs(d, exist_ok=True)

    def obj(name, path):
        return binding.SceneSession(lib, path, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    S = {}
    S["cornell"] = obj("cornell", scenes.cornell(os.path.join(d, "cornell.obj"))[0])
    S["cutout"] = obj("cutout", scenes.cutout(os.path.join(d, "cutout.obj"))[0])
    S["pbr_maps"] = obj("pbr_maps", scenes.pbr_maps(os.path.join(d, "pbr.obj"))[0])
    S["tess2"] = obj("tess2", scenes.cornell(os.path.join(d, "tess2.obj"), tess=2)[0])
    S["mid"] = obj("mid", scenes.cornell(os.path.join(d, "mid.obj"), tess=24, displace_fraction=0.2)[0])
    S["soup"] = obj("soup", _write_soup(os.path.join(d, "soup.obj"), 1000, 0))
    S["deep"] = obj("deep", _write_soup(os.path.join(d, "deep.obj"), 1000, 72))         # BVH2 deeper than 32
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    sph = [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0), dict(center=(1.0, 0.0, -1.0), radius=0.3, material=0)]
    S["spheres"] = binding.ProceduralSession(lib, mats, sph, ())
    yield S
    for s in S.values():
        s.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def test_default_choice_table(lib, plan_scenes):
    S = plan_scenes
    # Cornell: the leaf list, plain instance; with a sky image the general one; with rayTMin < 0 no leaf list (the scene in LDS, on its float boxes)
    p = plan(lib, S["cornell"])
    assert (p["poolK"], p["lds"], p["plain"], p["treeWidth"], p["tree"], p["stack"], p["pathsPerWave"]) == (0, 2, 1, 0, TREE_NONE, 16, 64), p
    assert p["eagerTree"] == TREE_NONE
    p = plan(lib, S["cornell"], sky=True)
    assert (p["lds"], p["plain"], p["treeWidth"]) == (2, 0, 0), p
    p = plan(lib, S["cornell"], tmin=-1e-4)
    assert (p["poolK"], p["lds"], p["plain"], p["treeWidth"], p["tree"]) == (0, 1, 0, 4, TREE_BOX4), p
    # textures / cut-outs: the general leaf-list instance
    for name in ("cutout", "pbr_maps"):
        p = plan(lib, S[name])
        assert (p["poolK"], p["lds"], p["plain"], p["treeWidth"]) == (0, 2, 0, 0), (name, p)
    # 144 triangles: above the LDS limit of 128 -- k_trace on the float boxes in global memory
    p = plan(lib, S["tess2"])
    assert (p["poolK"], p["lds"], p["tree"], p["treeWidth"], p["keepNodes4"], p["keepNodes4f"], p["nodeBytes"]) == (0, 0, TREE_BOX4, 4, 0, 1, 64), p
    # the 21 k-triangle room: the pool schedule (K = 2) on the 4-wide grid nodes, short stack; its grid goes to the device with the scene
    p = plan(lib, S["mid"])
    assert (p["poolK"], p["tree"], p["treeWidth"], p["lstack"], p["pathsPerWave"], p["nodeBytes"], p["eagerTree"]) == (2, TREE_GRID4, 4, POOL_SHORT_LSTACK, 128, 64, TREE_GRID4), p
    # rays expected to take many steps: the 8-wide tree, uploaded with the scene
    b = _bvh(lib, S["soup"])
    assert b["steps4"] >= 40 and b["levels8"] <= POOL8_MAXLEVELS and b["depth"] <= 32 and b["stack4"] <= 64, b
    p = plan(lib, S["soup"])
    assert (p["poolK"], p["tree"], p["treeWidth"], p["nodeBytes"], p["stack"], p["lstack"], p["eagerTree"]) == (2, TREE_WIDE8, 8, 80, 2 * POOL8_MAXLEVELS, POOL8_LSTACK, TREE_WIDE8), p
    # spheres / cubes: k_trace on the BVH2
    p = plan(lib, S["spheres"])
    assert (p["poolK"], p["prims"], p["tree"], p["treeWidth"], p["keepNodes4"], p["keepNodes4f"], p["lds"]) == (0, 1, TREE_BVH2, 2, 0, 0, 0), p
    # a debug render mode: k_aov on the BVH2
    p = plan(lib, S["mid"], mode=2)
    assert (p["pathTrace"], p["poolK"], p["treeWidth"], p["pathsPerWave"]) == (0, 0, 2, 64), p


def test_deep_scene_does_not_upload_a_tree_it_never_walks(lib, plan_scenes):
    """A scene whose rays are expected to take many steps on an 8-wide tree of few levels, but whose BVH2 is deeper than 32: the default plan is k_trace
    with the 64-deep stack, which walks no wide tree (its 4-wide stack need is above 64 as well), and no wide tree goes to the device with the scene."""
    S = plan_scenes
    b = _bvh(lib, S["deep"])
    assert b["depth"] > 32 and b["stack4"] > 64 and b["steps4"] >= 40 and b["levels8"] <= POOL8_MAXLEVELS, b
    p = plan(lib, S["deep"])
    assert (p["poolK"], p["stack"], p["tree"], p["treeWidth"]) == (0, 64, TREE_BVH2, 2), p
    assert p["eagerTree"] != TREE_WIDE8 and p["eagerTree"] == TREE_NONE, p


def test_every_switch_of_the_table(lib, plan_scenes, monkeypatch):
    S = plan_scenes

    def with_env(name, env, **kw):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            return plan(lib, S[name], **kw)
        finally:
            for k in env:
                monkeypatch.delenv(k)
    # RAYLIB_POOL / RAYLIB_POOL_MIN_TRIS
    p = with_env("mid", dict(RAYLIB_POOL="0"))
    assert p["poolK"] == 0 and p["pathsPerWave"] == 64 and p["lds"] == 0, p
    for k in (3, 4):
        p = with_env("mid", dict(RAYLIB_POOL=str(k)))
        assert (p["poolK"], p["tree"], p["treeWidth"], p["pathsPerWave"]) == (k, TREE_BVH2, 2, 64 * k), p
    assert with_env("mid", dict(RAYLIB_POOL="7"))["poolK"] == 0
    p = with_env("cornell", dict(RAYLIB_POOL="2"))
    assert (p["poolK"], p["tree"], p["treeWidth"], p["plain"]) == (2, TREE_GRID4, 4, 0), p
    assert with_env("spheres", dict(RAYLIB_POOL="2"))["poolK"] == 0   # (the pool schedule renders triangles only)
    assert with_env("mid", dict(RAYLIB_POOL_MIN_TRIS="100000"))["poolK"] == 0
    assert with_env("tess2", dict(RAYLIB_POOL_MIN_TRIS="100"))["poolK"] == 2
    # RAYLIB_POOL_SHORT_STACK: all 32 entries in LDS; on the BVH2 also the short stack and the test stack of 4 (scenes deeper than 16)
    p = with_env("mid", dict(RAYLIB_POOL_SHORT_STACK="0"))
    assert (p["tree"], p["lstack"], p["stack"]) == (TREE_GRID4, 32, 32) or (p["tree"], p["lstack"], p["stack"]) == (TREE_GRID4, 32, 64), p
    assert _bvh(lib, S["mid"])["depth"] > 16
    assert with_env("mid", dict(RAYLIB_BVH4="0", RAYLIB_POOL_SHORT_STACK="0"))["lstack"] == 32
    assert with_env("mid", dict(RAYLIB_BVH4="0", RAYLIB_POOL_SHORT_STACK="1"))["lstack"] == POOL_SHORT_LSTACK
    assert with_env("mid", dict(RAYLIB_BVH4="0", RAYLIB_POOL_SHORT_STACK="4"))["lstack"] == 4
    # RAYLIB_BVH4 / RAYLIB_BVH8
    p = with_env("mid", dict(RAYLIB_BVH4="0"))
    assert (p["tree"], p["treeWidth"]) == (TREE_BVH2, 2), p
    p = with_env("tess2", dict(RAYLIB_BVH4="0"))
    assert (p["tree"], p["treeWidth"], p["keepNodes4f"]) == (TREE_BVH2, 2, 0), p
    p = with_env("mid", dict(RAYLIB_BVH8="1"))
    assert (p["tree"], p["treeWidth"], p["nodeBytes"], p["eagerTree"]) == (TREE_WIDE8, 8, 80, TREE_GRID4), p
    p = with_env("soup", dict(RAYLIB_BVH8="0"))
    assert (p["tree"], p["treeWidth"], p["eagerTree"]) == (TREE_GRID4, 4, TREE_WIDE8), p
    # RAYLIB_LDS_SCENE / RAYLIB_LEAF_LIST / RAYLIB_PLAIN_KERNEL
    p = with_env("cornell", dict(RAYLIB_LDS_SCENE="0"))
    assert (p["lds"], p["tree"], p["treeWidth"], p["plain"]) == (0, TREE_BOX4, 4, 0), p
    p = with_env("cornell", dict(RAYLIB_LEAF_LIST="0"))
    assert (p["lds"], p["treeWidth"], p["plain"]) == (1, 4, 0), p
    p = with_env("cornell", dict(RAYLIB_PLAIN_KERNEL="0"))
    assert (p["lds"], p["treeWidth"], p["plain"]) == (2, 0, 0), p
    # RAYLIB_SAMPLE_BATCH / RAYLIB_SAMPLE_BUFFER_GIB
    p = with_env("cornell", dict(RAYLIB_SAMPLE_BATCH="3"), spp=8)
    assert (p["batch"], p["sampleCount"]) == (3, 3), p
    assert with_env("cornell", dict(RAYLIB_SAMPLE_BATCH="30"), spp=8)["batch"] == 8
    cells = (1920 // 8) * (1080 // 8)
    assert plan(lib, S["cornell"], w=1920, h=1080, spp=1000)["batch"] == (16 << 30) // (cells * 64 * 12)
    assert with_env("cornell", dict(RAYLIB_SAMPLE_BUFFER_GIB="1"), w=1920, h=1080, spp=1000)["batch"] == (1 << 30) // (cells * 64 * 12)
    # RAYLIB_BLOCKS_PER_CU
    assert plan(lib, S["mid"], w=1920, h=1080, spp=16)["blocks"] == 256 * 4
    assert with_env("mid", dict(RAYLIB_BLOCKS_PER_CU="1"), w=1920, h=1080, spp=16)["blocks"] == 256
    # RAYLIB_JOB_CHUNK / RAYLIB_JOB_HEADS / RAYLIB_GUIDED
    assert with_env("mid", dict(RAYLIB_JOB_CHUNK="100"), w=1920, h=1080, spp=16)["jobChunk"] == 64
    assert with_env("cornell", dict(RAYLIB_JOB_CHUNK="5000"), w=1920, h=1080, spp=16)["jobChunk"] == 1024
    assert with_env("cornell", dict(RAYLIB_JOB_CHUNK="0"), w=1920, h=1080, spp=16)["jobChunk"] == 64
    assert with_env("mid", dict(RAYLIB_JOB_HEADS="1"), w=1920, h=1080, spp=16)["heads"] == 1
    assert with_env("mid", dict(RAYLIB_JOB_HEADS="99"), w=1920, h=1080, spp=16)["heads"] == MAX_HEADS
    assert plan(lib, S["mid"], w=1920, h=1080, spp=16)["guideShift"] == 0
    assert with_env("mid", dict(RAYLIB_GUIDED="1"), w=1920, h=1080, spp=16)["guideShift"] > 0


def _launch(cells, spp, cus, per_cu, poolK, leaf_list, chunk_env=None, heads_env=None, guided=0):
    """PlanLaunch restated (one rank, every cell listed, the first launch, no sample-buffer limit reached)."""
    ppt = poolK if poolK > 0 else 1
    jobs = cells * spp * 64
    blocks = max(1, min(cus * max(1, per_cu), (jobs + BLOCK * ppt - 1) // (BLOCK * ppt)))
    waves = blocks * (BLOCK // 64)
    chunk = ((jobs // (waves * 16)) + 32) & ~63
    if chunk_env is not None:
        chunk = max(0, chunk_env)
    jc = min(1024, max(64, chunk))
    if poolK > 0 and chunk_env is None:
        h = max(1, heads_env) if heads_env is not None else MAX_HEADS
        if h >= 4:
            jc = min(jc, 256)
    if leaf_list and chunk_env is None:
        jc = min(1024, max(256, 4 * chunk))
    jc = max(64, jc & ~63)
    heads = min(MAX_HEADS, max(1, heads_env)) if heads_env is not None else MAX_HEADS
    per_head = (max(1, cells) + heads - 1) // heads
    heads = (max(1, cells) + per_head - 1) // per_head
    drawers = max(1, blocks * (1 if leaf_list else BLOCK // 64) // heads)
    shift = 1
    while (1 << shift) < 2 * drawers and shift < 24:
        shift += 1
    return dict(blocks=blocks, stackStride=blocks * BLOCK * ppt, jobChunk=jc, heads=heads, jobsPerHead=per_head * spp * 64,
                guideShift=shift + guided - 1 if guided > 0 else 0, jobs=jobs)


def test_launch_arithmetic(lib, plan_scenes, monkeypatch):
    S = plan_scenes
    sizes = ((8, 8, 1), (64, 48, 3), (256, 256, 16), (1920, 1080, 64), (1280, 720, 2), (3840, 2160, 16), (17, 9, 5))
    for name, poolK, leaf_list in (("cornell", 0, True), ("tess2", 0, False), ("mid", 2, False)):
        for (w, h, spp) in sizes:
            for cus, per_cu in ((256, 4), (256, 1), (80, 2), (1, 1)):
                cells = ((w + 7) // 8) * ((h + 7) // 8)
                p = plan(lib, S[name], w=w, h=h, spp=spp, cus=cus, per_cu=per_cu)
                assert p["jobChunk"] % 64 == 0 and 64 <= p["jobChunk"] <= 1024, (name, w, h, spp, p)
                assert p["heads"] * ((cells + p["heads"] - 1) // p["heads"]) >= cells and p["heads"] <= MAX_HEADS
                want = _launch(cells, spp, cus, per_cu, poolK, leaf_list)
                assert {k: p[k] for k in want} == want, (name, w, h, spp, cus, per_cu)
    # the switches against the restatement
    for env, kw in ((dict(RAYLIB_JOB_CHUNK="300"), dict(chunk_env=300)), (dict(RAYLIB_JOB_HEADS="3"), dict(heads_env=3)),
                    (dict(RAYLIB_JOB_HEADS="1"), dict(heads_env=1)), (dict(RAYLIB_GUIDED="2"), dict(guided=2))):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for name, poolK, leaf_list in (("cornell", 0, True), ("mid", 2, False)):
            p = plan(lib, S[name], w=1920, h=1080, spp=16)
            want = _launch(240 * 135, 16, 256, 4, poolK, leaf_list, **kw)
            assert {k: p[k] for k in want} == want, (env, name)
        for k in env:
            monkeypatch.delenv(k)
    # the leaf-list kernel's shared chunk: four waves' worth, at least 256
    p = plan(lib, S["cornell"], w=1920, h=1080, spp=64)
    assert p["jobChunk"] >= 256
    # (the pool schedule with fewer than four heads keeps its chunk: up to 1024)
    monkeypatch.setenv("RAYLIB_JOB_HEADS", "2")
    assert plan(lib, S["mid"], w=1920, h=1080, spp=64)["jobChunk"] > 256


def test_plan_export_arguments(lib, plan_scenes):
    from raylib_amd import binding
    st = binding.RendererSettings(64, 64, 1, 5, 1e-4, 0)
    out = binding.RenderPlan()
    assert lib.RaylibAMD_PlanRender(None, C.byref(st), 0, 256, 4, C.byref(out)) == 0
    assert lib.RaylibAMD_PlanRender(plan_scenes["cornell"].scene, None, 0, 256, 4, C.byref(out)) == 0
    assert lib.RaylibAMD_PlanRender(plan_scenes["cornell"].scene, C.byref(st), 0, 0, 4, C.byref(out)) == 0
    sc = lib.Raylib_CreateScene()
    assert lib.RaylibAMD_PlanRender(sc, C.byref(st), 0, 256, 4, C.byref(out)) == 0   # not finalized
    lib.Raylib_DestroyScene(sc)
