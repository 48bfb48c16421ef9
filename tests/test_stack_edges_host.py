"""The traversal stacks at their capacity edges, without a device.

csrc/rl_plan.cc gives a launch STACK 16 if the binary tree's depth is <= 16 (and the scene has no spheres or cubes), 32 if <= 32, else 64; walks a 4-wide tree
only if its stackNeed4 fits 32 or 64; walks the 8-wide tree only up to RL_POOL8_MAXLEVELS levels.  Every device walk guards its push with sp < STACK, so a rule
that is off by one faults nowhere: the walk drops a subtree and the image is plausible and wrong.  Here the device's stack discipline restated on the host with
the capacity as an argument (RaylibAMD_SceneWalkStackHost) runs the rays tests/test_gpu_stack_edges.py traces, on scenes whose builder numbers sit exactly on
and one past every edge (tests/stack_edges.py):
  * at the capacity the planner gives the instance every ray's t is the brute-force answer over all primitives (oracle_interval_hits), bit for bit;
  * some ray's stack reaches the builder's reported need -- the binary tree's depth, the 4-wide tree's stackNeed4 -- which on the "exactly full" scenes is the capacity;
  * one entry less than that and some of the same rays get another t.
So these rays would show an off-by-one in either direction.  Then the reachability sweep: every kernel instance of rl_kernels.h's four lists is either planned
for a named scene under named switches, or listed in UNREACHED with the reason; no plan names an instance outside the lists.

Measured here (profiles/r12_stack_edges.log): on the cones the high-water mark equals depth on the binary tree and stackNeed4 on both 4-wide formats.

The 8-wide walk's stack of groups takes an entry only at a level where two or more INNER children of a node are hit, one per level below the root: a tree of
L levels needs at most L - 1.  Two mirrored, tilted chains on one axis (twin_l16, twin_l17; twin_p16, twin_p17 with a
stackNeed4 that lets a render walk them) reach exactly that; the planner's rule, 16 levels on 16 groups, has
one entry to spare, so the guard at the 16th group is never met on a walked tree (WALK_EDGE_UNTESTED).  The cones load 5 groups and the flat chains beside a
soup 12, with rays in their plane, which hit nothing: those chains are the PLANNER's edge scenes (16 levels walked, 17 not), not a walk's."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import helpers
import stack_edges as se
from helpers import scenes, ffi, bits

TREE_NONE, TREE_BVH2, TREE_BOX4, TREE_GRID4, TREE_WIDE8 = range(5)
POOL_SHORT_LSTACK, POOL8_LSTACK, POOL8_MAXLEVELS = 18, 16, 16
SWITCHES = ("RAYLIB_POOL", "RAYLIB_POOL_MIN_TRIS", "RAYLIB_POOL_SHORT_STACK", "RAYLIB_BVH4", "RAYLIB_BVH8", "RAYLIB_LDS_SCENE", "RAYLIB_LEAF_LIST",
            "RAYLIB_PLAIN_KERNEL", "RAYLIB_QUERY_TREE")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def edge(lib, oracle, workdir):
    """name -> (session, flat scene, oracle scene, rays), built when first asked for."""
    made = {}

    def get(name):
        if name not in made:
            spec = se.SCENES[name]
            ses, obj = se.make_session(lib, spec, os.path.join(str(workdir), "stack_edges_host"), name)
            flat = se.make_flat(oracle, ses, obj, spec)
            rays = se.scene_rays(spec)
            if spec["sphere"] is not None:   # ... and some at the sphere, from the apex and from the far side: the analytic leaf
                c, r = se.scene_sphere(spec)
                rng = np.random.RandomState(2)
                tgt = np.asarray(c) + rng.uniform(-1.2, 1.2, (48, 3)) * r
                o = np.where(np.arange(48)[:, None] % 2 == 0, 0.0, np.asarray(c) * 2.0)
                rays = np.concatenate([rays, np.concatenate([o, tgt - o], 1).astype(np.float32)])
            made[name] = (ses, flat, oracle.scene_create(flat, 1), rays)
        return made[name]
    yield get
    for ses, _, sc, _ in made.values():
        ses.close(); oracle.scene_destroy(sc)


@pytest.mark.parametrize("name", sorted(se.SCENES))
def test_builder_numbers_sit_on_the_edges(lib, edge, name):
    spec = se.SCENES[name]
    b = se.tree_numbers(lib, edge(name)[0].scene)
    assert (b["depth"], b["need4"], b["levels8"]) == (spec["depth"], spec["need4"], spec["levels8"]), (name, b)


def _capacities(spec, tree):
    """The capacities rl_plan.cc gives a walk of `tree` (2 binary, 3 4-wide float boxes, 4 4-wide grid, 8 8-wide) on this scene; empty where the planner does not walk it."""
    by_depth = 16 if spec["depth"] <= 16 and spec["sphere"] is None else 32 if spec["depth"] <= 32 else 64
    if tree == 2:
        return [by_depth]
    if tree == 3:   # k_trace on the float boxes: its STACK by depth, if stackNeed4 fits that
        return [by_depth] if spec["need4"] <= by_depth else []
    if tree == 4:   # the pool schedule and the ray queries: 32 or 64 by stackNeed4
        return [32 if spec["need4"] <= 32 else 64] if spec["need4"] <= 64 else []
    return [POOL8_MAXLEVELS] if spec["levels8"] <= POOL8_MAXLEVELS else []


# the walks whose rays fill the capacity to its last entry
FULL = {("cone_d16", 2): 16, ("cone_d16", 3): 16, ("cone_d32", 2): 32, ("cone_d32", 3): 32, ("cone_d32", 4): 32, ("prims_d32", 2): 32, ("cone_n64", 4): 64}
# Every cone scene on its binary tree and on both formats of its 4-wide tree: the walks' edges.  The flat chains and the soup are the planner's edges
# (test_planner_only_edges); the 8-wide walk has a test of its own below.
CONES = sorted(n for n in se.SCENES if se.SCENES[n]["kind"] == "cone")
WALKS = [(n, t) for n in CONES for t in (2, 3, 4) if t == 2 or se.SCENES[n]["need4"] is not None]
PLANNER_ONLY = ("chain_l16", "chain_l17", "soup8")
WALK_EDGE_UNTESTED = {
    "Push8's guard at the 16th group (RL_POOL8_MAXLEVELS)":
        "unreachable on a tree the planner walks: the stack holds one group per level below the root, at most levels - 1 = 15 for 16 levels "
        "(test_eight_wide_walk_at_its_edge reaches 15 and shows the loss at 14; the 17-level tree that would fill 16 is not walked)",
}


def _brute_force(oracle, osc, rays):
    want = oracle.interval_hits(osc, helpers.rays8(rays[:, :3], rays[:, 3:], 0.0))
    assert int(want["nearerRejected"].sum()) == 0 and np.isfinite(want["t"]).sum() > len(rays) // 10
    return want


@pytest.mark.parametrize("name,tree", WALKS, ids=["%s-tree%d" % w for w in WALKS])
def test_walk_at_capacity_and_one_entry_short(lib, oracle, edge, name, tree):
    spec = se.SCENES[name]
    ses, flat, osc, rays = edge(name)
    want = _brute_force(oracle, osc, rays)
    need = spec["depth"] if tree == 2 else spec["need4"]
    caps = _capacities(spec, tree)
    # the walk with room to spare: the brute-force answer, and the stack's high-water mark -- exactly the builder's reported need
    t_free, hw = se.walk_host(lib, ses.scene, tree, rays, 0.0, 128)
    assert np.array_equal(bits(t_free), bits(want["t"])), (name, tree)
    top = int(hw.max())
    print("stack edge: %-10s tree %d  depth %2d need4 %s levels8 %s  capacities %s  high-water %2d (%d of %d rays)"
          % (name, tree, spec["depth"], spec["need4"], spec["levels8"], caps, top, int((hw == top).sum()), len(rays)))
    assert top == need, (name, tree, top)
    for cap in caps:
        # at the planner's capacity: every ray, the same bits
        t_cap, hw_cap = se.walk_host(lib, ses.scene, tree, rays, 0.0, cap)
        assert np.array_equal(bits(t_cap), bits(want["t"])), (name, tree, cap)
        assert int(hw_cap.max()) == need <= cap
    if (name, tree) in FULL:
        assert need == FULL[(name, tree)] == min(caps)
    if not caps and tree == 4:
        # the planner does not walk this tree here -- and must not: at the largest capacity it could give, a ray loses its hit
        assert need > 64
        t_big, _ = se.walk_host(lib, ses.scene, tree, rays, 0.0, 64)
        assert (bits(t_big) != bits(want["t"])).any(), (name, tree)
    # one entry short of the need: a pushed subtree is dropped, and with it some ray's closest hit
    t_short, hw_short = se.walk_host(lib, ses.scene, tree, rays, 0.0, need - 1)
    changed = bits(t_short) != bits(want["t"])
    print("            one entry short (%d): %d rays lose their closest hit" % (need - 1, int(changed.sum())))
    assert changed.any(), (name, tree, need)
    assert int(hw_short.max()) == need - 1
    assert (hw[changed] == need).all()          # only rays that filled the stack can lose anything


@pytest.mark.parametrize("name", ["twin_l16", "twin_l17", "twin_p16", "twin_p17"])
def test_eight_wide_walk_at_its_edge(lib, oracle, edge, name):
    """The 8-wide walk's stack of groups.  A group is pushed only while a node's hit inner children are worked through, one entry per level below the root, so a
    tree of L levels needs at most L - 1 groups: the planner's rule (walk up to RL_POOL8_MAXLEVELS = 16 levels on a stack of 16 groups) has one entry to spare,
    and Push8's guard at the 16th group cannot be met on a tree it walks (WALK_EDGE_UNTESTED).  The twin chains reach exactly L - 1: 15 on the deepest tree the
    planner walks, with the brute-force answer at the capacity and a lost hit at one group less than the rays use; the tree of 17 levels, which the planner
    does not walk, would fill all 16 groups, and loses hits at 15."""
    spec = se.SCENES[name]
    ses, flat, osc, rays = edge(name)
    want = _brute_force(oracle, osc, rays)
    need = spec["levels8"] - 1
    t_free, hw = se.walk_host(lib, ses.scene, 8, rays, 0.0, 128)
    assert np.array_equal(bits(t_free), bits(want["t"])), name
    top = int(hw.max())
    print("stack edge: %-10s tree 8  levels8 %d  capacities %s  high-water %2d groups (%d of %d rays)"
          % (name, spec["levels8"], _capacities(spec, 8), top, int((hw == top).sum()), len(rays)))
    assert top == need, (name, top)
    t_cap, hw_cap = se.walk_host(lib, ses.scene, 8, rays, 0.0, POOL8_MAXLEVELS)
    assert np.array_equal(bits(t_cap), bits(want["t"])) and int(hw_cap.max()) == need <= POOL8_MAXLEVELS
    assert (need == POOL8_MAXLEVELS) == (name in ("twin_l17", "twin_p17"))
    t_short, hw_short = se.walk_host(lib, ses.scene, 8, rays, 0.0, need - 1)
    changed = bits(t_short) != bits(want["t"])
    print("            one group short (%d): %d rays lose their closest hit" % (need - 1, int(changed.sum())))
    assert changed.any() and int(hw_short.max()) == need - 1 and (hw[changed] == need).all()


@pytest.mark.parametrize("name", ["cone_n64", "cone_n65", "chain_l16", "soup8"])
def test_eight_wide_walk_below_its_capacity(lib, oracle, edge, name):
    """The other scenes that carry an 8-wide tree load few groups (a chain gives every node one inner child): at the capacity every ray has the brute-force answer."""
    spec = se.SCENES[name]
    ses, flat, osc, rays = edge(name)
    want = _brute_force(oracle, osc, rays)
    t_cap, hw = se.walk_host(lib, ses.scene, 8, rays, 0.0, POOL8_MAXLEVELS)
    assert np.array_equal(bits(t_cap), bits(want["t"])), name
    print("below capacity: %-10s tree 8  levels8 %d  capacity %d groups  high-water %d" % (name, spec["levels8"], POOL8_MAXLEVELS, int(hw.max())))
    assert 1 <= int(hw.max()) <= spec["levels8"] - 1


def test_planner_only_edges(lib, edge, monkeypatch):
    """The flat chains and the soup sit on the planner's edges for the 8-wide tree, not on a walk's: 16 levels are walked, 17 are not."""
    from raylib_amd import binding
    assert set(PLANNER_ONLY) == {n for n in se.SCENES if se.SCENES[n]["kind"] == "chain"}
    monkeypatch.setenv("RAYLIB_QUERY_TREE", "8")
    for name, want in (("chain_l16", (8, 2 * POOL8_MAXLEVELS)), ("chain_l17", (2, 64))):
        rc, p = binding.plan_ray_query(lib, edge(name)[0].scene, 1)
        assert rc == 1 and (p["treeWidth"], p["stack"]) == want, (name, p)
    monkeypatch.delenv("RAYLIB_QUERY_TREE")
    p = _render_plan(lib, edge("soup8")[0])
    assert instance_of(p) == ("pool", (2 * POOL8_MAXLEVELS, 0, 2, POOL8_LSTACK, 3)), p
    p = _render_plan(lib, edge("chain_l17")[0])
    assert instance_of(p) == ("trace", (64, 0, 0, 0, 0)), p


def test_exactly_full_scenes(lib):
    """The scenes on an edge fill the capacity the planner gives them to the last entry; the ones one past select the next."""
    S = se.SCENES
    assert _capacities(S["cone_d16"], 2) == [16] and _capacities(S["cone_d17"], 2) == [32] and _capacities(S["prims_d16"], 2) == [32]
    assert _capacities(S["cone_d32"], 2) == [32] and _capacities(S["cone_d33"], 2) == [64]
    assert _capacities(S["prims_d32"], 2) == [32] and _capacities(S["prims_d33"], 2) == [64]
    assert _capacities(S["cone_d16"], 3) == [16] and _capacities(S["cone_d16"], 4) == [32] and _capacities(S["cone_d17"], 3) == [32]
    assert _capacities(S["cone_d32"], 3) == [32] and _capacities(S["cone_d32"], 4) == [32]
    assert _capacities(S["cone_n33"], 3) == [] and _capacities(S["cone_n33"], 4) == [64] and _capacities(S["cone_d33"], 3) == [64]
    assert _capacities(S["cone_n64"], 4) == [64] and _capacities(S["cone_n65"], 4) == []
    assert _capacities(S["chain_l16"], 8) == [16] and _capacities(S["chain_l17"], 8) == []
    assert _capacities(S["twin_p16"], 8) == [16] and _capacities(S["twin_p17"], 8) == [] and _capacities(S["twin_p17"], 4) == [64]
    assert _capacities(S["twin_l16"], 8) == [16] and _capacities(S["twin_l17"], 8) == [] and _capacities(S["twin_l16"], 4) == []


def test_walk_export_arguments(lib, edge):
    ses = edge("cone_d16")[0]
    r = np.zeros((1, 6), np.float32); r[0, 5] = 1.0
    t = np.zeros(1, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.RaylibAMD_SceneWalkStackHost(ses.scene, 2, fp(r), 1, 0.0, 16, fp(t), None) == 1
    assert lib.RaylibAMD_SceneWalkStackHost(ses.scene, 3, fp(r), 1, 0.0, 16, fp(t), None) == 1      # the float boxes
    assert lib.RaylibAMD_SceneWalkStackHost(ses.scene, 5, fp(r), 1, 0.0, 16, fp(t), None) == 0      # not a tree
    assert lib.RaylibAMD_SceneWalkStackHost(ses.scene, 8, fp(r), 1, 0.0, 16, fp(t), None) == 0      # the scene has no 8-wide tree
    assert lib.RaylibAMD_SceneWalkStackHost(ses.scene, 2, fp(r), 1, 0.0, -1, fp(t), None) == 0
    assert lib.RaylibAMD_SceneWalkStackHost(ses.scene, 2, None, 1, 0.0, 16, fp(t), None) == 0
    assert lib.RaylibAMD_SceneWalkStackHost(ses.scene, 2, fp(r), 1, 0.0, 16, None, None) == 0
    assert lib.RaylibAMD_SceneWalkStackHost(None, 2, fp(r), 1, 0.0, 16, fp(t), None) == 0
    assert lib.RaylibAMD_SceneWalkStackHost(ses.scene, 2, fp(r), 0, 0.0, 0, fp(t), None) == 1


def test_the_deepest_tree_stays_inside_the_builders_bound(lib, workdir):
    """A pure chain down to the depth at which the builder leaves the SAH for median splits, then thousands of degenerate triangles: the deepest binary tree this
    generator reaches.  The builder's own bound is 36 + 25 = 61 < 64, the largest stack."""
    from raylib_amd import binding
    obj = se.write_obj(os.path.join(str(workdir), "deepest.obj"), se.deepest_triangles())
    ses = binding.SceneSession(lib, obj, (0, 0, 0), (0, 0, 1), 90.0, 1.0)
    b = se.tree_numbers(lib, ses.scene)
    assert b["depth"] == se.DEEPEST_DEPTH <= 61, b
    p = _render_plan(lib, ses)
    assert (p["poolK"], p["stack"], p["tree"]) == (0, 64, TREE_BVH2), p
    ses.close()


# ---- reachability of every listed kernel instance ---------------------------------------------------------------------------------------------
# rl_kernels.h, written out as the other plan tests write theirs
TRACE_INSTANCES = {(16, 0, 0, 0, 0), (16, 0, 1, 0, 0), (16, 0, 1, 1, 0), (16, 0, 1, 2, 0), (16, 0, 1, 2, 1),
                   (32, 0, 0, 0, 0), (32, 0, 1, 0, 0), (32, 1, 0, 0, 0), (32, 1, 1, 0, 0),
                   (64, 0, 0, 0, 0), (64, 0, 1, 0, 0), (64, 1, 0, 0, 0), (64, 1, 1, 0, 0)}                 # (STACK, PRIMS, FULL, LDS, PLAIN)
POOL_INSTANCES = {(16, 0, 2, 16, 0), (16, 0, 3, 16, 0), (16, 0, 4, 16, 0), (32, 0, 2, 32, 0), (32, 0, 3, 32, 0), (32, 0, 4, 32, 0),
                  (32, 0, 2, 4, 0), (32, 0, 2, POOL_SHORT_LSTACK, 0),
                  (32, 0, 2, 32, 1), (64, 0, 2, 32, 1), (32, 0, 2, POOL_SHORT_LSTACK, 1), (64, 0, 2, POOL_SHORT_LSTACK, 1),
                  (2 * POOL8_MAXLEVELS, 0, 2, POOL8_LSTACK, 3)}                                           # (STACK, PRIMS, K, LSTACK, WIDE)
AOV_INSTANCES = {(16, 0), (32, 0), (32, 1), (64, 0), (64, 1)}                                            # (STACK, PRIMS)
QUERY_INSTANCES = {(tree, kind, stack, prims) for kind in (0, 1, 2)
                   for (tree, stack, prims) in ((2, 32, 0), (2, 32, 1), (2, 64, 0), (2, 64, 1), (4, 32, 0), (4, 64, 0), (8, 2 * POOL8_MAXLEVELS, 0))}
# listed, compiled, and selected by no plan:
UNREACHED = {
    ("trace", (32, 1, 1, 0, 0)): "Pick() walks a wide tree only when the scene has no spheres or cubes (wide = !p.prims && ...): FULL never goes with PRIMS",
    ("trace", (64, 1, 1, 0, 0)): "as k_trace<32, true, true>",
}


def _render_plan(lib, ses, tmin=1e-4, mode=0, sky=False):
    from raylib_amd import binding
    st = binding.RendererSettings(44, 36, 2, 4, tmin, mode)
    out = binding.RenderPlan()
    assert lib.RaylibAMD_PlanRender(ses.scene, C.byref(st), int(sky), 256, 4, C.byref(out)) == 1
    return out.as_dict()


instance_of = se.instance_of


@pytest.fixture(scope="module")
def sweep_scenes(lib, edge, workdir):
    """The edge scenes and the scenes of tests/test_render_plan_host.py."""
    from raylib_amd import binding
    d = os.path.join(str(workdir), "stack_edges_sweep"); os.makedirs(d, exist_ok=True)
    obj = lambda path: binding.SceneSession(lib, path, (0, 1, 4), (0, 1, -1), 45.0, 1.0)
    S = {"cornell": obj(scenes.cornell(os.path.join(d, "cornell.obj"))[0]), "cutout": obj(scenes.cutout(os.path.join(d, "cutout.obj"))[0]),
         "pbr_maps": obj(scenes.pbr_maps(os.path.join(d, "pbr.obj"))[0]), "tess2": obj(scenes.cornell(os.path.join(d, "tess2.obj"), tess=2)[0]),
         "mid": obj(scenes.cornell(os.path.join(d, "mid.obj"), tess=24, displace_fraction=0.2)[0])}
    S["soup"] = obj(se.write_obj(os.path.join(d, "soup.obj"), se.soup_chain_triangles(1000, 0)))
    S["deep"] = obj(se.write_obj(os.path.join(d, "deep.obj"), se.soup_chain_triangles(1000, 72)))     # tests/test_render_plan_host.py's deep scene
    mats = np.zeros(1, ffi.MAT_DTYPE)
    mats["type"] = 0; mats["albedo"] = (0.5, 0.5, 0.5); mats["roughness"] = 1.0; mats["ior"] = 1.5
    S["spheres"] = binding.ProceduralSession(lib, mats, [dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0)], ())
    own = list(S)
    for name in se.SCENES:
        S[name] = edge(name)[0]
    yield S
    for k in own:
        S[k].close()


def test_every_listed_instance_is_reached_or_named_unreachable(lib, sweep_scenes, monkeypatch):
    """Scenes x the per-render switches of INTEGRATION.md's table x sky or none x rayTMin below zero or not x path tracing or a debug mode."""
    values = {"RAYLIB_POOL": (None, "0", "2", "3", "4"), "RAYLIB_POOL_SHORT_STACK": (None, "0", "1", "4"), "RAYLIB_BVH4": (None, "0"),
              "RAYLIB_BVH8": (None, "0", "1"), "RAYLIB_LDS_SCENE": (None, "0"), "RAYLIB_LEAF_LIST": (None, "0"), "RAYLIB_PLAIN_KERNEL": (None, "0"),
              "RAYLIB_POOL_MIN_TRIS": (None, "100")}
    keys = sorted(values)
    reached = {}
    listed = {("trace", t) for t in TRACE_INSTANCES} | {("pool", t) for t in POOL_INSTANCES} | {("aov", t) for t in AOV_INSTANCES} | {("query", t) for t in QUERY_INSTANCES}
    for combo in itertools.product(*[values[k] for k in keys]):
        env = {k: v for k, v in zip(keys, combo) if v is not None}
        for k in keys:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for name, ses in sweep_scenes.items():
            for sky, tmin, mode in ((False, 1e-4, 0), (True, 1e-4, 0), (False, -1e-4, 0), (False, 1e-4, 1), (True, -1e-4, 1)):
                inst = instance_of(_render_plan(lib, ses, tmin=tmin, sky=sky, mode=mode))
                assert inst in listed, (name, env, sky, tmin, mode, inst)     # KernelFor / AovKernelFor would return null
                reached.setdefault(inst, (name, env, sky, tmin))
    for k in keys:
        monkeypatch.delenv(k, raising=False)
    from raylib_amd import binding
    for name, ses in sweep_scenes.items():
        for qt in (None, "2", "4", "8"):
            monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
            if qt:
                monkeypatch.setenv("RAYLIB_QUERY_TREE", qt)
            for kind in (0, 1, 2):
                rc, p = binding.plan_ray_query(lib, ses.scene, kind)
                assert rc == 1
                inst = ("query", (p["treeWidth"], kind, p["stack"], p["prims"]))
                assert inst in listed, (name, qt, inst)
                reached.setdefault(inst, (name, {"RAYLIB_QUERY_TREE": qt} if qt else {}, False, 1e-4))
    for inst in sorted(reached):
        print("reached: %-6s %-22s by %-10s %s%s%s" % (inst[0], inst[1], reached[inst][0], reached[inst][1] or "{}", " sky" if reached[inst][2] else "",
                                                       " rayTMin<0" if reached[inst][3] < 0 else ""))
    assert listed - set(reached) == set(UNREACHED), sorted(listed - set(reached))
    assert not (set(UNREACHED) & set(reached))
    print("instances listed %d, reached %d, unreached %d" % (len(listed), len(reached), len(UNREACHED)))
