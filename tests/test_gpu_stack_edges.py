"""Every traversal-stack size launched at its capacity edge, against the CPU oracle.

The scenes of tests/stack_edges.py sit exactly on and one past the edges of csrc/rl_plan.cc's stack rules, and tests/test_stack_edges_host.py proves without a
device that their rays fill the stacks to the last entry and lose a hit when one entry is missing.  Here the kernel instances those plans name -- the 16 / 32 / 64
stacks of k_trace on the binary tree and the float boxes, the scene in LDS, the pool schedule with K = 2, 3, 4 and its LDS stacks of 4 / 16 / 18 / 32 entries with
their private overflow, the 64-entry grid instances, the 8-wide tree, k_aov, and k_query on every tree -- render those scenes from the cone's apex, once through
Raylib_Render and once as two views through RaylibAMD_RenderViews (the views twin), at path lengths 1 and 4, and every pixel must equal oracle.render_region bit
for bit.  Every triangle emits its own colour, so the triangle a ray found shows at path length 1 already.  The frames are free of ties: the oracle reports
closest_hit_ties == 0 and hits_outside_own_box == 0 on each of them, which is asserted, so there is no tie budget.  Every launch asserts helpers.assert_planned
and the plan's instance against the tuple the case names, so the instance under test is the one that ran.  rayTMin is 0 (the default of 1e-4 hides what is
nearer than that; one case renders with the default).

The ray queries trace the host test's rays (and 1, 63, 64, 65 and 513 of them, the stack-filling ones first) on the tree RAYLIB_QUERY_TREE forces, against
oracle_interval_hits: every ray, none excused; SURFACE records equal RaylibAMD_ClosestHit's."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import stack_edges as se
from helpers import bits, ffi, same

pytestmark = pytest.mark.gpu

W, H, SPP = 44, 36, 2          # partial cells on both axes
SUN, SUN_DIR = (2.0, 1.5, 1.0), (0.1, 0.2, -1.0)    # a sun query from every ray that leaves the cone: the occlusion walks run up the chain as well
SWITCHES = ("RAYLIB_POOL", "RAYLIB_POOL_MIN_TRIS", "RAYLIB_POOL_SHORT_STACK", "RAYLIB_BVH4", "RAYLIB_BVH8", "RAYLIB_LDS_SCENE", "RAYLIB_LEAF_LIST",
            "RAYLIB_PLAIN_KERNEL", "RAYLIB_QUERY_TREE")
# two cameras per family (position, look-at, fov): the second is the views twin's other view.  Cones: at the apex, looking along the axis -- most pixels look
# down the chain.  The twin chains: at the apex, a narrow view along the shared axis just below the chains' mirror plane, where the 8-wide walk meets both chains
# at every level.  The soup around the flat chain: from outside, looking at the chain's small end.
CAMERAS = {"cone": (((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 100.0), ((0.0, 0.0, 0.0), (0.2, 0.1, 1.0), 80.0)),
           "twin": (((0.0, 0.0, 0.0), (1.0, 0.0, -0.1), 20.0), ((0.0, 0.0, 0.0), (1.0, 0.0, -0.15), 30.0)),
           "chain": (((0.6, 0.3, 5.0), (0.0, 0.0, 0.0), 50.0), ((3.0, 2.0, 4.0), (0.01, 0.01, 0.0), 40.0))}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


class Edge:
    pass


@pytest.fixture(scope="module")
def gedge(gpu_lib, oracle, workdir):
    """name -> the scene on the device and in the oracle, its two cameras and its rays; built when first asked for.  Oracle frames are rendered once per
    (camera, path length, rayTMin, mode) and shared."""
    from raylib_amd import binding
    made = {}

    def get(name):
        if name not in made:
            spec = se.SCENES[name]
            e = Edge()
            e.name, e.spec = name, spec
            cams = CAMERAS[spec["kind"]]
            e.ses, obj = se.make_session(gpu_lib, spec, os.path.join(str(workdir), "stack_edges_gpu"), name, origin=cams[0][0], look_at=cams[0][1],
                                         fov=cams[0][2], aspect=W / H, sun=SUN, sun_dir=SUN_DIR)
            e.flat = se.make_flat(oracle, e.ses, obj, spec, sun=SUN, sun_dir=SUN_DIR)
            e.osc = oracle.scene_create(e.flat, 1)
            e.cams = [e.ses.camera, binding.create_camera(gpu_lib, cams[1][0], cams[1][1], cams[1][2], W / H)]
            e.ocams = [ffi.make_camera(c[0], c[1], c[2], W / H) for c in cams]
            e.rays = se.scene_rays(spec)
            e.frames = {}
            made[name] = e
        return made[name]
    yield get
    for e in made.values():
        gpu_lib.Raylib_DestroyCamera(e.cams[1])
        e.ses.close(); oracle.scene_destroy(e.osc)


def oracle_frame(oracle, e, cam, max_path, tmin, mode=0):
    key = (cam, max_path, tmin, mode)
    if key not in e.frames:
        st = ffi.make_settings(W, H, SPP if mode == 0 else 1, max_path, tmin, mode)
        img = oracle.render_region(e.osc, e.ocams[cam], st, 0, 0, W, H, seed=1)
        cn = oracle.counters(e.osc)
        # no two surfaces at one t, no hit outside its triangle's own box: nothing on this frame depends on a tree's shape, so every pixel must match
        assert cn["closest_hit_ties"] == 0 and cn["hits_outside_own_box"] == 0, (e.name, key, cn)
        assert np.unique(bits(img[..., :3]).reshape(-1, 3), axis=0).shape[0] > 2, (e.name, key)      # (not a blank frame; at path length 1 a pixel shows the colour of the one triangle it found)
        e.frames[key] = img
    return e.frames[key]


def _set(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _same_frame(got, want, what):
    eq = same(got[..., :3], want[..., :3]).all(-1)
    assert eq.all(), "%s: %d of %d pixels differ from the oracle (L2 %.3e), first at %s" % (what, (~eq).sum(), eq.size, helpers.l2(got, want), np.argwhere(~eq)[0].tolist())


# (scene, switches, the instance the plan must name).  trace: (STACK, PRIMS, FULL, LDS, PLAIN); pool: (STACK, PRIMS, K, LSTACK, WIDE 0 binary / 1 grid / 3 8-wide)
RENDERS = [
    # k_trace: the 16 stack exactly full on the binary tree, on the float boxes, and with the scene in LDS
    ("cone_d16", dict(RAYLIB_LDS_SCENE="0", RAYLIB_BVH4="0"), ("trace", (16, 0, 0, 0, 0))),
    ("cone_d16", dict(RAYLIB_LDS_SCENE="0"), ("trace", (16, 0, 1, 0, 0))),
    ("cone_d16", dict(RAYLIB_LEAF_LIST="0"), ("trace", (16, 0, 1, 1, 0))),
    # one past 16: the 32 stack
    ("cone_d17", dict(), ("trace", (32, 0, 1, 0, 0))),
    ("cone_d17", dict(RAYLIB_BVH4="0"), ("trace", (32, 0, 0, 0, 0))),
    # the 32 stack exactly full, both trees; a 4-wide need of 33 falls back to the binary tree
    ("cone_d32", dict(), ("trace", (32, 0, 1, 0, 0))),
    ("cone_d32", dict(RAYLIB_BVH4="0"), ("trace", (32, 0, 0, 0, 0))),
    ("cone_n33", dict(), ("trace", (32, 0, 0, 0, 0))),
    # one past 32: the 64 stack (no pool schedule for it, whatever RAYLIB_POOL says)
    ("cone_d33", dict(), ("trace", (64, 0, 1, 0, 0))),
    ("cone_d33", dict(RAYLIB_BVH4="0"), ("trace", (64, 0, 0, 0, 0))),
    ("cone_d33", dict(RAYLIB_POOL="2"), ("trace", (64, 0, 1, 0, 0))),
    # spheres: 32 from the start, exactly full at depth 32, 64 one past
    ("prims_d16", dict(), ("trace", (32, 1, 0, 0, 0))),
    ("prims_d32", dict(), ("trace", (32, 1, 0, 0, 0))),
    ("prims_d33", dict(), ("trace", (64, 1, 0, 0, 0))),
    # the pool schedule on the binary tree: K = 2, 3, 4 with 16 entries exactly full ...
    ("cone_d16", dict(RAYLIB_POOL="2", RAYLIB_BVH4="0"), ("pool", (16, 0, 2, 16, 0))),
    ("cone_d16", dict(RAYLIB_POOL="3"), ("pool", (16, 0, 3, 16, 0))),
    ("cone_d16", dict(RAYLIB_POOL="4"), ("pool", (16, 0, 4, 16, 0))),
    # ... and with 32, all in LDS or 4 / 18 there and the rest in the private overflow
    ("cone_d32", dict(RAYLIB_POOL="2", RAYLIB_BVH4="0"), ("pool", (32, 0, 2, 32, 0))),
    ("cone_d32", dict(RAYLIB_POOL="3"), ("pool", (32, 0, 3, 32, 0))),
    ("cone_d32", dict(RAYLIB_POOL="4"), ("pool", (32, 0, 4, 32, 0))),
    ("cone_d32", dict(RAYLIB_POOL="2", RAYLIB_BVH4="0", RAYLIB_POOL_SHORT_STACK="4"), ("pool", (32, 0, 2, 4, 0))),
    ("cone_d32", dict(RAYLIB_POOL="2", RAYLIB_BVH4="0", RAYLIB_POOL_SHORT_STACK="1"), ("pool", (32, 0, 2, 18, 0))),
    ("cone_d17", dict(RAYLIB_POOL="2", RAYLIB_BVH4="0"), ("pool", (32, 0, 2, 18, 0))),
    # the pool schedule on the grid nodes: 32 exactly full, 64 one past and 64 exactly full; 65 falls back to the binary tree
    ("cone_d32", dict(RAYLIB_POOL="2"), ("pool", (32, 0, 2, 18, 1))),
    ("cone_d32", dict(RAYLIB_POOL="2", RAYLIB_POOL_SHORT_STACK="0"), ("pool", (32, 0, 2, 32, 1))),
    ("cone_n33", dict(RAYLIB_POOL="2"), ("pool", (64, 0, 2, 18, 1))),
    ("cone_n64", dict(RAYLIB_POOL="2"), ("pool", (64, 0, 2, 18, 1))),
    ("cone_n64", dict(RAYLIB_POOL="2", RAYLIB_POOL_SHORT_STACK="0"), ("pool", (64, 0, 2, 32, 1))),
    ("cone_n65", dict(RAYLIB_POOL="2"), ("pool", (32, 0, 2, 32, 0))),
    # the 8-wide tree: by default where rays are expected to take many steps, forced on the cone
    ("soup8", dict(), ("pool", (32, 0, 2, 16, 3))),
    ("cone_n64", dict(RAYLIB_POOL="2", RAYLIB_BVH8="1"), ("pool", (32, 0, 2, 16, 3))),
    # ... and at 16 levels with 15 of its 16 groups in use, 7 of them in the private overflow; 17 levels: one past, the 64-entry grid instance
    ("twin_p16", dict(RAYLIB_POOL="2", RAYLIB_BVH8="1"), ("pool", (32, 0, 2, 16, 3))),
    ("twin_p17", dict(RAYLIB_POOL="2", RAYLIB_BVH8="1"), ("pool", (64, 0, 2, 18, 1))),
]


def _id(case):
    return "%s-%s-%s" % (case[0], case[2][0], "_".join(str(x) for x in case[2][1])) + ("" if not case[1] else "-" + "".join(k.replace("RAYLIB_", "")[:6] + v for k, v in sorted(case[1].items())))


def _camera_rays_fill_the_stack(lib, oracle, e, want_instance):
    """The frame's own rays, not only the host test's, sit on the edge (the host restatement says so).  Cones: the pixel-centre rays of the first camera load
    the stack of the tree this instance walks to exactly the builder's need.  Twin chains on the 8-wide tree: the rays that use all levels - 1 groups lie in a
    sliver around the chains' mirror plane (the ray queries trace them), so of a camera's rays -- eight seeded positions in every pixel -- it is asserted that
    they load the stack of groups beyond the RL_POOL8_LSTACK / 2 = 8 groups the pool kernel keeps in LDS, into its private overflow; the most is printed."""
    kind, t = want_instance
    if kind == "trace" and t[3] == 2:
        return                                  # the leaf list has no stack
    tree = (3 if t[2] else 2) if kind == "trace" else {0: 2, 1: 4, 3: 8}[t[4]]
    family = e.spec["kind"]
    if family == "chain" or (family == "cone" and tree == 8) or (family == "twin" and tree != 8):
        return                                  # not an edge scene of that tree
    ys, xs = np.mgrid[0:H, 0:W]
    if family == "cone":
        uv = np.stack([(xs.ravel() + 0.5) / W, (ys.ravel() + 0.5) / H], 1)
    else:
        rng = np.random.RandomState(7)
        uv = np.concatenate([np.stack([(xs.ravel() + j[:, 0]) / W, (ys.ravel() + j[:, 1]) / H], 1) for j in rng.uniform(0, 1, (8, H * W, 2))])
    rays = oracle.camera_rays(e.ocams[0], uv.astype(np.float32), seed=1)[:, :6]
    _, hw = se.walk_host(lib, e.ses.scene, tree, rays, 0.0, 128)
    if family == "cone":
        need = e.spec["depth"] if tree == 2 else e.spec["need4"]
        assert int(hw.max()) == need, (e.name, want_instance, tree, int(hw.max()), need)
    else:
        print("camera rays: %s tree 8, levels8 %d: at most %d groups in use, %d of %d rays beyond the 8 in LDS" % (e.name, e.spec["levels8"], int(hw.max()), int((hw > 8).sum()), len(rays)))
        assert 8 < int(hw.max()) <= e.spec["levels8"] - 1, (e.name, int(hw.max()))


def _render_case(gpu_lib, oracle, monkeypatch, e, env, want_instance, tmin):
    _set(monkeypatch, env)
    _camera_rays_fill_the_stack(gpu_lib, oracle, e, want_instance)
    for max_path in (1, 4):
        img = e.ses.render(W, H, SPP, max_path=max_path, tmin=tmin)
        plan = helpers.assert_planned(gpu_lib, e.ses, e.ses.stats(), W, H, SPP, max_path=max_path, tmin=tmin)
        assert se.instance_of(plan) == want_instance, (e.name, env, plan)
        _same_frame(img, oracle_frame(oracle, e, 0, max_path, tmin), "%s %s one view, path length %d" % (e.name, env, max_path))
        # the views twin: both cameras in one launch
        got = e.ses.render_views(e.cams, W, H, SPP, max_path=max_path, tmin=tmin)
        st = e.ses.stats().as_dict()
        assert (st["treeWidth"], st["pathsPerWave"], st["nodeBytes"]) == (plan["treeWidth"], plan["pathsPerWave"], plan["nodeBytes"]) and st["traceLaunches"] == 1
        for v in (0, 1):
            _same_frame(got[v], oracle_frame(oracle, e, v, max_path, tmin), "%s %s view %d of 2, path length %d" % (e.name, env, v, max_path))
    print("launched: %-5s %-20s by %-10s %s  one view and as a views twin, path lengths 1 and 4, rayTMin %g" % (want_instance[0], want_instance[1], e.name, env or "{}", tmin))


@pytest.mark.parametrize("case", RENDERS, ids=[_id(c) for c in RENDERS])
def test_render_at_the_stack_edge(gpu_lib, oracle, gedge, monkeypatch, case):
    name, env, want_instance = case
    _render_case(gpu_lib, oracle, monkeypatch, gedge(name), env, want_instance, 0.0)


@pytest.mark.parametrize("case", [("cone_d32", dict(), ("trace", (32, 0, 1, 0, 0))), ("cone_d32", dict(RAYLIB_POOL="2"), ("pool", (32, 0, 2, 18, 1))),
                                  ("cone_d16", dict(), ("trace", (16, 0, 1, 2, 1)))], ids=["trace32", "pool32", "leaflist"])
def test_render_with_the_default_ray_tmin(gpu_lib, oracle, gedge, monkeypatch, case):
    """rayTMin 1e-4 hides the triangles nearer than that (sizes down to 2^-28 here): other frames, the same stacks.  With it the smallest scene takes the leaf list."""
    name, env, want_instance = case
    _render_case(gpu_lib, oracle, monkeypatch, gedge(name), env, want_instance, 1e-4)


AOVS = [("cone_d16", (16, 0)), ("cone_d17", (32, 0)), ("cone_d32", (32, 0)), ("cone_d33", (64, 0)), ("prims_d16", (32, 1)), ("prims_d32", (32, 1)), ("prims_d33", (64, 1))]


@pytest.mark.parametrize("name,want", AOVS, ids=["%s-aov_%d_%d" % (n, w[0], w[1]) for n, w in AOVS])
def test_debug_modes_at_the_stack_edge(gpu_lib, oracle, gedge, name, want):
    """k_aov walks the binary tree with the plan's STACK: the albedo and the emission mode show which triangle each pixel found."""
    from raylib_amd import binding
    e = gedge(name)
    for mode in (1, 5):
        st = binding.RendererSettings(W, H, 1, 4, 0.0, mode)
        p = binding.RenderPlan()
        assert gpu_lib.RaylibAMD_PlanRender(e.ses.scene, C.byref(st), 0, 256, 4, C.byref(p)) == 1
        assert se.instance_of(p.as_dict()) == ("aov", want), p.as_dict()
        img = e.ses.render(W, H, 1, max_path=4, tmin=0.0, mode=mode)
        _same_frame(img, oracle_frame(oracle, e, 0, 4, 0.0, mode), "%s mode %d one view" % (name, mode))
        got = e.ses.render_views(e.cams, W, H, 1, max_path=4, tmin=0.0, mode=mode)
        for v in (0, 1):
            _same_frame(got[v], oracle_frame(oracle, e, v, 4, 0.0, mode), "%s mode %d view %d of 2" % (name, mode, v))
    print("launched: aov   %-20s by %-10s modes 1 and 5, one view and as a views twin" % (want, name))


# (scene, RAYLIB_QUERY_TREE, the (TREE, STACK, PRIMS) the plan must name)
QUERIES = [("cone_d32", "2", (2, 32, 0)), ("cone_d33", "2", (2, 64, 0)), ("prims_d32", None, (2, 32, 1)), ("prims_d33", None, (2, 64, 1)),
           ("cone_d32", "4", (4, 32, 0)), ("cone_n33", "4", (4, 64, 0)), ("cone_n64", "4", (4, 64, 0)), ("cone_n65", "4", (2, 32, 0)),
           ("cone_n64", "8", (8, 32, 0)), ("chain_l16", "8", (8, 32, 0)), ("chain_l17", "8", (2, 64, 0)), ("chain_l17", "4", (2, 64, 0)),
           ("twin_l16", "8", (8, 32, 0)), ("twin_l17", "8", (2, 32, 0))]      # the 8-wide walk with 15 of its 16 groups in use; 17 levels: the binary tree


@pytest.mark.parametrize("name,tree,want", QUERIES, ids=["%s-tree%s-k_query_%d_%d_%d" % ((n, t or "default") + w) for n, t, w in QUERIES])
def test_ray_queries_at_the_stack_edge(gpu_lib, oracle, gedge, monkeypatch, name, tree, want):
    from raylib_amd import binding
    e = gedge(name)
    rays6 = e.rays
    if e.spec["sphere"] is not None:
        c, r = se.scene_sphere(e.spec)
        rng = np.random.RandomState(2)
        tgt = np.asarray(c) + rng.uniform(-1.2, 1.2, (48, 3)) * r
        o = np.where(np.arange(48)[:, None] % 2 == 0, 0.0, np.asarray(c) * 2.0)
        rays6 = np.concatenate([rays6, np.concatenate([o, tgt - o], 1).astype(np.float32)])
    # the rays that fill the stack first (the host restatement says which), so that the short batches are made of them
    _, hw = se.walk_host(gpu_lib, e.ses.scene, want[0], rays6, 0.0, 128)
    rays6 = rays6[np.argsort(-hw.astype(np.int64), kind="stable")]
    rays = helpers.rays8(rays6[:, :3], rays6[:, 3:], 0.0)
    want_all = oracle.interval_hits(e.osc, rays)
    hit_all = np.isfinite(want_all["t"])
    assert hit_all.sum() > len(rays) // 10 and int(want_all["nearerRejected"].sum()) == 0
    r6 = np.ascontiguousarray(rays6, np.float32)
    hook = np.zeros(len(r6), ffi.HIT_DTYPE)
    assert gpu_lib.RaylibAMD_ClosestHit(e.ses.scene, r6.ctypes.data_as(C.POINTER(C.c_float)), len(r6), 0.0, hook.ctypes.data) == 1
    if tree:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
    for kind in (binding.QUERY_ANY, binding.QUERY_CLOSEST, binding.QUERY_SURFACE):
        rc, plan = binding.plan_ray_query(gpu_lib, e.ses.scene, kind)
        assert rc == 1 and (plan["treeWidth"], plan["stack"], plan["prims"]) == want, plan
    for n in (1, 63, 64, 65, 513, len(rays)):
        sub, w, hit = rays[:n], want_all[:n], hit_all[:n]
        closest = binding.trace_rays(gpu_lib, e.ses.scene, sub, binding.QUERY_CLOSEST)
        st = binding.Stats(); gpu_lib.RaylibAMD_GetLastStats(C.byref(st))
        assert st.treeWidth == want[0]
        got = closest["prim"] >= 0
        assert np.array_equal(got, hit), (name, tree, n, int((got != hit).sum()), int(np.argmax(got != hit)))
        assert np.array_equal(bits(closest["t"][hit]), bits(w["t"][hit])), (name, tree, n)
        assert (closest["prim"][:, None] == w["prims"])[hit].any(1).all(), (name, tree, n)
        anyhit = binding.trace_rays(gpu_lib, e.ses.scene, sub, binding.QUERY_ANY)
        assert np.array_equal(anyhit, hit.astype(np.uint32)), (name, tree, n)
        surf = binding.trace_rays(gpu_lib, e.ses.scene, sub, binding.QUERY_SURFACE)
        assert surf.tobytes() == hook[:n].tobytes(), (name, tree, n)
    print("launched: query k_query<%d, ANY|CLOSEST|SURFACE, %d, %d> by %-10s RAYLIB_QUERY_TREE=%s  %d rays (and 1, 63, 64, 65, 513 of them), %d hits"
          % (want + (name, tree, len(rays), int(hit_all.sum()))))
