"""The motion plane on the device (include/raylib_amd.h, statements T1 to T6; csrc/rl_k_motion.inl).

The hit plane is held to RaylibAMD_RenderGBuffer's bytes on every tree.  The motion plane is held to RaylibAMD_MotionHost byte for byte, the oracle fed
RaylibAMD_EvalCameraRays' rays and the device's own hit plane.  Identity and a rigid translation check the orientation independently (the 1 - t included):
there |prevX - x|, |prevY - y| and the relative |prevT - t| stay below the margin of tests/temporal_cases.margins() -- four times what the float32 oracle was
measured to differ from float64 on the CPU (profiles/temporal_accuracy.json), far below the 0.5 at which another pixel would be fetched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch    # before the library is loaded: the device entry is handed torch's tensors

import helpers
import move_cases as mc
import temporal_cases as tc
from raylib_amd import binding

pytestmark = pytest.mark.gpu

W, H, TMIN = tc.W, tc.H, 1e-4
F = np.float32


def _procedural(lib, shutter=None):
    mats, sph, cub, cam = helpers.procedural_case()
    return binding.ProceduralSession(lib, mats, sph, cub, origin=cam["origin"], look_at=cam["look_at"], fov=cam["fov"], aspect=cam["aspect"], sun=cam["sun"],
                                     sun_dir=cam["sun_dir"], aperture=cam["aperture"], focal=cam["focal"], shutter=cam["shutter"] if shutter is None else shutter)


@pytest.fixture(scope="module")
def cases(gpu_lib, sessions, workdir):
    d = os.path.join(str(workdir), "motion"); os.makedirs(d, exist_ok=True)
    own = {"procedural": _procedural(gpu_lib), "procedural_still": _procedural(gpu_lib, (0.0, 0.0)),
           "cornell_tess4": binding.SceneSession(gpu_lib, helpers.scenes.cornell(os.path.join(d, "c4.obj"), tess=4)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)}
    yield dict(sessions, **own)
    for s in own.values():
        s.close()


def _tree(monkeypatch, tree):
    if tree is None:
        monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    else:
        monkeypatch.setenv("RAYLIB_QUERY_TREE", str(tree))


def motion(lib, ses, prev=None, first=0, pp=None, planes=("hit", "motion")):
    return binding.motion(lib, ses.scene, ses.camera, W, H, prev, first, pp, TMIN, planes)


def oracle(lib, ses, hit, prev=None, first=0, pp=None):
    return binding.motion_host(lib, ses.scene, ses.camera, W, H, tc.device_rays(lib, ses.camera, W, H), hit, prev, first, pp)


def assert_oracle(lib, ses, got, what, prev=None, first=0, pp=None):
    want = oracle(lib, ses, got["hit"], prev, first, pp)
    assert got["motion"].tobytes() == want.tobytes(), "%s: %d records differ from RaylibAMD_MotionHost" % (what, (got["motion"] != want).sum())
    return want


# ---- 1. the hit plane is the G-buffer's; the motion plane depends on neither the tree nor the hit plane being asked for ----
@pytest.mark.parametrize("tree", [None, 2, 4, 8])
def test_hit_plane_is_the_gbuffers_on_each_tree(gpu_lib, cases, monkeypatch, tree):
    lib = gpu_lib
    for name in ("cornell_tess4", "cutout_sky", "procedural_still"):
        ses = cases[name]
        _tree(monkeypatch, None)
        base = motion(lib, ses)
        _tree(monkeypatch, tree)
        got = motion(lib, ses)
        want = binding.gbuffer(lib, ses.scene, ses.camera, W, H, TMIN, ("hit",))
        assert got["hit"].tobytes() == want["hit"].tobytes(), (name, tree)
        assert got["motion"].tobytes() == base["motion"].tobytes(), (name, tree)
        alone = motion(lib, ses, planes=("motion",))
        assert list(alone) == ["motion"] and alone["motion"].tobytes() == got["motion"].tobytes(), (name, tree)
        assert motion(lib, ses, planes=("hit",))["hit"].tobytes() == want["hit"].tobytes(), (name, tree)
        if name == "cornell_tess4" and tree is not None:
            st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
            assert st.treeWidth == tree, st.as_dict()


# ---- 2. the motion plane against the oracle ----
@pytest.mark.parametrize("name", list(helpers.CASES) + ["cornell_tess4", "procedural_still", "procedural"])
def test_motion_plane_is_the_oracles(gpu_lib, cases, monkeypatch, name):
    """Same camera; a previous camera translated and rotated; one facing away -- on every case: thin lenses, sky pixels, spheres and cubes, a moving cube."""
    _tree(monkeypatch, None)
    lib, ses = gpu_lib, cases[name]
    c = tc.camera19(lib, ses.camera)
    o = c[0:3].astype(np.float64)
    fwd = -np.cross(c[7:10].astype(np.float64), c[10:13].astype(np.float64)); fwd /= np.linalg.norm(fwd)
    moved = binding.create_camera(lib, o + (0.3, 0.15, -0.2), o + (0.3, 0.15, -0.2) + fwd + (-0.05, -0.03, 0.0), 40.0, W / H)
    away = binding.create_camera(lib, o, o - fwd, 40.0, W / H)
    try:
        same = motion(lib, ses)
        assert_oracle(lib, ses, same, name + ", same camera")
        hit = same["hit"]["prim"] >= 0
        assert (same["motion"]["status"][hit] == binding.MOTION_SURFACE).all()
        if name == "cutout_sky":
            assert (~hit).sum() > 20 and (same["motion"]["status"][~hit] == binding.MOTION_SKY).all() and (same["motion"]["prevT"][~hit] == 0).all()
        if name == "procedural_still":
            assert set((same["hit"]["prim"][hit] >> 28).tolist()) == {1, 2}
        got = motion(lib, ses, moved)
        assert_oracle(lib, ses, got, name + ", camera moved", moved)
        assert got["motion"].tobytes() != same["motion"].tobytes() and got["hit"].tobytes() == same["hit"].tobytes()
        got = motion(lib, ses, away)
        assert_oracle(lib, ses, got, name + ", camera facing away", away)
        assert (got["motion"]["status"] == binding.MOTION_NONE).all() and not got["motion"].view(np.uint32).any()
        st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
        assert st.cameraSamples == st.pixels == W * H and st.rays == W * H and st.ranks == 1 and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    finally:
        lib.Raylib_DestroyCamera(moved); lib.Raylib_DestroyCamera(away)


@pytest.mark.parametrize("refitted", [False, True])
def test_partial_range_moved(gpu_lib, workdir, monkeypatch, refitted):
    """A range with first > 0 and first + count < n had other vertices; on a fresh scene, and on one whose trees a move refitted; alone and with a moved camera."""
    _tree(monkeypatch, None)
    lib = gpu_lib
    soup = mc.soup_triangles()
    ses = mc.soup_session(lib, workdir, "motion_soup_%d" % refitted, soup)
    prev_cam = binding.create_camera(lib, (0.5, 0.2, 3.8), (0.1, 0.0, 0.0), 45.0, W / H)
    try:
        first, end = 200, 400
        before = mc.pos9(mc.export(ses))
        if refitted:          # the scene moves; the previous positions are where the range was
            now = before[first:end] + np.tile(np.asarray((0.35, -0.2, 0.15), F), 3)
            assert binding.move_triangles(lib, ses.scene, first, now) == 1
            pp = before[first:end]
        else:                 # the scene stands; the range is said to have been elsewhere
            pp = before[first:end] - np.tile(np.asarray((0.2, 0.1, -0.1), F), 3)
        for what, prev in (("triangles moved", None), ("both", prev_cam)):
            got = motion(lib, ses, prev, first, pp)
            assert_oracle(lib, ses, got, what, prev, first, pp)
            assert got["hit"].tobytes() == binding.gbuffer(lib, ses.scene, ses.camera, W, H, TMIN, ("hit",))["hit"].tobytes()
            still = motion(lib, ses, prev)
            inside = (got["hit"]["prim"] >= first) & (got["hit"]["prim"] < end)
            assert inside.sum() > 10 and (~inside & (got["hit"]["prim"] >= 0)).sum() > 10
            assert (got["motion"][inside] != still["motion"][inside]).all() and got["motion"][~inside].tobytes() == still["motion"][~inside].tobytes()
        if refitted:
            assert binding.plan_motion(lib, ses.scene)[1]["treeWidth"] == 8
    finally:
        lib.Raylib_DestroyCamera(prev_cam); ses.close()


# ---- 3. identity and a rigid translation ----
def _assert_lands_on_itself(got, what):
    bound = tc.margins()
    hit = got["hit"]["prim"] >= 0
    m = got["motion"]
    assert hit.sum() > 50 and (m["status"][hit] == binding.MOTION_SURFACE).all(), what
    ys, xs = np.mgrid[0:H, 0:W]
    dx, dy = np.abs(m["prevX"] - xs)[hit].max(), np.abs(m["prevY"] - ys)[hit].max()
    dt = (np.abs(m["prevT"] - got["hit"]["t"]) / np.where(hit, got["hit"]["t"], 1))[hit].max()
    print("%s: |prevX - x| %g, |prevY - y| %g, |prevT - t| / t %g; margins %s" % (what, dx, dy, dt, bound))
    assert dx <= bound["prevX"] and dy <= bound["prevY"] and dt <= bound["prevT_rel"], (what, dx, dy, dt, bound)


@pytest.mark.parametrize("name", ["cornell", "cornell_tess4", "cutout_sky"])
def test_identity(gpu_lib, cases, monkeypatch, name):
    _tree(monkeypatch, None)
    _assert_lands_on_itself(motion(gpu_lib, cases[name]), name)


def test_rigid_translation(gpu_lib, workdir, monkeypatch):
    """Every triangle and the camera moved by one vector (multiples of 2^-3, so that the sums are exact); the untranslated positions and camera are 'previous'."""
    _tree(monkeypatch, None)
    lib = gpu_lib
    v = np.asarray((0.375, -0.25, 0.125))
    soup = mc.soup_triangles()
    grid = np.round(soup * 1024.0) / 1024.0          # on a grid of 2^-10: adding v is exact in float32
    ses = mc.soup_session(lib, workdir, "motion_rigid", grid + v, origin=tuple(np.asarray((0.25, 0.25, 4.0)) + v), look_at=tuple(v))
    prev_cam = binding.create_camera(lib, (0.25, 0.25, 4.0), (0, 0, 0), 45.0, 1.0)
    try:
        c, p = tc.camera19(lib, ses.camera), tc.camera19(lib, prev_cam)
        assert np.array_equal(c[7:13], p[7:13]) and np.array_equal((c[0:3].astype(np.float64) - v).astype(F), p[0:3]), "the two cameras differ by the translation alone"
        pp = np.ascontiguousarray(grid.reshape(-1, 9), F)
        got = motion(lib, ses, prev_cam, 0, pp)
        assert_oracle(lib, ses, got, "rigid translation", prev_cam, 0, pp)
        _assert_lands_on_itself(got, "rigid translation")
    finally:
        lib.Raylib_DestroyCamera(prev_cam); ses.close()


# ---- 4. the device entry ----
def _stats(lib):
    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
    return bytes(st)


def test_device_entry_behind_a_move_on_the_callers_stream(gpu_lib, workdir, monkeypatch):
    _tree(monkeypatch, None)
    lib = gpu_lib
    soup = mc.soup_triangles()
    moved = soup.copy(); moved[200:400] += np.asarray((0.35, -0.2, 0.15), F).astype(np.float64)
    ses = mc.soup_session(lib, workdir, "motion_move_a", soup)
    fresh = mc.soup_session(lib, workdir, "motion_move_b", moved.astype(F).astype(np.float64))
    try:
        pp_host = mc.pos9(mc.export(ses))[200:400]
        want = motion(lib, fresh, None, 200, pp_host)
        before = motion(lib, ses)                 # (the scene and its tree are on the device before it moves)
        assert before["hit"].tobytes() != want["hit"].tobytes()
        ses.render(16, 16, 1)
        stats_before = _stats(lib)
        guard = 64
        big = {k: torch.full((W * H * 4 + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for k in ("hit", "motion")}
        out = {k: v[:W * H * 4].view(H, W, 4) for k, v in big.items()}
        pp = torch.from_numpy(pp_host).cuda()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            rc, first, end = mc.move_to(lib, ses, fresh, device=True)
            got = binding.motion_device(lib, ses.scene, ses.camera, W, H, None, 200, pp, TMIN, out=out)      # straight behind the move, on the same stream
        s.synchronize()
        assert (rc, first, end) == (1, 200, 400)
        assert _stats(lib) == stats_before, "a call on a caller's stream leaves the stats alone"
        for k in ("hit", "motion"):
            words = big[k].cpu().numpy()
            assert (words[W * H * 4:] == 0x5A5A5A5A).all() and words[:W * H * 4].tobytes() == want[k].tobytes(), k
            assert got[k].data_ptr() == out[k].data_ptr()
        inside = (want["hit"]["prim"] >= 200) & (want["hit"]["prim"] < 400)
        assert inside.any() and (want["hit"]["prim"] == -1).any()
        # torch's default stream: handle 0, the library's stream, synchronous, with stats
        on_null = binding.motion_device(lib, ses.scene, ses.camera, W, H, None, 200, pp, TMIN)
        st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
        assert st.cameraSamples == st.pixels == W * H and st.rays == W * H and st.kernelMs > 0, st.as_dict()
        for k in ("hit", "motion"):
            assert on_null[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    finally:
        ses.close(); fresh.close()


def test_device_entry_refusals(gpu_lib, cases):
    lib, ses = gpu_lib, cases["cornell"]
    st = binding.RendererSettings(W, H, 1, 1, TMIN, 0)
    hit = torch.full((W * H * 4 + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    mot = torch.full((W * H * 4 + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pos = torch.zeros(4 * 9 + 4, dtype=torch.float32, device="cuda")
    host = np.full(W * H * 4, 0x5A5A5A5A, np.int32)
    host_pos = np.zeros((4, 9), F)
    good = binding.MotionParams(None, 0, 0, None)
    ok_planes = binding.MotionPlanes(hit=hit.data_ptr(), motion=mot.data_ptr())
    tries = {"a host plane": (good, binding.MotionPlanes(hit=hit.data_ptr(), motion=host.ctypes.data)),
             "hit off by 4 bytes": (good, binding.MotionPlanes(hit=hit.data_ptr() + 4)),
             "motion off by 8 bytes": (good, binding.MotionPlanes(motion=mot.data_ptr() + 8)),
             "host positions": (binding.MotionParams(None, 0, 4, host_pos.ctypes.data), ok_planes),
             "positions off by 2 bytes": (binding.MotionParams(None, 0, 4, pos.data_ptr() + 2), ok_planes)}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for what, (prm, planes) in tries.items():
        for handle in (None, C.c_void_p(stream.cuda_stream)):
            assert lib.RaylibAMD_RenderMotionDevice(C.byref(st), ses.scene, ses.camera, C.byref(prm), C.byref(planes), handle) == 0, what
    torch.cuda.synchronize()
    assert (host == 0x5A5A5A5A).all() and (hit.cpu().numpy() == 0x5A5A5A5A).all() and (mot.cpu().numpy() == 0x5A5A5A5A).all()
    # positions need 4-byte alignment only
    prm = binding.MotionParams(None, 0, 4, pos.data_ptr() + 4)
    assert lib.RaylibAMD_RenderMotionDevice(C.byref(st), ses.scene, ses.camera, C.byref(prm), C.byref(ok_planes), None) == 1
