"""Path-traced radiance for caller rays (RaylibAMD_TraceRadiance, include/raylib_amd.h) on the device.  The yardstick is always Raylib_Render, which the rest of
the suite pins to the oracle: the rays a camera generates, on the pixels' streams, must give the render's RGBA bit for bit on every pixel -- both sides break
ties the device's way, so nothing is masked.  Then the in-kernel sample runs, the path lengths, the batch edges, the device entry and the stats."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch    # before the library is loaded: test_device_entry hands it torch's tensors, and both must run on one HIP runtime

import helpers
from helpers import bits
import radiance_cases as rc

pytestmark = pytest.mark.gpu

TREE_BVH2, TREE_GRID4 = 1, 3
# RL_QUERY_CHUNK, the jobs a wave takes per atomic: read from where the kernels take it
with open(os.path.join(helpers.ROOT, "software-raytracing_amd", "csrc", "rl_kernels.h")) as _f:
    QUERY_CHUNK = int(re.search(r"^#define RL_QUERY_CHUNK (\d+)u$", _f.read(), re.M).group(1))
F = np.float32
FRAME_CASES = ["cornell", "cornell_glass_sun", "cutout_sky", "pbr_maps", "procedural"]


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, F).reshape(-1, 4), np.ascontiguousarray(want, F).reshape(-1, 4)
    eq = helpers.same(got, want).all(-1)
    assert eq.all(), "%s: %d of %d records differ (first at %d: %s against %s)" % (what, (~eq).sum(), len(eq), np.nonzero(~eq)[0][0],
                                                                                   got[~eq][0].tolist(), want[~eq][0].tolist())


def _stats(lib):
    from raylib_amd import binding
    st = binding.Stats()
    lib.RaylibAMD_GetLastStats(C.byref(st))
    return st


@pytest.fixture(scope="module")
def procedural(gpu_lib):
    from raylib_amd import binding
    mats, sph, cub, c = helpers.procedural_case()
    ses = binding.ProceduralSession(gpu_lib, mats, sph, cub, c["origin"], c["look_at"], c["fov"], c["aspect"], sun=c["sun"], sun_dir=c["sun_dir"],
                                    aperture=c["aperture"], focal=c["focal"], shutter=c["shutter"])
    yield ses
    ses.close()


@pytest.fixture(scope="module")
def pinhole_glass(gpu_lib, workdir):
    """cornell_glass_sun behind a pinhole with a closed shutter: the lens and time draws do not enter its camera rays"""
    from raylib_amd import binding
    obj, c = helpers.build_case("cornell_glass_sun", workdir)
    ses = binding.SceneSession(gpu_lib, obj, c["origin"], c["look_at"], c["fov"], c["aspect"], sun=c["sun"], sun_dir=c["sun_dir"])
    yield ses
    ses.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)


@pytest.fixture(scope="module")
def glass_frame(gpu_lib, sessions):
    """cornell_glass_sun (thin lens, open shutter, sun) at 32 x 24: its sample-0 camera rays and their radiance, computed once"""
    from raylib_amd import binding
    ses = sessions["cornell_glass_sun"]
    rays = rc.frame_rays(gpu_lib, ses, 32, 24)
    return ses, rays, binding.trace_radiance(gpu_lib, ses.scene, rays)


@pytest.mark.parametrize("name", FRAME_CASES)
def test_a_frame_through_the_side_door(gpu_lib, sessions, procedural, monkeypatch, name):
    from raylib_amd import binding
    ses = procedural if name == "procedural" else sessions[name]
    w, h = (48, 32) if name == "procedural" else (48, 48)
    for tree in ("2", "4"):
        monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
        want = ses.render(w, h, 1)
        code, plan = binding.plan_radiance(gpu_lib, ses.scene)
        assert code == 1
        assert plan["tree"] == (TREE_BVH2 if tree == "2" or name == "procedural" else TREE_GRID4), (name, tree, plan)
        assert plan["prims"] == int(name == "procedural")
        rays = rc.frame_rays(gpu_lib, ses, w, h)
        got = binding.trace_radiance(gpu_lib, ses.scene, rays, sample_first=0, sample_count=1, skip_draws=3)
        st = _stats(gpu_lib)
        assert st.treeWidth == plan["treeWidth"] == (2 if plan["tree"] == TREE_BVH2 else 4)
        assert (got[:, 3] == 1.0).all()
        _same_bits(got, want, "%s, tree %s" % (name, tree))
        assert (want[..., :3] != 0).any(), name     # (the frame shows something: at one sample per pixel at least the light itself)
    if name == "procedural":
        assert (rays[:, 3] != rays[0, 3]).any() and (rays[:, 0:3] != rays[0, 0:3]).any()    # open shutter, thin lens


@pytest.mark.parametrize("name", ["cornell", "cornell_glass_sun"])
def test_jittered_samples_and_sample_runs(gpu_lib, sessions, pinhole_glass, name):
    """Caller-side accumulation of four jittered samples equals Raylib_Render at spp = 4; a run of samples in the kernel equals the in-order float mean of the
    single-sample calls on the same rays."""
    from raylib_amd import binding
    ses = sessions["cornell"] if name == "cornell" else pinhole_glass
    w, h, spp = 32, 24, 4
    want = ses.render(w, h, spp)
    per_sample = []
    for s in range(spp):
        rays = rc.frame_rays(gpu_lib, ses, w, h, s)
        assert (rays[:, 3] == 0).all()            # closed shutter
        per_sample.append(binding.trace_radiance(gpu_lib, ses.scene, rays, sample_first=s, sample_count=1, skip_draws=3 if s == 0 else 5))
    _same_bits(rc.mean_in_order(per_sample), want, name + ", 4 jittered samples")
    assert (bits(per_sample[1]) != bits(per_sample[2])).any()
    # in-kernel runs, on the sample-0 rays
    rays = rc.frame_rays(gpu_lib, ses, w, h)
    single = [binding.trace_radiance(gpu_lib, ses.scene, rays, sample_first=s, sample_count=1, skip_draws=3) for s in range(4)]
    assert (bits(single[0]) != bits(single[1])).any()
    run = binding.trace_radiance(gpu_lib, ses.scene, rays, sample_first=0, sample_count=4, skip_draws=3)
    _same_bits(run, rc.mean_in_order(single), name + ", samples 0..3 in the kernel")
    st = _stats(gpu_lib)
    assert st.cameraSamples == len(rays) * 4 and st.rays >= st.cameraSamples
    run = binding.trace_radiance(gpu_lib, ses.scene, rays, sample_first=2, sample_count=2, skip_draws=3)
    _same_bits(run, rc.mean_in_order(single[2:4]), name + ", samples 2..3 in the kernel")


@pytest.mark.parametrize("max_path", [0, 1, 2, 5, 64])
def test_path_lengths(gpu_lib, glass_frame, max_path):
    from raylib_amd import binding
    ses, rays, _ = glass_frame
    want = ses.render(32, 24, 1, max_path=max_path)
    got = binding.trace_radiance(gpu_lib, ses.scene, rays, max_path=max_path)
    _same_bits(got, want, "maxPathLength %d" % max_path)
    if max_path == 0:
        assert (got[:, :3] == 0).all() and (got[:, 3] == 1).all()
    else:
        assert (got[:, :3] != 0).any()


def test_a_long_path_length_runs_on_a_smaller_grid(gpu_lib, glass_frame):
    """The path stack is held to 256 MiB by cutting the grid (include/raylib_amd.h).  768 rays are 3 workgroups; at maxPathLength 8192 their stack is 192 MiB and
    all 3 run, at 32768 one workgroup's is 256 MiB and 1 runs.  No path of this frame comes near 8192 bounces, so both calls trace the same paths (the same ray
    count) and must give the same bytes: a job's result does not depend on the lane, or the grid, that runs it.  Above 32768 the call is refused."""
    from raylib_amd import binding
    ses, rays, _ = glass_frame
    assert len(rays) == 3 * 256
    wide = binding.trace_radiance(gpu_lib, ses.scene, rays, max_path=8192)
    wide_rays = _stats(gpu_lib).rays
    cut = binding.trace_radiance(gpu_lib, ses.scene, rays, max_path=32768)
    assert _stats(gpu_lib).rays == wide_rays
    _same_bits(cut, wide, "maxPathLength 32768 on one workgroup against 8192 on three")
    assert (cut[:, :3] != 0).any()
    out = np.full((len(rays), 4), 7.0, F)
    prm = binding.RadianceParams(32769, 1e-4, 0, 1, 3, 0.0, 0.0)
    assert gpu_lib.RaylibAMD_TraceRadiance(ses.scene, C.byref(prm), rays.ctypes.data_as(C.POINTER(binding.PathRay)), len(rays), out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert (out == 7.0).all()


def test_batch_edges(gpu_lib, glass_frame):
    from raylib_amd import binding
    ses, rays, full = glass_frame
    long_n = QUERY_CHUNK * 4 + 1
    assert len(rays) > long_n
    for n in (1, 63, 64, 65, long_n):
        got = binding.trace_radiance(gpu_lib, ses.scene, np.ascontiguousarray(rays[:n]))
        _same_bits(got, full[:n], "the first %d rays" % n)
    # n == 0 is a success that writes nothing
    prm = binding.RadianceParams(5, 1e-4, 0, 1, 3, 0.0, 0.0)
    assert gpu_lib.RaylibAMD_TraceRadiance(ses.scene, C.byref(prm), None, 0, None) == 1
    assert len(binding.trace_radiance(gpu_lib, ses.scene, np.zeros((0, 8), F))) == 0
    # degenerate rays end, and leave their neighbours' records alone (one run)
    bad = np.ascontiguousarray(rays[:long_n]).copy()
    bad[3, 4:7] = 0.0                        # a zero direction
    bad[70, 0] = np.nan                      # NaN in the origin
    bad[71, 5] = np.nan                      # ... in the direction
    bad[130, 0:3] = np.nan; bad[130, 4:7] = np.nan
    bad[200, 4:7] = np.inf
    got = binding.trace_radiance(gpu_lib, ses.scene, bad)
    keep = np.ones(long_n, bool); keep[[3, 70, 71, 130, 200]] = False
    _same_bits(got[keep], full[:long_n][keep], "the rays beside degenerate ones")
    assert (got[:, 3] == 1).all()


def test_device_entry(gpu_lib, glass_frame):
    """Torch tensors through the device entry: a non-default stream and torch's default stream give the host entry's bytes, two calls enqueued on two streams
    give the bytes of the same calls made one after the other, and misaligned, host and foreign-device pointers are refused with nothing written."""
    from raylib_amd import binding
    ses, rays, full = glass_frame
    dev = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = binding.trace_radiance(gpu_lib, ses.scene, dev)
    s.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(rays), 4)
    assert got.cpu().numpy().tobytes() == full.tobytes()
    # torch's default stream: synchronous, on the library's stream, with stats
    got = binding.trace_radiance(gpu_lib, ses.scene, dev, sample_count=2)
    assert _stats(gpu_lib).cameraSamples == 2 * len(rays)
    want2 = binding.trace_radiance(gpu_lib, ses.scene, rays, sample_count=2)
    assert got.cpu().numpy().tobytes() == want2.tobytes()
    # two calls enqueued on two streams before either is waited for: the bytes of the same calls one after the other
    want64 = binding.trace_radiance(gpu_lib, ses.scene, rays, max_path=64)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = binding.trace_radiance(gpu_lib, ses.scene, dev, max_path=64)
    with torch.cuda.stream(s2):
        b = binding.trace_radiance(gpu_lib, ses.scene, dev, sample_count=2)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == want64.tobytes() and b.cpu().numpy().tobytes() == want2.tobytes()
    # refusals: misaligned pointers, host memory, memory of another device
    n = len(rays)
    prm = binding.RadianceParams(5, 1e-4, 0, 1, 3, 0.0, 1.0)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    ray_p = lambda p: C.cast(p, C.POINTER(binding.PathRay))
    out_p = lambda p: C.cast(p, C.POINTER(C.c_float))
    out = torch.full((n + 1, 4), 7.0, dtype=torch.float32, device="cuda")
    big = torch.zeros(n * 8 + 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fn = gpu_lib.RaylibAMD_TraceRadianceDevice
    assert fn(ses.scene, C.byref(prm), ray_p(ptr(dev)), n, out_p(ptr(out, 4)), None) == 0         # results are written as 16-byte stores
    assert fn(ses.scene, C.byref(prm), ray_p(ptr(big, 8)), n, out_p(ptr(out)), None) == 0         # rays are read as 16-byte loads
    host_out = np.full((n, 4), 7.0, F)
    assert fn(ses.scene, C.byref(prm), rays.ctypes.data_as(C.POINTER(binding.PathRay)), n, out_p(ptr(out)), None) == 0
    assert fn(ses.scene, C.byref(prm), ray_p(ptr(dev)), n, host_out.ctypes.data_as(C.POINTER(C.c_float)), None) == 0
    if torch.cuda.device_count() > 1:
        other = torch.zeros((n, 8), dtype=torch.float32, device="cuda:1")
        assert fn(ses.scene, C.byref(prm), ray_p(ptr(other)), n, out_p(ptr(out)), None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all() and (host_out == 7.0).all()
    assert fn(ses.scene, C.byref(prm), ray_p(ptr(dev)), n, out_p(ptr(out, 16)), None) == 1
    assert out[1:].cpu().numpy().tobytes() == full.tobytes()


def test_stats(gpu_lib, glass_frame, monkeypatch):
    from raylib_amd import binding
    ses, rays, _ = glass_frame
    for tree, width in (("2", 2), ("4", 4)):
        monkeypatch.setenv("RAYLIB_QUERY_TREE", tree)
        for count in (1, 3):
            binding.trace_radiance(gpu_lib, ses.scene, rays, sample_count=count)
            st = _stats(gpu_lib)
            assert st.cameraSamples == len(rays) * count and st.rays >= st.cameraSamples, st.as_dict()
            assert st.treeWidth == width == binding.plan_radiance(gpu_lib, ses.scene)[1]["treeWidth"] and st.nodeBytes == 64
            assert st.nodesVisited > 0 and st.trisTested > 0 and st.shadedHits > 0 and st.kernelMs > 0 and st.wallMs >= st.kernelMs
