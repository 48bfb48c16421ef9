"""The variance-guided filter on the device (include/raylib_amd.h, statements S1 to S7; csrc/rl_temporal.hip k_temporal_moments, csrc/rl_variance.hip) against its
host oracles, byte for byte: on the crafted planes of tests/test_variance_host.py, on sizes from one pixel to several tiles at the smallest and the largest
iteration count, on the device's own G-buffer planes, as a four-frame loop of move -> render -> G-buffer -> motion -> accumulate -> filter on a stream of the
caller's, and, as a condition on the statement itself, that filtering an accumulated Cornell frame brings it nearer to the converged one."""
import ctypes as C

import numpy as np
import pytest
import torch    # before the library is loaded: the device entry is handed torch's tensors

import helpers
import move_cases as mc
import temporal_cases as tc
import variance_cases as vc
from raylib_amd import binding

pytestmark = pytest.mark.gpu

W, H, TMIN = vc.W, vc.H, 1e-4
F = np.float32
ACC = ("outColour", "outLength", "outMoments")
FIL = ("outColour", "outVariance")


def _same(got, want, what, names):
    for g, w_, n in zip(got, want, names):
        assert g.tobytes() == w_.tobytes(), "%s: %s differs in %d values" % (what, n, (helpers.bits(g) != helpers.bits(w_)).sum())


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.int32).reshape(a.shape + (a.dtype.itemsize // 4,))
    return torch.from_numpy(a).cuda()


def _frame(lib, ses, seed, w=W, h=H, spp=1):
    """A colour frame: RaylibAMD_RenderCellsHost at cellFirst 0, cellStride 1 -- the row-major image"""
    lib.RaylibAMD_SetSeed(seed)
    try:
        return np.ascontiguousarray(ses.render_cells(w, h, spp, 0, 1)).reshape(h, w, 4)
    finally:
        lib.RaylibAMD_SetSeed(1)


_identity_motion = vc.identity_motion


def test_crafted_planes(gpu_lib):
    """Both calls through the host-array entries, then through the device entries: a stream of the caller's with guard words behind the outputs and the stats left
    alone, then torch's default stream, synchronous, with stats."""
    lib = gpu_lib
    a = vc.moments_history()
    want_a = binding.temporal_accumulate_moments(lib, a[0], a[1], a[2], a[3], tc.TOL, tc.CAP, host=True)
    _same(binding.temporal_accumulate_moments(lib, a[0], a[1], a[2], a[3], tc.TOL, tc.CAP), want_a, "accumulate, host entry", ACC)
    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.pixels == W * H and st.ranks == 1 and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    _same(binding.temporal_accumulate_moments(lib, a[0], a[1], a[2], None, tc.TOL, tc.CAP),
          binding.temporal_accumulate_moments(lib, a[0], a[1], a[2], None, tc.TOL, tc.CAP, host=True), "accumulate, no history", ACC)
    b = vc.crafted_filter()
    prm = dict(iterations=3, history_length=2.5)
    want_f = binding.filter_variance(lib, *b, params=prm, host=True)
    _same(binding.filter_variance(lib, *b, params=prm), want_f, "filter, host entry", FIL)
    lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.pixels == W * H and st.ranks == 1 and st.kernelMs > 0 and st.traceLaunches == 5, st.as_dict()
    no_v = binding.filter_variance(lib, *b, params=prm, variance=False)
    assert no_v[1] is None and no_v[0].tobytes() == want_f[0].tobytes(), "S7: the colour without the variance plane"
    # the device entries
    lib.RaylibAMD_GetLastStats(C.byref(st))
    before = bytes(st)
    guard, n = 64, W * H
    big = [torch.full((n * k + guard,), 7.0, dtype=torch.float32, device="cuda") for k in (4, 1, 2, 4, 1)]
    ta = [_dev(x) for x in (a[0], a[1], a[2]) + a[3]]
    tb = [_dev(x) for x in b]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        binding.temporal_accumulate_moments_device(lib, ta[0], ta[1], ta[2], tuple(ta[3:]), tc.TOL, tc.CAP,
                                                   out=(big[0][:n * 4].view(H, W, 4), big[1][:n].view(H, W), big[2][:n * 2].view(H, W, 2)))
        binding.filter_variance_device(lib, *tb, params=prm, out=(big[3][:n * 4].view(H, W, 4), big[4][:n].view(H, W)))
    s.synchronize()
    now = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(now))
    assert bytes(now) == before, "a call on a caller's stream leaves the stats alone"
    host = [t.cpu().numpy() for t in big]
    for t, k in zip(host, (4, 1, 2, 4, 1)):
        assert (t[n * k:] == 7).all(), "the guard words behind an output"
    _same((host[0][:n * 4].reshape(H, W, 4), host[1][:n].reshape(H, W), host[2][:n * 2].reshape(H, W, 2)), want_a, "accumulate, device entry on a stream", ACC)
    _same((host[3][:n * 4].reshape(H, W, 4), host[4][:n].reshape(H, W)), want_f, "filter, device entry on a stream", FIL)
    on_null = binding.temporal_accumulate_moments_device(lib, ta[0], ta[1], ta[2], tuple(ta[3:]), tc.TOL, tc.CAP)
    _same(tuple(x.cpu().numpy() for x in on_null), want_a, "accumulate, device entry, synchronous", ACC)
    lib.RaylibAMD_GetLastStats(C.byref(now))
    assert now.pixels == n and now.kernelMs > 0
    on_null = binding.filter_variance_device(lib, *tb, params=prm)
    _same(tuple(x.cpu().numpy() for x in on_null), want_f, "filter, device entry, synchronous", FIL)
    lib.RaylibAMD_GetLastStats(C.byref(now))
    assert now.pixels == n and now.kernelMs > 0 and now.traceLaunches == 5


def _random_planes(w, h, seed):
    """Random planes of any size: surfaces and sky, smooth positions with bumps, normals from a small set, short and long histories."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    colour = rng.uniform(0, 2, (h, w, 4)).astype(F); colour[..., 3] = 1
    hit = np.zeros((h, w), binding.HITT_DTYPE); hit["t"] = 2; hit["prim"] = rng.randint(-1, 3, (h, w))
    normals = np.asarray([(0, 0, 1), (0, 1, 0), (0.6, 0, 0.8)], F)
    N = normals[((xs // 5 + ys // 3) % 3)]
    P = np.stack([xs * 0.1, ys * 0.1, rng.uniform(-0.05, 0.05, (h, w))], -1).astype(F)
    m1 = rng.uniform(0, 2, (h, w)).astype(F)
    moments = np.stack([m1, m1 * m1 + rng.uniform(-0.1, 0.5, (h, w))], -1).astype(F)
    length = rng.choice(np.asarray([1, 2, 4, 9], F), (h, w)).astype(F)
    return colour, moments, length, hit, vc.surface_plane(hit["prim"], P, N)


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (64, 40), (37, 21)])
def test_sizes(gpu_lib, size, k):
    """One pixel, half a tile, several tiles, and a frame that is no multiple of the 16 x 16 tile (nor of the accumulation's 8 x 8 cell); at K = 6 the step of 32
    exceeds 21 rows, so whole tap rows fall off the frame."""
    w, h = size
    planes = _random_planes(w, h, 10 * w + k)
    prm = dict(iterations=k)
    _same(binding.filter_variance(gpu_lib, *planes, params=prm), binding.filter_variance(gpu_lib, *planes, params=prm, host=True), "filter %d x %d, K = %d" % (w, h, k), FIL)
    if k == 1:
        rng = np.random.RandomState(w)
        ys, xs = np.mgrid[0:h, 0:w]
        colour, _, length, hit, _ = planes
        motion = _identity_motion(hit)
        motion["prevX"] = xs + rng.uniform(-1.5, 1.5, (h, w)); motion["prevY"] = ys + rng.uniform(-1.5, 1.5, (h, w))
        history = (rng.uniform(0, 2, (h, w, 4)).astype(F), hit, rng.choice(np.asarray([0, 1, 5], F), (h, w)).astype(F), rng.uniform(0, 4, (h, w, 2)).astype(F))
        _same(binding.temporal_accumulate_moments(gpu_lib, colour, hit, motion, history, 0.01, 4),
              binding.temporal_accumulate_moments(gpu_lib, colour, hit, motion, history, 0.01, 4, host=True), "accumulate %d x %d" % size, ACC)


def test_on_the_devices_gbuffer_planes(gpu_lib, sessions):
    """Real planes: the G-buffer's hit and surface, a 1-spp frame accumulated once onto another, then filtered."""
    lib = gpu_lib
    for name in ("cornell", "cutout_sky"):
        ses = sessions[name]
        gb = binding.gbuffer(lib, ses.scene, ses.camera, W, H, TMIN, ("hit", "surface"))
        motion = _identity_motion(gb["hit"])
        first = binding.temporal_accumulate_moments(lib, _frame(lib, ses, 3), gb["hit"], motion, None, 0.02, 32)
        acc = binding.temporal_accumulate_moments(lib, _frame(lib, ses, 2), gb["hit"], motion, (first[0], gb["hit"], first[1], first[2]), 0.02, 32)
        want = binding.temporal_accumulate_moments(lib, _frame(lib, ses, 2), gb["hit"], motion, (first[0], gb["hit"], first[1], first[2]), 0.02, 32, host=True)
        _same(acc, want, name + ": accumulate", ACC)
        assert (acc[1] == 2).all()
        got = binding.filter_variance(lib, acc[0], acc[2], acc[1], gb["hit"], gb["surface"])
        _same(got, binding.filter_variance(lib, acc[0], acc[2], acc[1], gb["hit"], gb["surface"], host=True), name + ": filter", FIL)
        sky = gb["hit"]["prim"] == -1
        assert (name == "cornell" or sky.any()) and (~sky).sum() > W * H // 4
        assert got[0][sky].tobytes() == np.where(np.isfinite(acc[0]), acc[0], F(0))[sky].tobytes() and not got[1][sky].any()
        assert (got[0][~sky] != acc[0][~sky]).any(), "%s: the filter changed the surfaces" % name


def test_four_frame_loop_on_a_callers_stream(gpu_lib, workdir, monkeypatch):
    """move -> render -> G-buffer (surface) -> motion (hit + motion) -> accumulate with moments -> filter -> swap, four times: the device entries on one stream of
    the caller's with no host synchronisation between the motion launch, the accumulation and the filter; the oracles' chain at every frame."""
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    lib = gpu_lib
    ses = mc.soup_session(lib, workdir, "variance_loop", mc.soup_triangles())
    prm = dict(iterations=3, history_length=3.0)
    try:
        first, end = 150, 450
        step = np.tile(np.asarray((0.04, -0.02, 0.03), F), 3)
        pos = mc.pos9(mc.export(ses))[first:end]
        s = torch.cuda.Stream()
        hist_dev = hist_host = None
        for k in range(4):
            prev_pos = pos.copy()
            pos = (pos + step).astype(F)
            t_pos, t_prev = torch.from_numpy(pos).cuda(), torch.from_numpy(prev_pos).cuda()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                assert binding.move_triangles(lib, ses.scene, first, t_pos) == 1
            colour = _frame(lib, ses, 10 + k)                      # 1 spp of the moved scene (synchronous, on the library's stream; it settles the move)
            t_colour = torch.from_numpy(colour).cuda()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g = binding.gbuffer_device(lib, ses.scene, ses.camera, W, H, TMIN, ("surface",))
                m = binding.motion_device(lib, ses.scene, ses.camera, W, H, None, first, t_prev, TMIN)
                acc = binding.temporal_accumulate_moments_device(lib, t_colour, m["hit"], m["motion"], hist_dev, 0.05, 5.0)     # straight behind the motion launch
                fil = binding.filter_variance_device(lib, acc[0], acc[2], acc[1], m["hit"], g["surface"], params=prm)          # ... and behind the accumulation
            s.synchronize()
            hit = m["hit"].cpu().numpy().view(binding.HITT_DTYPE).reshape(H, W)
            mot = m["motion"].cpu().numpy().view(binding.MOTION_DTYPE).reshape(H, W)
            surface = g["surface"].cpu().numpy().view(binding.SURFACE_DTYPE).reshape(H, W)
            want_m = binding.motion_host(lib, ses.scene, ses.camera, W, H, tc.device_rays(lib, ses.camera, W, H), hit, None, first, prev_pos)
            assert mot.tobytes() == want_m.tobytes(), "frame %d: the motion plane" % k
            assert surface.tobytes() == binding.gbuffer(lib, ses.scene, ses.camera, W, H, TMIN, ("surface",))["surface"].tobytes(), "frame %d: the surface plane" % k
            want = binding.temporal_accumulate_moments(lib, colour, hit, want_m, hist_host, 0.05, 5.0, host=True)
            _same(tuple(x.cpu().numpy() for x in acc), want, "frame %d: accumulate" % k, ACC)
            want_f = binding.filter_variance(lib, want[0], want[2], want[1], hit, surface, params=prm, host=True)
            _same(tuple(x.cpu().numpy() for x in fil), want_f, "frame %d: filter" % k, FIL)
            if k:
                assert (want[1] > 1).sum() > W * H // 4 and (want[1] == 1).any(), "frame %d: history is found, and lost somewhere" % k
            hist_dev, hist_host = (acc[0], m["hit"], acc[1], acc[2]), (want[0], hit, want[1], want[2])
        assert (want[1] >= 3).any() and (want[1] < 3).any(), "both kinds of initial variance were taken"
    finally:
        ses.close()


def test_device_entry_refusals(gpu_lib):
    lib = gpu_lib
    a = vc.moments_history()
    b = vc.crafted_filter()
    ta = [_dev(x) for x in (a[0], a[1], a[2]) + a[3]]
    tb = [_dev(x) for x in b]
    pad = torch.zeros(W * H * 11 + 8, dtype=torch.float32, device="cuda")
    out_c = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda"); out_l = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda")
    out_m = torch.full((H, W, 2), 7.0, dtype=torch.float32, device="cuda")
    host_c, host_l, host_m = np.full((H, W, 4), 7, F), np.full((H, W), 7, F), np.full((H, W, 2), 7, F)
    torch.cuda.synchronize()
    P = C.byref(binding.TemporalParams(tc.TOL, tc.CAP))
    hp = dict(colour=ta[3].data_ptr(), hit=ta[4].data_ptr(), length=ta[5].data_ptr(), moments=ta[6].data_ptr())
    fr = lambda **kw: C.byref(binding.TemporalMomentsFrame(**dict(hp, **kw)))
    c_, h_, m_, oc, ol, om = ta[0].data_ptr(), ta[1].data_ptr(), ta[2].data_ptr(), out_c.data_ptr(), out_l.data_ptr(), out_m.data_ptr()
    acc = {"a host colour": (W, H, P, a[0].ctypes.data, h_, m_, fr(), oc, ol, om),
           "a host history moments": (W, H, P, c_, h_, m_, fr(moments=a[3][3].ctypes.data), oc, ol, om),
           "a host outMoments": (W, H, P, c_, h_, m_, fr(), oc, ol, host_m.ctypes.data),
           "a host outColour": (W, H, P, c_, h_, m_, fr(), host_c.ctypes.data, ol, om),
           "history moments off by 4 bytes": (W, H, P, c_, h_, m_, fr(moments=pad.data_ptr() + 4), oc, ol, om),
           "history length off by 2 bytes": (W, H, P, c_, h_, m_, fr(length=pad.data_ptr() + 2), oc, ol, om),
           "outMoments off by 4 bytes": (W, H - 1, P, c_, h_, m_, None, oc, ol, om + 4),
           "outColour off by 8 bytes": (W, H - 1, P, c_, h_, m_, None, oc + 8, ol, om),
           "outMoments is the history's moments": (W, H, P, c_, h_, m_, fr(moments=om), oc, ol, om)}
    fp = dict(colour=tb[0].data_ptr(), moments=tb[1].data_ptr(), length=tb[2].data_ptr(), hit=tb[3].data_ptr(), surface=tb[4].data_ptr())
    pl = lambda **kw: C.byref(binding.VarianceFilterPlanes(**dict(fp, **kw)))
    fil = {"a host colour": (W, H, None, pl(colour=b[0].ctypes.data), oc, ol), "a host surface": (W, H, None, pl(surface=b[4].ctypes.data), oc, ol),
           "a host length": (W, H, None, pl(length=b[2].ctypes.data), oc, ol), "a host outColour": (W, H, None, pl(), host_c.ctypes.data, ol),
           "a host outVariance": (W, H, None, pl(), oc, host_l.ctypes.data),
           "colour off by 8 bytes": (W, H, None, pl(colour=pad.data_ptr() + 8), oc, ol), "hit off by 4 bytes": (W, H, None, pl(hit=pad.data_ptr() + 4), oc, ol),
           "moments off by 4 bytes": (W, H, None, pl(moments=pad.data_ptr() + 4), oc, ol), "surface off by 2 bytes": (W, H, None, pl(surface=pad.data_ptr() + 2), oc, ol),
           "length off by 2 bytes": (W, H, None, pl(length=pad.data_ptr() + 2), oc, ol),
           "outColour off by 4 bytes": (W, H - 1, None, pl(), oc + 4, ol), "outVariance off by 2 bytes": (W, H - 1, None, pl(), oc, ol + 2),
           "outColour is colour": (W, H, None, pl(colour=oc), oc, ol)}
    stream = torch.cuda.Stream()
    for handle in (None, C.c_void_p(stream.cuda_stream)):
        for what, args in acc.items():
            assert lib.RaylibAMD_TemporalAccumulateMomentsDevice(*args, handle) == 0, what
        for what, args in fil.items():
            assert lib.RaylibAMD_FilterVarianceDevice(*args, handle) == 0, what
    torch.cuda.synchronize()
    for t in (out_c, out_l, out_m):
        assert (t.cpu().numpy() == 7).all()
    assert (host_c == 7).all() and (host_l == 7).all() and (host_m == 7).all()
    # a surface, a length and a variance plane need 4-byte alignment only, a moments plane 8
    assert lib.RaylibAMD_FilterVarianceDevice(W, H - 1, None, pl(surface=tb[4].data_ptr() + 4, length=tb[2].data_ptr() + 4, moments=tb[1].data_ptr() + 8), oc, ol + 4, None) == 1


def test_filtering_brings_an_accumulated_frame_nearer_to_the_converged_one(gpu_lib, sessions):
    """The statement's purpose, as a condition and not a tuned number: eight 1-spp Cornell frames (seeds 10 .. 17) accumulated under identity motion and filtered
    with the defaults have a smaller mean squared error against a 1024-spp frame than the accumulated frame has unfiltered."""
    mse_acc, mse_fil = vc.quality(gpu_lib, sessions["cornell"], _frame)
    print("Cornell 64 x 40, 8 x 1 spp against 1024 spp: mse accumulated %.6g, filtered %.6g" % (mse_acc, mse_fil))
    assert mse_fil < mse_acc, "mse of the filtered frame %.6g is not below the accumulated frame's %.6g" % (mse_fil, mse_acc)
