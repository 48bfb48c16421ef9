"""The temporal accumulation on the device (include/raylib_amd.h, statements T7 and T8; csrc/rl_temporal.hip) against its host oracle, byte for byte: on the
crafted planes of tests/test_temporal_host.py, on the device's own motion planes with 1-spp colour frames under different seeds, and as a four-frame loop of
move -> render -> motion -> accumulate on a stream of the caller's, which must equal the oracle's chain at every frame."""
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


def _same(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), "%s: outColour differs in %d pixels" % (what, (helpers.bits(got[0]) != helpers.bits(want[0])).any(-1).sum())
    assert got[1].tobytes() == want[1].tobytes(), "%s: outLength differs in %d pixels" % (what, (helpers.bits(got[1]) != helpers.bits(want[1])).sum())


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.int32).reshape(a.shape + (4,))
    return torch.from_numpy(a).cuda()


def _frame(lib, ses, seed, w=W, h=H):
    """A 1-spp colour frame: RaylibAMD_RenderCellsHost at cellFirst 0, cellStride 1 -- the row-major image"""
    lib.RaylibAMD_SetSeed(seed)
    try:
        return np.ascontiguousarray(ses.render_cells(w, h, 1, 0, 1)).reshape(h, w, 4)
    finally:
        lib.RaylibAMD_SetSeed(1)


def test_crafted_planes(gpu_lib):
    lib = gpu_lib
    colour, hit, motion, history = tc.crafted()
    want = binding.temporal_accumulate(lib, colour, hit, motion, history, tc.TOL, tc.CAP, host=True)
    _same(binding.temporal_accumulate(lib, colour, hit, motion, history, tc.TOL, tc.CAP), want, "host entry")
    st = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(st))
    assert st.pixels == W * H and st.ranks == 1 and st.kernelMs > 0 and st.wallMs >= st.kernelMs, st.as_dict()
    first = binding.temporal_accumulate(lib, colour, hit, motion, None, tc.TOL, tc.CAP)
    _same(first, binding.temporal_accumulate(lib, colour, hit, motion, None, tc.TOL, tc.CAP, host=True), "no history")
    # the device entry: a stream of the caller's, guard words behind the outputs, the stats left alone; then torch's default stream, synchronous
    lib.RaylibAMD_GetLastStats(C.byref(st))
    before = bytes(st)
    guard = 64
    big_c = torch.full((W * H * 4 + guard,), 7.0, dtype=torch.float32, device="cuda"); big_l = torch.full((W * H + guard,), 7.0, dtype=torch.float32, device="cuda")
    t = [_dev(a) for a in (colour, hit, motion) + history]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        binding.temporal_accumulate_device(lib, t[0], t[1], t[2], tuple(t[3:]), tc.TOL, tc.CAP, out=(big_c[:W * H * 4].view(H, W, 4), big_l[:W * H].view(H, W)))
    s.synchronize()
    now = binding.Stats(); lib.RaylibAMD_GetLastStats(C.byref(now))
    assert bytes(now) == before, "a call on a caller's stream leaves the stats alone"
    c, l = big_c.cpu().numpy(), big_l.cpu().numpy()
    assert (c[W * H * 4:] == 7).all() and (l[W * H:] == 7).all()
    _same((c[:W * H * 4].reshape(H, W, 4), l[:W * H].reshape(H, W)), want, "device entry on a stream")
    on_null = binding.temporal_accumulate_device(lib, t[0], t[1], t[2], tuple(t[3:]), tc.TOL, tc.CAP)
    _same(tuple(x.cpu().numpy() for x in on_null), want, "device entry, synchronous")
    lib.RaylibAMD_GetLastStats(C.byref(now))
    assert now.pixels == W * H and now.kernelMs > 0


@pytest.mark.parametrize("size", [(1, 1), (8, 8), (37, 21), (64, 40)])
def test_sizes(gpu_lib, size):
    """One pixel, one whole cell, a frame that is no multiple of the cell with an odd pixel count, several blocks' worth of cells: random planes with fractional
    motion everywhere."""
    w, h = size
    rng = np.random.RandomState(w)
    ys, xs = np.mgrid[0:h, 0:w]
    colour = rng.uniform(0, 2, (h, w, 4)).astype(F); hc = rng.uniform(0, 2, (h, w, 4)).astype(F)
    hit = np.zeros((h, w), binding.HITT_DTYPE); hit["t"] = 2; hit["prim"] = rng.randint(-1, 2, (h, w))
    motion = np.zeros((h, w), binding.MOTION_DTYPE)
    motion["prevX"] = xs + rng.uniform(-1.5, 1.5, (h, w)); motion["prevY"] = ys + rng.uniform(-1.5, 1.5, (h, w))
    motion["prevT"] = np.where(hit["prim"] >= 0, 2, 0); motion["status"] = np.where(hit["prim"] >= 0, binding.MOTION_SURFACE, binding.MOTION_SKY)
    history = (hc, hit, rng.choice(np.asarray([0, 1, 5], F), (h, w)).astype(F))
    _same(binding.temporal_accumulate(gpu_lib, colour, hit, motion, history, 0.01, 4), binding.temporal_accumulate(gpu_lib, colour, hit, motion, history, 0.01, 4, host=True),
          "%d x %d" % size)


def test_on_the_devices_motion_planes(gpu_lib, sessions):
    """Real planes: this frame's and a previous camera's, 1-spp colour frames under two seeds as colour and history."""
    lib = gpu_lib
    for name in ("cornell", "cutout_sky"):
        ses = sessions[name]
        prev = binding.create_camera(lib, (0.05, 1.02, 4.0), (0, 1, -1), 45.0, 1.0)
        try:
            now = binding.motion(lib, ses.scene, ses.camera, W, H, prev, tmin=TMIN)
            old = binding.motion(lib, ses.scene, prev, W, H, planes=("hit",), tmin=TMIN)["hit"]       # the previous frame's hit plane: the walk through that camera
            colour, hist = _frame(lib, ses, 2), _frame(lib, ses, 3)
            length = np.full((H, W), 3, F)
            got = binding.temporal_accumulate(lib, colour, now["hit"], now["motion"], (hist, old, length), 0.02, 32)
            want = binding.temporal_accumulate(lib, colour, now["hit"], now["motion"], (hist, old, length), 0.02, 32, host=True)
            _same(got, want, name)
            assert (got[1] == 4).sum() > W * H // 4, "%s: most of a slightly moved camera's pixels find their history" % name
            assert (got[1] == 1).any() or name == "cornell"
        finally:
            lib.Raylib_DestroyCamera(prev)


def test_four_frame_loop_on_a_callers_stream(gpu_lib, workdir, monkeypatch):
    """move -> render -> motion (hit + motion) -> accumulate -> swap, four times: the device entries on one stream of the caller's with no host synchronisation
    between the motion launch and the accumulation (the 1-spp render between the move and them is synchronous); the oracle's chain (RaylibAMD_MotionHost, RaylibAMD_TemporalAccumulateHost) at every frame."""
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    lib = gpu_lib
    ses = mc.soup_session(lib, workdir, "temporal_loop", mc.soup_triangles())
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
                m = binding.motion_device(lib, ses.scene, ses.camera, W, H, None, first, t_prev, TMIN)
                acc = binding.temporal_accumulate_device(lib, t_colour, m["hit"], m["motion"], hist_dev, 0.05, 3.0)      # straight behind the motion launch
            s.synchronize()
            hit = m["hit"].cpu().numpy().view(binding.HITT_DTYPE).reshape(H, W)
            mot = m["motion"].cpu().numpy().view(binding.MOTION_DTYPE).reshape(H, W)
            want_m = binding.motion_host(lib, ses.scene, ses.camera, W, H, tc.device_rays(lib, ses.camera, W, H), hit, None, first, prev_pos)
            assert mot.tobytes() == want_m.tobytes(), "frame %d: the motion plane" % k
            assert hit.tobytes() == binding.gbuffer(lib, ses.scene, ses.camera, W, H, TMIN, ("hit",))["hit"].tobytes(), "frame %d: the moved triangles are seen" % k
            want = binding.temporal_accumulate(lib, colour, hit, want_m, hist_host, 0.05, 3.0, host=True)
            _same(tuple(x.cpu().numpy() for x in acc), want, "frame %d" % k)
            if k:
                assert (want[1] > 1).sum() > W * H // 4 and (want[1] == 1).any(), "frame %d: history is found, and lost somewhere" % k
            hist_dev, hist_host = (acc[0], m["hit"], acc[1]), (want[0], hit, want[1])
        assert want[1].max() == 3.0                                # the cap was reached
    finally:
        ses.close()


def test_device_entry_refusals(gpu_lib):
    lib = gpu_lib
    colour, hit, motion, history = tc.crafted()
    t = [_dev(a) for a in (colour, hit, motion) + history]
    pad = torch.zeros(W * H * 4 + 8, dtype=torch.float32, device="cuda")
    out_c = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda"); out_l = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda")
    host_c, host_l = np.full((H, W, 4), 7, F), np.full((H, W), 7, F)
    torch.cuda.synchronize()
    P = C.byref(binding.TemporalParams(tc.TOL, tc.CAP))
    fr = lambda **kw: C.byref(binding.TemporalFrame(**dict(dict(colour=t[3].data_ptr(), hit=t[4].data_ptr(), length=t[5].data_ptr()), **kw)))
    c_, h_, m_, oc, ol = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), out_c.data_ptr(), out_l.data_ptr()
    tries = {"a host colour": (W, H, P, colour.ctypes.data, h_, m_, fr(), oc, ol),
             "a host history length": (W, H, P, c_, h_, m_, fr(length=history[2].ctypes.data), oc, ol),
             "a host outColour": (W, H, P, c_, h_, m_, fr(), host_c.ctypes.data, ol),
             "a host outLength": (W, H, P, c_, h_, m_, fr(), oc, host_l.ctypes.data),
             "colour off by 4 bytes": (W, H, P, pad.data_ptr() + 4, h_, m_, fr(), oc, ol),
             "motion off by 8 bytes": (W, H, P, c_, h_, pad.data_ptr() + 8, fr(), oc, ol),
             "history hit off by 4 bytes": (W, H, P, c_, h_, m_, fr(hit=pad.data_ptr() + 4), oc, ol),
             "history length off by 2 bytes": (W, H, P, c_, h_, m_, fr(length=pad.data_ptr() + 2), oc, ol),
             "outColour off by 4 bytes": (W, H - 1, P, c_, h_, m_, None, oc + 4, ol),
             "outLength off by 2 bytes": (W, H - 1, P, c_, h_, m_, None, oc, ol + 2),
             "outColour is the history's colour": (W, H, P, c_, h_, m_, fr(colour=oc), oc, ol)}
    stream = torch.cuda.Stream()
    for what, args in tries.items():
        for handle in (None, C.c_void_p(stream.cuda_stream)):
            assert lib.RaylibAMD_TemporalAccumulateDevice(*args, handle) == 0, what
    torch.cuda.synchronize()
    assert (out_c.cpu().numpy() == 7).all() and (out_l.cpu().numpy() == 7).all() and (host_c == 7).all() and (host_l == 7).all()
    # a length plane needs 4-byte alignment only
    assert lib.RaylibAMD_TemporalAccumulateDevice(W, H - 1, P, c_, h_, m_, None, oc, ol + 4, None) == 1
