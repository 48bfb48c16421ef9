"""Every rank-0 entry point behind a multi-rank frame in flight.  With RAYLIB_NUM_GPUS > 1 Raylib_Render returns while its frame is still executing
(csrc/rl_rt_render.hip RenderMulti); INTEGRATION.md ("Several GPUs behind the same calls") tells a front-end to set RAYLIB_NUM_GPUS and change nothing else, so a ray query, a gather, a
lightmap bake, a batch of views, a progressive session, the denoiser, a strided render or a test hook may be the very next call.  Each must drain where it
shares rank 0's slot-0 events, counter block or work buffers, order itself behind the frame on rank 0's stream where it does not, leave the frame's pixels
alone, and -- a synchronous entry that reports stats -- have RaylibAMD_GetLastStats report ITS numbers, not the frame's that completes later.

tests/rank0_entries_child.py runs one block per entry (frame enqueued, entry at once, stats, outputs, the frame's pixels) in a process per rank layout; the
same functions on the pytest process's one-rank library are the reference, itself tied to the oracle by the one-rank suites.  Every comparison is bit for bit."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch    # before the library is loaded: the device entries are handed torch's tensors

import helpers
import rank0_entries_child as child
from raylib_amd import binding

pytestmark = pytest.mark.gpu

LAYOUTS = [
    dict(RAYLIB_NUM_GPUS="3", RAYLIB_GPU_MAP="0,0,0"),
    dict(RAYLIB_NUM_GPUS="2", RAYLIB_GPU_MAP="0,0", RAYLIB_GATHER_SELF="1", RAYLIB_GATHER="peer"),
    dict(RAYLIB_NUM_GPUS="1", RAYLIB_GATHER_SELF="1", RAYLIB_GATHER="rccl"),
    # two PHYSICAL devices: run where the box has them, SKIPPED -- and not counted as covered -- where it has one
    dict(RAYLIB_NUM_GPUS="2", RAYLIB_GPU_MAP="0,1", RAYLIB_GATHER="rccl"),
]
GATHER_MODE = {"none": 0, "rccl": 1, "peer": 2}
LAYOUT_ENV = ("RAYLIB_NUM_GPUS", "RAYLIB_GPU_MAP", "RAYLIB_GATHER", "RAYLIB_GATHER_SELF", "RAYLIB_PIPELINE", "RAYLIB_DEVICE", "RAYLIB_POOL", "RAYLIB_LIB",
              "RAYLIB_GATHER_BATCH", "RAYLIB_QUERY_TREE")
CHILD_KILL_SECONDS = 300     # a kill limit; a child takes seconds
# A child that faulted, aborted or hung: nothing more is started on the device by this module -- the remaining layouts fail at once.
TROUBLE = []


def _layout_id(d):
    return "-".join("%s%s" % (k.replace("RAYLIB_", "").lower(), v) for k, v in d.items())


def run_child(layout, workdir, *mode):
    """rank0_entries_child.py in a fresh process under `layout`; returns (arrays, seconds)."""
    if TROUBLE:
        pytest.fail("not started: an earlier child of this module %s" % TROUBLE[0])
    out = os.path.join(str(workdir), "rank0_%s%s.npz" % ("_".join(layout.values()).replace(",", "") or "one", "_".join(mode)))
    env = dict(os.environ)
    for k in LAYOUT_ENV:
        env.pop(k, None)
    env.update(layout)
    cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rank0_entries_child.py"), str(workdir), out] + list(mode)
    t0 = time.time()
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_KILL_SECONDS)
    except subprocess.TimeoutExpired as e:
        TROUBLE.append("under %s was killed after %d s" % (_layout_id(layout), CHILD_KILL_SECONDS))
        pytest.fail("the child %s: %s" % (TROUBLE[0], (e.stderr or b"")[-3000:]))
    seconds = time.time() - t0
    if r.returncode < 0 or r.returncode in (134, 139):
        TROUBLE.append("under %s ended with return code %d" % (_layout_id(layout), r.returncode))
        pytest.fail("the child %s: %s" % (TROUBLE[0], r.stderr[-3000:]))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    print("rank0_entries_child under %s: %.1f s" % (_layout_id(layout) or "one rank", seconds))
    return np.load(out), seconds


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(helpers.same(a, b).all()) if a.dtype == np.float32 else a.tobytes() == b.tobytes()


def how_different(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return ": %s %s against %s %s" % (a.dtype, a.shape, b.dtype, b.shape)
    if a.size <= 8:
        return ": %s against %s" % (a.tolist(), b.tolist())
    return " in %d of %d bytes" % ((np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8)).sum(), a.nbytes)


@pytest.fixture(scope="module")
def one_rank(gpu_lib, workdir):
    """The same blocks on the one-rank library of this process, where nothing is ever in flight."""
    saved = {k: os.environ.pop(k) for k in ("RAYLIB_GATHER_BATCH", "RAYLIB_QUERY_TREE") if k in os.environ}
    try:
        out = child.run_all(gpu_lib, workdir, keep_guides=True)
        out.update(child.control(gpu_lib, workdir))
    finally:
        os.environ.update(saved)
    return out


@pytest.fixture(scope="module")
def denoised_on_the_host(gpu_lib, one_rank):
    """RaylibAMD_DenoiseHost on the one-rank pixels of the frame and its two guides"""
    fp = child.fp
    color, albedo, normal = (np.ascontiguousarray(one_rank[k]) for k in ("frame", "denoise/albedo", "denoise/normal"))
    h, w = color.shape[:2]
    out = np.zeros((h, w, 4), np.float32)
    prm = binding.DenoiseParams(*child.DENOISE)
    assert gpu_lib.RaylibAMD_DenoiseHost(w, h, fp(color), 1, fp(albedo), fp(normal), C.byref(prm), fp(out)) == 1
    return out


def test_the_one_rank_run_is_a_reference(one_rank, denoised_on_the_host):
    """What the N-rank runs are compared with is not trivial: rays hit, radiance and gathers are not all zero, atlases are covered, the views differ, every
    synchronous entry reported its own numbers on one rank and left the frame alone, and the documented relations between the entries hold."""
    R = one_rank
    for E in child.ENTRIES:
        if E.keeps_frame:
            assert R[E.name + "/frame_pixels_differing"] == 0, E.name
        if E.stats:
            st = R[E.name + "/stats"]
            assert st[0] == 1 and not np.array_equal(st[1:4], R["frame_stats"][1:4]), (E.name, st)
        if E.on_stream:
            assert np.array_equal(R[E.name + "/render_stats"], [1, 1, 1, 0, 1, 0]), E.name
    assert R["frame_stats"][0] == 1 and R["frame_stats"][2] + 0 > 0
    for scene in ("cornell", "cutout_sky"):
        assert R["trace_rays_any_%s/hits" % scene].sum() > 100
        closest = R["trace_rays_closest_%s/hits" % scene].view(binding.HITT_DTYPE).reshape(-1)
        surface = R["trace_rays_surface_%s/hits" % scene].view(binding.SURFACE_DTYPE).reshape(-1)
        assert np.array_equal(closest["prim"] >= 0, surface["hit"] != 0) and (surface["hit"] != 0).sum() > 100
        assert np.array_equal(helpers.bits(closest["t"][closest["prim"] >= 0]), helpers.bits(surface["t"][surface["hit"] != 0]))
        assert R["trace_rays_any_%s/stats" % scene][1] == 513
    for n in (1, 64, 65):       # the device entry on a caller's stream gives the host entry's records
        for k in ("any", "closest", "surface"):
            want = R["trace_rays_%s_cornell/hits" % k].reshape(513, -1)[:n]
            assert np.array_equal(R["trace_rays_device_%s_%d/hits" % (k, n)].view(np.uint32).reshape(n, -1), want), (k, n)
    assert same(R["trace_rays_closest_behind_a_frame_that_was_read/hits"], R["trace_rays_closest_cornell/hits"])
    assert (R["trace_radiance/radiance"][:, :3] > 0).any() and same(R["trace_radiance_device/radiance"], R["trace_radiance/radiance"])
    assert R["trace_radiance/stats"][2] == 16 * 16 * 2
    for kind in ("irradiance", "sh9"):
        assert (R["gather_%s/values" % kind][:, :3] != 0).any()
        assert same(R["gather_%s_several_launches/values" % kind], R["gather_%s/values" % kind])
        assert R["gather_%s/stats" % kind][4] == 1 < R["gather_%s_several_launches/stats" % kind][4]
        assert R["gather_%s/stats" % kind][2] == 64 * 8
    assert same(R["gather_device/values"], R["gather_irradiance/values"])
    n = int(R["lightmap_points/count"])
    assert n == len(R["lightmap_points/texel"]) > 500
    for name in ("bake_lightmap_irradiance", "bake_lightmap_sh9", "bake_lightmap_filtered", "filter_lightmap"):
        cov = R[name + "/coverage"]
        assert (cov == 1).sum() == n and (cov == 2).any() and R[name + "/stats"][3] == n, name
    assert R["bake_lightmap_irradiance/stats"][2] == n * child.LM_SAMPLES and R["filter_lightmap/stats"][1] == 0
    assert not same(R["bake_lightmap_filtered/atlas"], R["bake_lightmap_irradiance/atlas"])
    for name in ("render_views", "render_views_into_the_frames_image"):
        assert not same(R[name + "/view0"], R[name + "/view1"]) and R[name + "/batch_stats"][0] == 1
    assert same(R["render_views_into_the_frames_image/view0"], R["render_views/view0"])
    assert same(R["progressive_into_the_frames_image/frame"], R["progressive/frame"]) and R["progressive/frame"].shape == (64, 64, 4)
    assert R["progressive/pass_stats"][0] == 1 and (R["progressive/live"] > 0).all()
    assert same(R["denoise/denoised"], denoised_on_the_host) and not same(R["denoise/denoised"], R["frame"])
    assert not same(R["postprocess/A"], R["frame"])
    assert same(R["render_device_strided/cells"].reshape(-1, 4), R["render_cells_host/cells"]) and (R["render_cells_host/cells"][:, :3] > 0).any()
    assert R["sky_panorama_is_the_frame/lit"][..., :3].sum() > R["sky_panorama_is_the_frame/dark"][..., :3].sum() + 1.0
    g = helpers.golden("cornell")
    assert R["closest_hit/hits"].tobytes() == g["hits"][:65].tobytes()
    assert same(R["eval_scatter/scatter"], g["scatter_mat0"][:65])
    assert (R["eval_texture/texels"] != 0).any()


@pytest.mark.parametrize("layout", LAYOUTS, ids=_layout_id)
def test_entries_behind_a_frame_in_flight(layout, one_rank, denoised_on_the_host, workdir):
    need = 1 + max(int(x) for x in layout.get("RAYLIB_GPU_MAP", "0").split(","))
    if torch.cuda.device_count() < need:
        pytest.skip("needs %d physical devices, %d visible: NOT covered on this box" % (need, torch.cuda.device_count()))
    got, _ = run_child(layout, workdir)
    n = int(layout["RAYLIB_NUM_GPUS"])
    remote = layout.get("RAYLIB_GATHER_SELF") == "1" or need > 1
    want_mode = GATHER_MODE[layout.get("RAYLIB_GATHER", "rccl")] if remote else 0
    comm = need if want_mode == 1 else None
    # control: the multi-rank path really ran -- a layout that silently fell back to one rank would pass everything else
    for key in ("control_stats", "reinit_stats"):
        st = got[key]
        assert st[0] == n and st[1] == want_mode and st[2] == need and (comm is None or st[3] == comm), (key, st)
        assert np.array_equal(st[4:], one_rank["control_stats"][4:]), key
    assert same(got["control"], one_rank["control"])
    assert same(got["reinit"], one_rank["control"])            # Raylib_Terminate with a frame in flight, Raylib_Initialize, and the same bits again
    # the frame every block enqueues, rendered and read with nothing in between
    assert same(got["frame"], one_rank["frame"])
    assert got["frame_stats"][0] == n and np.array_equal(got["frame_stats"][1:], one_rank["frame_stats"][1:])
    failed = []
    for E in child.ENTRIES:
        keys = [k for k in one_rank if k.startswith(E.name + "/") and k not in ("denoise/albedo", "denoise/normal")]
        assert keys and sorted(keys) == sorted(k for k in got.files if k.startswith(E.name + "/")), E.name
        for key in keys:
            if key.endswith("/render_stats"):
                # 3'. an entry on a caller's stream reports nothing: the stats behind it are the render's, complete
                st = got[key]
                if not (st[0] == n and st[1] == 1 and st[2] == 1 and st[3] == want_mode and st[4] == need and (comm is None or st[5] == comm)):
                    failed.append("%s: %s are not the frame's complete numbers under %d ranks" % (key, st.tolist(), n))
            elif key.endswith("stats"):
                # 3. a synchronous entry's numbers are its own: one rank, the one-rank run's counts, not the frame's
                st = got[key]
                if not (st[0] == 1 and np.array_equal(st, one_rank[key]) and not np.array_equal(st[1:4], got["frame_stats"][1:4])):
                    failed.append("%s: %s, one rank %s, the frame %s" % (key, st.tolist(), one_rank[key].tolist(), got["frame_stats"].tolist()))
            elif not same(got[key], one_rank[key]):                # 4. the outputs, and 5. the frame (frame_pixels_differing == 0 on one rank)
                failed.append("%s differs from the one-rank run%s" % (key, how_different(got[key], one_rank[key])))
    assert same(got["denoise/denoised"], denoised_on_the_host)
    assert not failed, "\n".join(failed)


def test_terminate_and_reinitialise_on_one_rank(one_rank, workdir):
    """Raylib_Terminate returns 0, Raylib_Initialize 1 again, and the library renders the same bits -- in a child of its own: the pytest process's
    library is shared with the other tests."""
    got, _ = run_child({}, workdir, "terminate")
    for key in ("control_stats", "reinit_stats"):
        assert np.array_equal(got[key], one_rank["control_stats"]) and got[key][0] == 1, key
    assert same(got["control"], one_rank["control"]) and same(got["reinit"], one_rank["control"])
