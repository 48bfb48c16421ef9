"""Child process of tests/test_gpu_rank0_entries.py: every entry point that runs on rank 0's device and stream, called straight behind a multi-rank
Raylib_Render whose frame is still in flight (csrc/rl_rt_render.hip RenderMulti).  The library reads RAYLIB_NUM_GPUS / RAYLIB_GPU_MAP / RAYLIB_GATHER* once,
when it initialises, so every rank layout needs its own process; the one-rank run of the same functions, in the pytest process, is the reference.

One block per entry (run_block): Raylib_Render of the Cornell scene at 1920 x 1080, 2 samples, into image A -- nothing is read afterwards --, the entry at
once, then (a synchronous entry that reports stats) RaylibAMD_GetLastStats, the entry's outputs, and A's pixels.

usage: python rank0_entries_child.py <workdir> <out.npz>             every entry, the control render, then Raylib_Terminate / Raylib_Initialize
       python rank0_entries_child.py <workdir> <out.npz> terminate   the control render and Raylib_Terminate / Raylib_Initialize alone"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch    # before the library is loaded: the device entries are handed torch's tensors, and both must run on one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import radiance_cases as rc  # noqa: E402
import gather_cases as gc  # noqa: E402
import lightmap_cases as lc  # noqa: E402
import lightmap_filter_cases as fc  # noqa: E402
from raylib_amd import binding  # noqa: E402

F = np.float32
FRAME = ("cornell", 1920, 1080, 2)          # multi_rank_child.FRAMES' large frame: still executing when Raylib_Render returns
STATS_FIELDS = ("ranks", "rays", "cameraSamples", "pixels", "traceLaunches", "treeWidth", "nodeBytes")   # of a synchronous entry; no waveTrips, no times
LM_W, LM_H, LM_SAMPLES, LM_MAX_PATH = 61, 47, 4, 3     # lightmap_cases.ATLASES[0], the grid atlas
LM_FILTER = (3, 0.8, 0.5, 0.05)
GATHER_BATCH = "37"                          # test_gpu_gather.py::test_several_launches: less than one sample of every point, so cut over point ranges too
DENOISE = (2, 2.0, 0.3, 0.05)


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def last_stats(lib):
    s = binding.Stats()
    lib.RaylibAMD_GetLastStats(C.byref(s))
    return s


def dump(lib, img):
    w, h = C.c_uint32(), C.c_uint32()
    assert lib.RaylibAMD_ImageSize(img, C.byref(w), C.byref(h)) == 1
    out = np.zeros((h.value, w.value, 4), F)
    lib.RaylibAMD_DumpImageRGBA(img, fp(out))
    return out


class Ctx:
    """The scenes and inputs the entries share, made once; frame: the large frame rendered and read with nothing in between."""

    def __init__(self, lib, workdir):
        self.lib, self.workdir = lib, workdir
        self.ses = {name: helpers.session_for_case(lib, name, workdir) for name in ("cornell", "cutout_sky", "cornell_glass_sun")}
        d = os.path.join(str(workdir), "rank0_entries"); os.makedirs(d, exist_ok=True)
        self.lm = binding.SceneSession(lib, helpers.scenes.cornell(os.path.join(d, "cornell12.obj"), tess=12)[0], (0, 1, 4), (0, 1, -1), 45.0, 1.0)
        self.lm_uv = lc.grid_uv(len(lc.scene_triangles(lib, self.lm.scene)))
        obj, _ = helpers.build_case("cornell", workdir)
        self.sky = binding.SceneSession(lib, obj, (0, 1, 9), (0, 1, -1), 60.0, 1.0)      # far enough back to see the sky around the box
        self.cams = [binding.create_camera(lib, (0.0, 1.0, 14.0), (0.0, 1.0, -1.0), 45.0, 64 / 48),
                     binding.create_camera(lib, (0.3, 1.2, 4.0), (0.0, 0.9, -1.0), 45.0, 64 / 48, aperture=0.3, focal=4.0)]
        name, w, h, spp = FRAME
        self.frame_settings = self.ses[name].settings(w, h, spp)
        self.frame = self.ses[name].render(w, h, spp)
        s = last_stats(lib)
        self.frame_stats = np.asarray([getattr(s, k) for k in STATS_FIELDS], np.int64)

    def enqueue_frame(self, image=None, mode=0):
        """Raylib_Render of the large frame into `image` (a new one by default); nothing is read: with several ranks the frame is in flight when this returns."""
        name, w, h, spp = FRAME
        ses = self.ses[name]
        img = self.lib.Raylib_CreateImage(w, h) if image is None else image
        st = ses.settings(w, h, 1 if mode else spp, mode=mode)
        self.lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, img)
        return img

    def close(self):
        for c in self.cams:
            self.lib.Raylib_DestroyCamera(c)
        for s in list(self.ses.values()) + [self.lm, self.sky]:
            s.close()


class Entry:
    """prep(ctx) -> call; call(A) -> {key: array or torch tensor}.  stats: synchronous and documented to report its numbers through RaylibAMD_GetLastStats;
    on_stream: enqueued on a caller's stream, reports nothing -- the stats read behind it are the render's; keeps_frame: A still holds the frame afterwards
    (otherwise the entry returns A's new pixels itself); env: set around the block."""

    def __init__(self, name, prep, stats=False, on_stream=False, keeps_frame=True, env=None):
        self.name, self.prep, self.stats, self.on_stream, self.keeps_frame, self.env = name, prep, stats, on_stream, keeps_frame, env or {}


def run_block(ctx, E):
    lib = ctx.lib
    saved = {k: os.environ.get(k) for k in E.env}
    os.environ.update(E.env)
    try:
        call = E.prep(ctx)
        torch.cuda.synchronize()
        A = ctx.enqueue_frame()                                   # 1. the frame, in flight; nothing read
        out = call(A)                                             # 2. the entry, at once
        if E.stats or E.on_stream:                                # 3. the entry's own numbers / (a caller's stream) the render's, complete
            s = last_stats(lib)
            if E.stats:
                out["stats"] = np.asarray([getattr(s, k) for k in STATS_FIELDS], np.int64)
            else:
                name, w, h, spp = FRAME
                out["render_stats"] = np.asarray([s.ranks, int(s.cameraSamples + s.culledSamples == w * h * spp), int(s.kernelMs > 0), s.gatherMode,
                                                  s.devices, s.rcclCommSize], np.int64)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if any(isinstance(v, torch.Tensor) for v in out.values()):
        torch.cuda.synchronize()
    out = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}   # 4. the entry's outputs
    if E.keeps_frame:                                             # 5. the frame, undisturbed
        got = dump(lib, A)
        out["frame_pixels_differing"] = np.asarray(int((~helpers.same(got, ctx.frame).all(-1)).sum()) if got.shape == ctx.frame.shape else -1, np.int64)
    lib.Raylib_DestroyImage(A)
    return out


# ---- the entries ---------------------------------------------------------------------------------------------------------------------
def _query_rays(n, seed):
    rng = np.random.RandomState(seed)
    o = rng.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 3.0), (n, 3)).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(F)
    return helpers.rays8(o, d)


def _trace_rays_host(scene, kind, read_first=False):
    def prep(ctx):
        rays, ses = _query_rays(513, 11), ctx.ses[scene]

        def call(A):
            if read_first:
                # the frame's pixels are read before the query: that completes the frame, whose numbers nobody has asked for yet -- and nobody will:
                # the query's are the last call's
                assert helpers.same(dump(ctx.lib, A), ctx.frame).all()
            if kind == binding.QUERY_SURFACE:
                hits, prim = binding.trace_rays(ctx.lib, ses.scene, rays, kind, with_prim=True)
                return {"hits": hits.view(np.uint32), "prim": prim}
            return {"hits": binding.trace_rays(ctx.lib, ses.scene, rays, kind).view(np.uint32)}
        return call
    return prep


def _trace_rays_stream(n, kind):
    def prep(ctx):
        dev = torch.from_numpy(_query_rays(513, 11)[:n].copy()).cuda()
        s = torch.cuda.Stream()

        def call(A):
            with torch.cuda.stream(s):
                if kind == binding.QUERY_SURFACE:
                    hits, prim = binding.trace_rays(ctx.lib, ctx.ses["cornell"].scene, dev, kind, with_prim=True)
                    return {"hits": hits, "prim": prim}
                return {"hits": binding.trace_rays(ctx.lib, ctx.ses["cornell"].scene, dev, kind)}
        return call
    return prep


def _radiance(stream):
    def prep(ctx):
        ses = ctx.ses["cornell_glass_sun"]
        rays = rc.frame_rays(ctx.lib, ses, 16, 16)
        dev, s = (torch.from_numpy(rays).cuda(), torch.cuda.Stream()) if stream else (None, None)

        def call(A):
            if not stream:
                return {"radiance": binding.trace_radiance(ctx.lib, ses.scene, rays, sample_count=2)}
            with torch.cuda.stream(s):
                return {"radiance": binding.trace_radiance(ctx.lib, ses.scene, dev, sample_count=2)}
        return call
    return prep


def gather_points(ctx):
    """64 surface points a 16 x 12 frame of the glass-and-sun scene's camera rays meets, with the hits' normals (tests/test_gpu_gather.py `cases`)."""
    ses = ctx.ses["cornell_glass_sun"]
    rays = rc.frame_rays(ctx.lib, ses, 16, 12)
    hits = binding.trace_rays(ctx.lib, ses.scene, helpers.rays8(rays[:, 0:3], rays[:, 4:7]), binding.QUERY_SURFACE)
    ok = hits["hit"] != 0
    assert ok.sum() >= 64, int(ok.sum())
    return ses, np.ascontiguousarray(gc.points(hits["p"][ok][:64], hits["n"][ok][:64], rays[ok, 3][:64]))


def _gather(kind, stream=False):
    def prep(ctx):
        ses, pts = gather_points(ctx)
        dev, s = (torch.from_numpy(pts).cuda(), torch.cuda.Stream()) if stream else (None, None)

        def call(A):
            if not stream:
                return {"values": binding.gather(ctx.lib, ses.scene, pts, kind, sample_count=8)}
            with torch.cuda.stream(s):
                return {"values": binding.gather(ctx.lib, ses.scene, dev, kind, sample_count=8)}
        return call
    return prep


def _lightmap_points(ctx):
    def call(A):
        pts, tex, n = binding.lightmap_points(ctx.lib, ctx.lm.scene, LM_W, LM_H, ctx.lm_uv)
        return {"points": pts, "texel": tex, "count": np.asarray(n, np.int64)}
    return call


def _bake(kind, filt=None):
    def prep(ctx):
        def call(A):
            atlas, cov = binding.bake_lightmap(ctx.lib, ctx.lm.scene, LM_W, LM_H, ctx.lm_uv, kind, dilate=1, max_path=LM_MAX_PATH, sample_count=LM_SAMPLES, filter=filt)
            return {"atlas": atlas, "coverage": cov}
        return call
    return prep


def _filter_lightmap(ctx):
    pts, tex, n = binding.lightmap_points(ctx.lib, ctx.lm.scene, LM_W, LM_H, ctx.lm_uv, host=True)
    vals = fc.synthetic_values(len(tex), 0, 5)
    atlas = np.full((LM_H * LM_W, 4), 1e30, F)        # what the filter must ignore at the texels nobody covers
    atlas[tex] = vals
    atlas = np.ascontiguousarray(atlas.reshape(LM_H, LM_W, 4))

    def call(A):
        out, cov = binding.filter_lightmap(ctx.lib, ctx.lm.scene, LM_W, LM_H, atlas, LM_FILTER, ctx.lm_uv, 0, dilate=1)
        return {"atlas": out, "coverage": cov}
    return call


def _views(into_a):
    def prep(ctx):
        lib, ses = ctx.lib, ctx.ses["cornell"]
        st = ses.settings(64, 48, 2)

        def call(A):
            # into_a: the frame in flight must finish before A is reallocated or overwritten, and A then holds view 0
            imgs = [A if into_a else lib.Raylib_CreateImage(64, 48), lib.Raylib_CreateImage(64, 48)]
            assert lib.RaylibAMD_RenderViews(C.byref(st), ses.scene, binding.handle_array(ctx.cams), 2, binding.handle_array(imgs)) == 1
            s = last_stats(lib)                                   # before the dumps: the batch's numbers
            out = {"view0": dump(lib, imgs[0]), "view1": dump(lib, imgs[1]), "batch_stats": np.asarray([getattr(s, k) for k in STATS_FIELDS], np.int64)}
            for img in imgs:
                if img != A:
                    lib.Raylib_DestroyImage(img)
            return out
        return call
    return prep


def _progressive(into_a):
    def prep(ctx):
        def call(A):
            P = binding.Progressive(ctx.ses["cornell"], 64, 64, 8, image=A if into_a else None)
            assert P.handle
            live = [P.step(2), P.step(2)]
            s = last_stats(ctx.lib)                               # the second pass's
            out = {"live": np.asarray(live, np.int64), "frame": P.frame(), "pass_stats": np.asarray([getattr(s, k) for k in STATS_FIELDS], np.int64)}
            assert P.close() == 1
            return out
        return call
    return prep


def _denoise(ctx):
    lib = ctx.lib
    prm = binding.DenoiseParams(*DENOISE)

    def call(A):
        # main, albedo and normal rendered straight after one another: all three frames are in flight when the denoiser is called
        albedo = ctx.enqueue_frame(mode=binding.RENDERMODE_ALBEDO)
        normal = ctx.enqueue_frame(mode=binding.RENDERMODE_SURFACE_NORMAL)
        out = lib.Raylib_CreateImage(0, 0)
        assert lib.RaylibAMD_Denoise(A, 1, albedo, normal, out, C.byref(prm)) == 1
        got = {"denoised": dump(lib, out)}
        if getattr(ctx, "keep_guides", False):
            got["albedo"], got["normal"] = dump(lib, albedo), dump(lib, normal)
        for img in (albedo, normal, out):
            lib.Raylib_DestroyImage(img)
        return got
    return call


def _postprocess(ctx):
    def call(A):
        ctx.lib.Raylib_PostProcess(A)                             # works on the frame that was just enqueued
        return {"A": dump(ctx.lib, A)}
    return call


def _render_device_strided(ctx):
    lib, ses = ctx.lib, ctx.ses["cornell"]
    st = ses.settings(64, 64, 4)
    n = lib.RaylibAMD_CellBufferFloats(64, 64, 1, 3)
    buf = torch.zeros(int(n), dtype=torch.float32, device="cuda")

    def call(A):
        # cells 1, 4, 7, ...: the single-rank path behind a drain; synchronous (the library's stream has been waited for when it returns)
        assert lib.RaylibAMD_RenderDevice(C.byref(st), ses.scene, ses.camera, 1, 3, C.c_void_p(buf.data_ptr())) == 1
        return {"cells": buf}
    return call


def _render_cells_host(ctx):
    def call(A):
        return {"cells": ctx.ses["cornell"].render_cells(64, 64, 4, 1, 3)}
    return call


def _sky_is_the_frame(ctx):
    lib = ctx.lib

    def call(A):
        lib.Raylib_SetSkyPanorama(ctx.sky.scene, A)               # the sky is the frame that is in flight
        lit = ctx.sky.render(32, 32, 2)
        lib.Raylib_SetSkyPanorama(ctx.sky.scene, None)
        return {"lit": lit, "dark": ctx.sky.render(32, 32, 2)}
    return call


def _closest_hit(ctx):
    rays = np.ascontiguousarray(helpers.golden("cornell")["hit_rays"][:65], F)

    def call(A):
        out = np.zeros(len(rays), helpers.ffi.HIT_DTYPE)
        assert ctx.lib.RaylibAMD_ClosestHit(ctx.ses["cornell"].scene, fp(rays), len(rays), 1e-4, out.ctypes.data) == 1
        return {"hits": out.view(np.uint8)}
    return call


def _eval_scatter(ctx):
    rec = np.ascontiguousarray(helpers.golden("cornell")["scatter_in"][:65], F)

    def call(A):
        out = np.zeros((len(rec), 16), F)
        assert ctx.lib.RaylibAMD_EvalScatter(ctx.ses["cornell"].scene, 0, fp(rec), len(rec), 1, fp(out)) == 1
        return {"scatter": out}
    return call


def _eval_texture(ctx):
    uv = np.random.RandomState(3).uniform(-1.5, 2.5, (65, 2)).astype(F)

    def call(A):
        out = np.zeros((len(uv), 4), F)
        assert ctx.lib.RaylibAMD_EvalTexture(ctx.ses["cutout_sky"].scene, 0, 1, fp(uv), len(uv), fp(out)) == 1      # texture 0 = leaf.png
        return {"texels": out}
    return call


_KINDS = (("any", binding.QUERY_ANY), ("closest", binding.QUERY_CLOSEST), ("surface", binding.QUERY_SURFACE))
ENTRIES = []
for _scene in ("cornell", "cutout_sky"):
    ENTRIES += [Entry("trace_rays_%s_%s" % (_k, _scene), _trace_rays_host(_scene, _kind), stats=True) for _k, _kind in _KINDS]
ENTRIES.append(Entry("trace_rays_closest_behind_a_frame_that_was_read", _trace_rays_host("cornell", binding.QUERY_CLOSEST, read_first=True), stats=True))
for _n in (1, 64, 65):
    ENTRIES += [Entry("trace_rays_device_%s_%d" % (_k, _n), _trace_rays_stream(_n, _kind), on_stream=True) for _k, _kind in _KINDS]
ENTRIES += [
    Entry("trace_radiance", _radiance(False), stats=True),
    Entry("trace_radiance_device", _radiance(True), on_stream=True),
    Entry("gather_irradiance", _gather(gc.IRRADIANCE), stats=True),
    Entry("gather_sh9", _gather(gc.SH9), stats=True),
    Entry("gather_irradiance_several_launches", _gather(gc.IRRADIANCE), stats=True, env={"RAYLIB_GATHER_BATCH": GATHER_BATCH}),
    Entry("gather_sh9_several_launches", _gather(gc.SH9), stats=True, env={"RAYLIB_GATHER_BATCH": GATHER_BATCH}),
    Entry("gather_device", _gather(gc.IRRADIANCE, stream=True), on_stream=True),
    Entry("lightmap_points", _lightmap_points),
    Entry("bake_lightmap_irradiance", _bake(gc.IRRADIANCE), stats=True),
    Entry("bake_lightmap_sh9", _bake(gc.SH9), stats=True),
    Entry("bake_lightmap_filtered", _bake(gc.IRRADIANCE, LM_FILTER), stats=True),
    Entry("filter_lightmap", _filter_lightmap, stats=True),
    Entry("render_views", _views(False)),
    Entry("render_views_into_the_frames_image", _views(True), keeps_frame=False),
    Entry("progressive", _progressive(False)),
    Entry("progressive_into_the_frames_image", _progressive(True), keeps_frame=False),
    Entry("denoise", _denoise),
    Entry("postprocess", _postprocess, keeps_frame=False),
    Entry("render_device_strided", _render_device_strided, stats=True),
    Entry("render_cells_host", _render_cells_host, stats=True),
    Entry("sky_panorama_is_the_frame", _sky_is_the_frame),
    Entry("closest_hit", _closest_hit),
    Entry("eval_scatter", _eval_scatter),
    Entry("eval_texture", _eval_texture),
]


def run_all(lib, workdir, keep_guides=False):
    """Every entry's block, and the frame the blocks compare A with; {"<entry>/<key>": array}."""
    ctx = Ctx(lib, workdir)
    ctx.keep_guides = keep_guides
    out = {"frame": ctx.frame, "frame_stats": ctx.frame_stats}
    for E in ENTRIES:
        for k, v in run_block(ctx, E).items():
            out["%s/%s" % (E.name, k)] = v
    ctx.close()
    return out


def control(lib, workdir):
    """The multi-rank path really ran: a Raylib_Render and its stats -- who rendered, how the cells were gathered, over which devices."""
    ses = helpers.session_for_case(lib, "cornell", workdir)
    img = ses.render(64, 64, 4)
    s = ses.stats()
    ses.close()
    return {"control": img, "control_stats": np.asarray([s.ranks, s.gatherMode, s.devices, s.rcclCommSize, s.cameraSamples, s.pixels, s.rays], np.int64)}


def terminate_and_reinitialise(lib, workdir):
    """Raylib_Terminate with a frame in flight, then the library again: the reference's front-ends call the pair once per run, a host application may call it
    more often.  (Never on the pytest process's shared library: a child's last act.)"""
    ses = helpers.session_for_case(lib, "cornell", workdir)
    name, w, h, spp = FRAME
    st = ses.settings(w, h, spp)
    lib.Raylib_Render(C.byref(st), ses.scene, ses.camera, lib.Raylib_CreateImage(w, h))      # (image leaked on purpose) in flight over Terminate
    lib.Raylib_FlushLogThread()
    assert lib.Raylib_Terminate() == 0           # the reference returns 0 here (raylib.cc:50)
    assert lib.Raylib_Initialize() == 1
    img = ses.render(64, 64, 4)
    s = ses.stats()
    ses.close()
    return {"reinit": img, "reinit_stats": np.asarray([s.ranks, s.gatherMode, s.devices, s.rcclCommSize, s.cameraSamples, s.pixels, s.rays], np.int64)}


if __name__ == "__main__":
    t0 = time.time()
    lib = binding.load()
    assert lib.Raylib_Initialize() == 1
    lib.RaylibAMD_SetSeed(1)
    out = {} if len(sys.argv) > 3 and sys.argv[3] == "terminate" else run_all(lib, sys.argv[1])
    out.update(control(lib, sys.argv[1]))
    out.update(terminate_and_reinitialise(lib, sys.argv[1]))
    out["seconds"] = np.asarray(time.time() - t0)
    np.savez(sys.argv[2], **out)
