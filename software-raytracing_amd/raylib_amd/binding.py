"""ctypes binding of libraylib.so -- the Python mirror of the reference's own FFI
wrapper (gui-app/gui-app/RaylibWrapper.cs:43-145 binds the same 33 functions with
P/Invoke).  Function names, argument order and return conventions are the C-ABI's.

There is no fallback: if the shared library is missing this module raises, and if
no HIP device is present Raylib_Initialize returns 0 and Raylib_Render fails loudly.
"""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RAYLIB_LIB") or os.path.join(os.path.dirname(HERE), "libraylib.so")

RENDERMODE_DEFAULT, RENDERMODE_ALBEDO, RENDERMODE_SURFACE_NORMAL, RENDERMODE_MICROSURFACE_NORMAL, \
    RENDERMODE_TEXCOORD, RENDERMODE_EMISSION, RENDERMODE_REFLECTANCE = range(7)


class RendererSettings(C.Structure):
    """reference raylib_types.h:41-57 / RaylibWrapper.cs:27-38 (24 bytes)."""
    _fields_ = [("viewportWidth", C.c_uint32), ("viewportHeight", C.c_uint32),
                ("samplesPerPixel", C.c_int32), ("maxPathLength", C.c_int32),
                ("rayTMin", C.c_float), ("renderMode", C.c_uint32)]


class DenoiseParams(C.Structure):
    """include/raylib_amd.h RaylibAMDDenoiseParams."""
    _fields_ = [("iterations", C.c_int32), ("sigmaColor", C.c_float), ("sigmaNormal", C.c_float), ("sigmaAlbedo", C.c_float)]


class ProgressiveParams(C.Structure):
    """include/raylib_amd.h RaylibAMDProgressiveParams."""
    _fields_ = [("threshold", C.c_float), ("minSamples", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("nodesVisited", C.c_uint64), ("trisTested", C.c_uint64),
                ("shadedHits", C.c_uint64), ("texFetches", C.c_uint64), ("cameraSamples", C.c_uint64),
                ("pixels", C.c_uint64), ("kernelMs", C.c_double), ("traceKernelMs", C.c_double), ("wallMs", C.c_double),
                ("traceLaunches", C.c_uint32), ("numNodes", C.c_uint32), ("numTriangles", C.c_uint32), ("bvhDepth", C.c_uint32),
                ("waveTrips", C.c_uint64), ("pathsPerWave", C.c_uint32), ("ranks", C.c_uint32),
                ("gatherMode", C.c_uint32), ("rcclCommSize", C.c_uint32), ("devices", C.c_uint32), ("jobHeads", C.c_uint32),
                ("gatherMs", C.c_double), ("scatterMs", C.c_double), ("rankKernelMs", C.c_double * 16), ("rankTraceMs", C.c_double * 16),
                ("culledCells", C.c_uint32), ("listedCells", C.c_uint32), ("culledSamples", C.c_uint64), ("culledRays", C.c_uint64),
                ("treeWidth", C.c_uint32), ("nodeBytes", C.c_uint32), ("litPaths", C.c_uint64), ("litFoldedInPlace", C.c_uint64)]

    GATHER_MODES = {0: "none", 1: "rccl", 2: "peer"}

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["rankKernelMs"] = list(self.rankKernelMs)[: max(1, self.ranks)]
        d["rankTraceMs"] = list(self.rankTraceMs)[: max(1, self.ranks)]
        d["gatherMode"] = self.GATHER_MODES.get(self.gatherMode, "?")
        # the frame's totals, whatever share of it the kernels had to execute: equal with and without the silhouette cull (csrc/rl_cull.cc)
        d["frameSamples"] = self.cameraSamples + self.culledSamples
        d["frameRays"] = self.rays + self.culledRays
        d["frameNodes"] = self.nodesVisited + self.culledRays
        return d


class RenderPlan(C.Structure):
    """include/raylib_amd.h RaylibAMDRenderPlan."""
    _fields_ = [(k, C.c_int32) for k in ("pathTrace", "stack", "prims", "poolK", "tree", "lstack", "lds", "plain")] + \
               [(k, C.c_uint32) for k in ("pathsPerWave", "treeWidth", "nodeBytes")] + \
               [(k, C.c_int32) for k in ("keepNodes4", "keepNodes4f", "eagerTree")] + \
               [(k, C.c_uint32) for k in ("batch", "sampleCount", "blocks", "stackStride", "jobChunk", "heads", "jobsPerHead", "guideShift")] + \
               [("jobs", C.c_uint64), ("lazy", C.c_int32), ("hitQueue", C.c_int32)]
    TREES = {0: "none", 1: "bvh2", 2: "box4", 3: "grid4", 4: "wide8"}

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Ray(C.Structure):
    """include/raylib_amd.h RaylibAMDRay (32 bytes): org, tMin, dir, tMax."""
    _fields_ = [("org", C.c_float * 3), ("tMin", C.c_float), ("dir", C.c_float * 3), ("tMax", C.c_float)]


class HitT(C.Structure):
    """include/raylib_amd.h RaylibAMDHitT (16 bytes)."""
    _fields_ = [("t", C.c_float), ("prim", C.c_int32), ("b1", C.c_float), ("b2", C.c_float)]


class QueryPlan(C.Structure):
    """include/raylib_amd.h RaylibAMDQueryPlan."""
    _fields_ = [("tree", C.c_int32), ("treeWidth", C.c_uint32), ("nodeBytes", C.c_uint32), ("stack", C.c_int32), ("prims", C.c_int32), ("early", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


QUERY_ANY, QUERY_CLOSEST, QUERY_SURFACE = 0, 1, 2   # RAYLIB_AMD_QUERY_*
PRIM_SPHERE, PRIM_CUBE = 0x10000000, 0x20000000     # RAYLIB_AMD_PRIM_*
HITT_DTYPE = np.dtype([("t", "f4"), ("prim", "i4"), ("b1", "f4"), ("b2", "f4")])
SURFACE_DTYPE = np.dtype([("hit", "i4"), ("t", "f4"), ("p", "f4", 3), ("n", "f4", 3), ("paramU", "f4"), ("paramV", "f4"), ("material", "i4")])   # = RaylibAMD_ClosestHit's
_QUERY_DTYPES = {QUERY_ANY: np.dtype("u4"), QUERY_CLOSEST: HITT_DTYPE, QUERY_SURFACE: SURFACE_DTYPE}
_TORCH_WORDS = {QUERY_ANY: 1, QUERY_CLOSEST: 4, QUERY_SURFACE: 11}


def _plan(lib, entry, scene, *args):
    """A RaylibAMD_Plan* entry whose last argument is the plan: (return code, plan dict)."""
    p = QueryPlan()
    r = getattr(lib, entry)(scene, *args, C.byref(p))
    return r, p.as_dict()


def _ordered(stream):
    """The handle of a torch stream for a device entry.  The library reads handle 0 -- torch's default stream -- as its own stream, which is not ordered against
    torch's: that stream is synchronised first (the inputs may come from a copy just queued there, and the outputs' memory must be ready), and the call is synchronous."""
    if stream.cuda_stream == 0:
        stream.synchronize()
    return C.c_void_p(stream.cuda_stream)


def _query(lib, scene, data, cols, entry, specs, pre=(), mid=(), host=False, device=False, records=None, type_error="", host_error=None):
    """One query call, behind the public wrappers.  data: the input, `cols` float32 columns per record (a NumPy array of dtype `records` is taken as it stands).
    entry: the host-memory entry's name; entry + "Host" is its oracle and entry + "Device" the device entry, and all three take (scene, *pre, input, n, *mid,
    *outputs) -- the device entry then the stream.  specs(n): the outputs as (shape, NumPy dtype) pairs, None for one not asked for; a tensor has the shape with
    the record's 4-byte words as a last axis, int32 (float32 where a third element of the spec is True).
    A NumPy array goes through the host-memory entry (host=True: the oracle) and NumPy outputs come back; with device=True it is copied to the device, goes through
    the device entry, and the outputs are copied back.  A float32 torch tensor on the device goes through the device entry on torch.cuda.current_stream() and
    tensors come back: enqueued on a stream of the caller's, synchronous on torch's default stream (_ordered).  Returns the list of outputs; raises TypeError
    (type_error; host_error for host=True without a host array) and RuntimeError when the library refuses the call."""
    if isinstance(data, np.ndarray) and not device:
        d = np.ascontiguousarray(data)
        d = d.view(np.uint8).reshape(-1, records.itemsize) if records is not None and d.dtype == records else np.ascontiguousarray(d, np.float32).reshape(-1, cols)
        n = len(d)
        outs = [None if s is None else np.zeros(s[0], s[1]) for s in specs(n)]
        name = entry + "Host" if host else entry
        if getattr(lib, name)(scene, *pre, d.ctypes.data, n, *mid, *[None if o is None else o.ctypes.data for o in outs]) != 1:
            raise RuntimeError(name + " refused the query")
        return outs
    import torch
    if host:
        raise TypeError(host_error or type_error)
    as_numpy = isinstance(data, np.ndarray)
    if as_numpy:
        data = torch.from_numpy(np.ascontiguousarray(data, np.float32).reshape(-1, cols)).cuda()
    if not (isinstance(data, torch.Tensor) and data.is_cuda and data.dtype == torch.float32):
        raise TypeError(type_error)
    d = data.reshape(-1, cols).contiguous()
    n = d.shape[0]
    specs = specs(n)
    outs = []
    for s in specs:
        words = 0 if s is None else np.dtype(s[1]).itemsize // 4
        shape = None if s is None else (s[0] if isinstance(s[0], tuple) else (s[0],)) + ((words,) if words > 1 else ())
        outs.append(None if s is None else torch.empty(shape, dtype=torch.float32 if len(s) > 2 and s[2] else torch.int32, device=d.device))
    stream = torch.cuda.current_stream(d.device)
    if getattr(lib, entry + "Device")(scene, *pre, C.c_void_p(d.data_ptr()), n, *mid, *[None if o is None else C.c_void_p(o.data_ptr()) for o in outs], _ordered(stream)) != 1:
        raise RuntimeError(entry + "Device refused the query")
    if as_numpy:
        stream.synchronize()
        outs = [None if o is None else o.cpu().numpy().view(s[1]).reshape(s[0]) for o, s in zip(outs, specs)]
    return outs


_RAYS_TYPE_ERROR = "rays: a float32 NumPy array or a float32 torch tensor on the device"
_POINTS_TYPE_ERROR = "points: a float32 NumPy array, or a float32 torch tensor on the device (host=False)"
_QUERIES_TYPE_ERROR = "queries: a NumPy array, or a float32 torch tensor on the device (host=False)"


def plan_ray_query(lib, scene, kind):
    """RaylibAMD_PlanRayQuery: (return code, plan dict)."""
    return _plan(lib, "RaylibAMD_PlanRayQuery", scene, int(kind))


def trace_rays(lib, scene, rays, kind, ray_time=0.0, with_prim=False):
    """Batched ray queries (RaylibAMD_TraceRays / RaylibAMD_TraceRaysDevice).

    rays: an (n, 8) float32 array -- org xyz, tMin, dir xyz, tMax per row.  A NumPy array goes through the host entry and returns a NumPy array of
    the kind's records (uint32 for QUERY_ANY, HITT_DTYPE, SURFACE_DTYPE).  A torch tensor on the device goes through the device entry, ordered after
    the work already queued on torch.cuda.current_stream(): on a stream of the caller's the query is enqueued there and the call returns; on torch's
    default stream (whose handle is 0, which the library reads as its own stream) that stream is synchronised first and the call is synchronous.  It
    returns a tensor: (n,) int32 for QUERY_ANY (0 / 1), (n, 4) int32 words for QUERY_CLOSEST and (n, 11) int32 words for
    QUERY_SURFACE (reinterpret with .view(torch.float32) or move to NumPy and .view(HITT_DTYPE / SURFACE_DTYPE)).  with_prim (QUERY_SURFACE): also
    return the primitive of each ray as a second array / tensor.  Raises RuntimeError when the library refuses the call."""
    kind = int(kind)
    if kind not in _QUERY_DTYPES:
        raise ValueError("unknown query kind %r" % kind)
    want_prim = with_prim and kind == QUERY_SURFACE
    out, prim = _query(lib, scene, rays, 8, "RaylibAMD_TraceRays", lambda n: [(n, _QUERY_DTYPES[kind]), (n, np.int32) if want_prim else None],
                       pre=(kind,), mid=(float(ray_time),), type_error=_RAYS_TYPE_ERROR)
    return (out, prim) if with_prim else out


class GBufferPlanes(C.Structure):
    """include/raylib_amd.h RaylibAMDGBufferPlanes: a null pointer is a plane not asked for."""
    _fields_ = [(k, C.c_void_p) for k in ("hit", "surface", "albedo", "surfaceNormal", "microNormal", "texcoord", "emission")]


GBUFFER_PLANES = tuple(k for k, _ in GBufferPlanes._fields_)
_GBUFFER_DTYPES = {k: np.dtype("f4") for k in GBUFFER_PLANES}
_GBUFFER_DTYPES.update(hit=HITT_DTYPE, surface=SURFACE_DTYPE)


def plan_gbuffer(lib, scene):
    """RaylibAMD_PlanGBuffer: (return code, plan dict)."""
    return _plan(lib, "RaylibAMD_PlanGBuffer", scene)


def _gbuffer_names(planes):
    names = tuple(planes)
    for k in names:
        if k not in GBUFFER_PLANES:
            raise ValueError("unknown G-buffer plane %r" % (k,))
    return names


def gbuffer(lib, scene, camera, w, h, tmin=1e-4, planes=GBUFFER_PLANES):
    """The primary-hit G-buffer through the host entry (RaylibAMD_RenderGBuffer, statements G1 to G6): a dict of NumPy arrays, one per plane named in `planes` --
    hit (h, w) HITT_DTYPE, surface (h, w) SURFACE_DTYPE, the colour planes (h, w, 4) float32.  Raises RuntimeError when the library refuses the call."""
    names = _gbuffer_names(planes)
    out = {k: np.zeros((h, w) if k in ("hit", "surface") else (h, w, 4), _GBUFFER_DTYPES[k]) for k in names}
    st = RendererSettings(int(w), int(h), 1, 1, float(tmin), RENDERMODE_DEFAULT)
    p = GBufferPlanes(**{k: out[k].ctypes.data for k in names})
    if lib.RaylibAMD_RenderGBuffer(C.byref(st), scene, camera, C.byref(p)) != 1:
        raise RuntimeError("RaylibAMD_RenderGBuffer refused the call")
    return out


def gbuffer_device(lib, scene, camera, w, h, tmin=1e-4, planes=GBUFFER_PLANES, out=None):
    """The same through the device entry (RaylibAMD_RenderGBufferDevice) on torch.cuda.current_stream(), as trace_rays: enqueued on a stream of the caller's,
    synchronous on torch's default stream (synchronised first).  Returns a dict of tensors on the device: hit (h, w, 4) and surface (h, w, 11) int32 words
    (reinterpret with .view(torch.float32), or move to NumPy and .view(HITT_DTYPE / SURFACE_DTYPE)), the colour planes (h, w, 4) float32.  out: tensors of the
    caller's to write into, by plane name (contiguous, on the device).  Raises RuntimeError when the library refuses the call."""
    import torch
    names = _gbuffer_names(planes)
    res = {}
    for k in names:
        if out is not None and k in out:
            res[k] = out[k]
        elif k in ("hit", "surface"):
            res[k] = torch.empty((h, w, _GBUFFER_DTYPES[k].itemsize // 4), dtype=torch.int32, device="cuda")
        else:
            res[k] = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    st = RendererSettings(int(w), int(h), 1, 1, float(tmin), RENDERMODE_DEFAULT)
    p = GBufferPlanes(**{k: res[k].data_ptr() for k in names})
    if lib.RaylibAMD_RenderGBufferDevice(C.byref(st), scene, camera, C.byref(p), _ordered(torch.cuda.current_stream())) != 1:
        raise RuntimeError("RaylibAMD_RenderGBufferDevice refused the call")
    return res


def render_guides(lib, scene, camera, w, h, albedo, micro_normal, tmin=1e-4):
    """RaylibAMD_RenderGuides into image handles (either may be 0 / None): the denoiser's two guides in one launch.  Returns the library's return code."""
    st = RendererSettings(int(w), int(h), 1, 1, float(tmin), RENDERMODE_DEFAULT)
    return lib.RaylibAMD_RenderGuides(C.byref(st), scene, camera, albedo or None, micro_normal or None)


MOTION_NONE, MOTION_SURFACE, MOTION_SKY = 0, 1, 2   # RAYLIB_AMD_MOTION_*
MOTION_DTYPE = np.dtype([("prevX", "f4"), ("prevY", "f4"), ("prevT", "f4"), ("status", "u4")])


class MotionPlanes(C.Structure):
    """include/raylib_amd.h RaylibAMDMotionPlanes: a null pointer is a plane not asked for."""
    _fields_ = [("hit", C.c_void_p), ("motion", C.c_void_p)]


class MotionParams(C.Structure):
    """include/raylib_amd.h RaylibAMDMotionParams."""
    _fields_ = [("prevCamera", C.c_void_p), ("first", C.c_int32), ("count", C.c_int32), ("prevPositions", C.c_void_p)]


class TemporalParams(C.Structure):
    """include/raylib_amd.h RaylibAMDTemporalParams."""
    _fields_ = [("depthTolerance", C.c_float), ("maxLength", C.c_float)]


class TemporalFrame(C.Structure):
    """include/raylib_amd.h RaylibAMDTemporalFrame: the previous call's colour, that frame's hit plane, its length plane."""
    _fields_ = [("colour", C.c_void_p), ("hit", C.c_void_p), ("length", C.c_void_p)]


def plan_motion(lib, scene):
    """RaylibAMD_PlanMotion: (return code, plan dict)."""
    return _plan(lib, "RaylibAMD_PlanMotion", scene)


def _motion_names(planes):
    names = tuple(planes)
    for k in names:
        if k not in ("hit", "motion"):
            raise ValueError("unknown motion plane %r" % (k,))
    return names


def motion(lib, scene, camera, w, h, prev_camera=None, first=0, prev_positions=None, tmin=1e-4, planes=("hit", "motion")):
    """The motion plane and / or the hit plane through the host entry (RaylibAMD_RenderMotion, statements T1 to T6): a dict of NumPy arrays, hit (h, w) HITT_DTYPE
    and motion (h, w) MOTION_DTYPE.  prev_positions: (count, 9) float32, last frame's vertices of triangles [first, first + count), or None.  Raises
    RuntimeError when the library refuses the call."""
    names = _motion_names(planes)
    out = {k: np.zeros((h, w), HITT_DTYPE if k == "hit" else MOTION_DTYPE) for k in names}
    pp = None if prev_positions is None else np.ascontiguousarray(prev_positions, np.float32).reshape(-1, 9)
    prm = MotionParams(prev_camera or None, int(first), 0 if pp is None else len(pp), None if pp is None else pp.ctypes.data)
    st = RendererSettings(int(w), int(h), 1, 1, float(tmin), RENDERMODE_DEFAULT)
    p = MotionPlanes(**{k: out[k].ctypes.data for k in names})
    if lib.RaylibAMD_RenderMotion(C.byref(st), scene, camera, C.byref(prm), C.byref(p)) != 1:
        raise RuntimeError("RaylibAMD_RenderMotion refused the call")
    return out


def motion_device(lib, scene, camera, w, h, prev_camera=None, first=0, prev_positions=None, tmin=1e-4, planes=("hit", "motion"), out=None):
    """The same through the device entry (RaylibAMD_RenderMotionDevice) on torch.cuda.current_stream(), as gbuffer_device.  prev_positions: a contiguous float32
    tensor of count * 9 elements on the device, or None.  Returns a dict of (h, w, 4) int32 tensors on the device (move to NumPy and .view(HITT_DTYPE /
    MOTION_DTYPE)); out: tensors of the caller's to write into, by plane name.  Raises RuntimeError when the library refuses the call."""
    import torch
    names = _motion_names(planes)
    res = {k: out[k] if out is not None and k in out else torch.empty((h, w, 4), dtype=torch.int32, device="cuda") for k in names}
    count = 0 if prev_positions is None else prev_positions.numel() // 9
    prm = MotionParams(prev_camera or None, int(first), int(count), None if prev_positions is None else prev_positions.data_ptr())
    st = RendererSettings(int(w), int(h), 1, 1, float(tmin), RENDERMODE_DEFAULT)
    p = MotionPlanes(**{k: res[k].data_ptr() for k in names})
    if lib.RaylibAMD_RenderMotionDevice(C.byref(st), scene, camera, C.byref(prm), C.byref(p), _ordered(torch.cuda.current_stream())) != 1:
        raise RuntimeError("RaylibAMD_RenderMotionDevice refused the call")
    return res


def motion_host(lib, scene, camera, w, h, rays, hit, prev_camera=None, first=0, prev_positions=None):
    """RaylibAMD_MotionHost, the oracle of the motion plane: no device, no walk.  rays: (w * h, 7) float32 as RaylibAMD_EvalCameraRays returns them; hit: the
    frame's hit plane (HITT_DTYPE).  Returns (h, w) MOTION_DTYPE.  Raises RuntimeError when the library refuses the call."""
    rays = np.ascontiguousarray(rays, np.float32)
    hit = np.ascontiguousarray(hit, HITT_DTYPE)
    assert rays.size == w * h * 7 and hit.size == w * h
    out = np.zeros((h, w), MOTION_DTYPE)
    pp = None if prev_positions is None else np.ascontiguousarray(prev_positions, np.float32).reshape(-1, 9)
    prm = MotionParams(prev_camera or None, int(first), 0 if pp is None else len(pp), None if pp is None else pp.ctypes.data)
    if lib.RaylibAMD_MotionHost(int(w), int(h), scene, camera, C.byref(prm), rays.ctypes.data, hit.ctypes.data, out.ctypes.data) != 1:
        raise RuntimeError("RaylibAMD_MotionHost refused the call")
    return out


class TemporalMomentsFrame(C.Structure):
    """include/raylib_amd.h RaylibAMDTemporalMomentsFrame: a TemporalFrame and the previous call's moments plane."""
    _fields_ = [("colour", C.c_void_p), ("hit", C.c_void_p), ("length", C.c_void_p), ("moments", C.c_void_p)]


class VarianceFilterParams(C.Structure):
    """include/raylib_amd.h RaylibAMDVarianceFilterParams (a null pointer: 5, 4, 0.35, 0.1, 4)."""
    _fields_ = [("iterations", C.c_int32), ("sigmaLuminance", C.c_float), ("sigmaNormal", C.c_float), ("sigmaPlane", C.c_float), ("historyLength", C.c_float)]


class VarianceFilterPlanes(C.Structure):
    """include/raylib_amd.h RaylibAMDVarianceFilterPlanes: all five are required."""
    _fields_ = [("colour", C.c_void_p), ("moments", C.c_void_p), ("length", C.c_void_p), ("hit", C.c_void_p), ("surface", C.c_void_p)]


VARIANCE_DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.35, sigma_plane=0.1, history_length=4.0)
_TEMPORAL_PLANES = ((np.float32, 4), (HITT_DTYPE, 1), (MOTION_DTYPE, 1))            # colour, hit, motion
_HISTORY_PLANES = ((np.float32, 4), (HITT_DTYPE, 1), (np.float32, 1), (np.float32, 2))   # colour, hit, length, moments


def _planes(lib, entry, host, planes, kinds, outs, args):
    """One plane call on NumPy arrays, behind the public wrappers.  planes: the input arrays, kinds: each one's (dtype, elements per pixel); the first is the
    frame's colour, (h, w, 4).  entry: the host-memory entry's name, entry + "Host" its oracle; both take (w, h, *args(addresses of the planes), *outputs).
    outs: the outputs' shapes behind (h, w), None for one not asked for.  Returns the tuple of float32 outputs; raises RuntimeError on a refusal."""
    keep = [np.ascontiguousarray(a, d) for a, (d, _) in zip(planes, kinds)]
    h, w = keep[0].shape[:2]
    assert keep[0].shape == (h, w, 4) and all(a.size == w * h * k for a, (_, k) in zip(keep, kinds))
    res = tuple(None if s is None else np.zeros((h, w) + s, np.float32) for s in outs)
    name = entry + "Host" if host else entry
    if getattr(lib, name)(int(w), int(h), *args([a.ctypes.data for a in keep]), *[None if o is None else o.ctypes.data for o in res]) != 1:
        raise RuntimeError(name + " refused the call")
    return res


def _planes_device(lib, entry, colour, args, outs, out):
    """The same through the device entry (`entry`) on tensors, on torch.cuda.current_stream(): args are the entry's arguments between (w, h) and the outputs;
    out: the caller's output tensors, or None for fresh ones of the shapes `outs`."""
    import torch
    h, w = colour.shape[:2]
    res = tuple(out) if out is not None else tuple(None if s is None else torch.empty((h, w) + s, dtype=torch.float32, device="cuda") for s in outs)
    if getattr(lib, entry)(int(w), int(h), *args, *[None if o is None else o.data_ptr() for o in res], _ordered(torch.cuda.current_stream())) != 1:
        raise RuntimeError(entry + " refused the call")
    return res


def _accumulation(moments):
    """Entry, history structure (its fields are the planes a history has) and output shapes of the accumulation with or without the moments."""
    if moments:
        return "RaylibAMD_TemporalAccumulateMoments", TemporalMomentsFrame, ((4,), (), (2,))
    return "RaylibAMD_TemporalAccumulate", TemporalFrame, ((4,), ())


def _accumulate(lib, moments, host, colour, hit, motion, history, depth_tolerance, max_length):
    entry, frame, outs = _accumulation(moments)
    n = 0 if history is None else len(frame._fields_)
    prm = TemporalParams(float(depth_tolerance), float(max_length))
    return _planes(lib, entry, host, (colour, hit, motion) + (() if history is None else tuple(history)[:n]), _TEMPORAL_PLANES + _HISTORY_PLANES[:n], outs,
                   lambda p: (C.byref(prm), p[0], p[1], p[2], C.byref(frame(*p[3:])) if n else None))


def _accumulate_device(lib, moments, colour, hit, motion, history, depth_tolerance, max_length, out):
    entry, frame, outs = _accumulation(moments)
    hist = None if history is None else C.byref(frame(*[t.data_ptr() for t in history]))
    args = (C.byref(TemporalParams(float(depth_tolerance), float(max_length))), colour.data_ptr(), hit.data_ptr(), motion.data_ptr(), hist)
    return _planes_device(lib, entry + "Device", colour, args, outs, out)


def temporal_accumulate(lib, colour, hit, motion, history=None, depth_tolerance=0.02, max_length=32.0, host=False):
    """RaylibAMD_TemporalAccumulate on NumPy arrays (host=True: RaylibAMD_TemporalAccumulateHost, the oracle, no device): colour (h, w, 4) float32, hit (h, w)
    HITT_DTYPE, motion (h, w) MOTION_DTYPE, history None or the (colour, hit, length) of the previous frame.  Returns (outColour (h, w, 4), outLength (h, w)).
    Raises RuntimeError when the library refuses the call."""
    return _accumulate(lib, False, host, colour, hit, motion, history, depth_tolerance, max_length)


def temporal_accumulate_device(lib, colour, hit, motion, history=None, depth_tolerance=0.02, max_length=32.0, out=None):
    """RaylibAMD_TemporalAccumulateDevice on torch.cuda.current_stream(), as gbuffer_device: colour (h, w, 4) float32, hit and motion (h, w, 4) int32 as
    motion_device returns them, history None or (colour, hit, length) tensors of the previous frame; all contiguous, on the device.  out: (outColour, outLength)
    tensors to write into.  Returns (outColour (h, w, 4) float32, outLength (h, w) float32).  Raises RuntimeError when the library refuses the call."""
    return _accumulate_device(lib, False, colour, hit, motion, history, depth_tolerance, max_length, out)


def temporal_accumulate_moments(lib, colour, hit, motion, history=None, depth_tolerance=0.02, max_length=32.0, host=False):
    """RaylibAMD_TemporalAccumulateMoments on NumPy arrays (host=True: RaylibAMD_TemporalAccumulateMomentsHost, the oracle, no device): temporal_accumulate's
    arguments with a history of (colour, hit, length, moments), moments (h, w, 2) float32.  Returns (outColour (h, w, 4), outLength (h, w), outMoments (h, w, 2)).
    Raises RuntimeError when the library refuses the call."""
    return _accumulate(lib, True, host, colour, hit, motion, history, depth_tolerance, max_length)


def temporal_accumulate_moments_device(lib, colour, hit, motion, history=None, depth_tolerance=0.02, max_length=32.0, out=None):
    """RaylibAMD_TemporalAccumulateMomentsDevice on torch.cuda.current_stream(), as temporal_accumulate_device: history None or (colour, hit, length, moments)
    tensors of the previous frame; out: (outColour, outLength, outMoments) tensors to write into.  Returns (outColour (h, w, 4), outLength (h, w),
    outMoments (h, w, 2)), float32 on the device.  Raises RuntimeError when the library refuses the call."""
    return _accumulate_device(lib, True, colour, hit, motion, history, depth_tolerance, max_length, out)


def _variance_params(params):
    """None (the library's defaults: a null pointer) or a dict / VarianceFilterParams -> what the call is handed."""
    if params is None:
        return None
    if isinstance(params, VarianceFilterParams):
        return C.byref(params)
    p = dict(VARIANCE_DEFAULTS, **params)
    return C.byref(VarianceFilterParams(int(p["iterations"]), float(p["sigma_luminance"]), float(p["sigma_normal"]), float(p["sigma_plane"]), float(p["history_length"])))


def filter_variance(lib, colour, moments, length, hit, surface, params=None, variance=True, host=False):
    """RaylibAMD_FilterVariance on NumPy arrays (host=True: RaylibAMD_FilterVarianceHost, the oracle, no device): colour (h, w, 4), moments (h, w, 2) and length
    (h, w) float32 as the accumulation leaves them, hit (h, w) HITT_DTYPE and surface (h, w) SURFACE_DTYPE as the G-buffer does.  params: None for the library's
    defaults, or a dict with any of VARIANCE_DEFAULTS' keys.  Returns (outColour (h, w, 4), outVariance (h, w) or None when variance is False).  Raises
    RuntimeError when the library refuses the call."""
    kinds = ((np.float32, 4), (np.float32, 2), (np.float32, 1), (HITT_DTYPE, 1), (SURFACE_DTYPE, 1))
    return _planes(lib, "RaylibAMD_FilterVariance", host, (colour, moments, length, hit, surface), kinds, ((4,), () if variance else None),
                   lambda p: (_variance_params(params), C.byref(VarianceFilterPlanes(*p))))


def filter_variance_device(lib, colour, moments, length, hit, surface, params=None, variance=True, out=None):
    """RaylibAMD_FilterVarianceDevice on torch.cuda.current_stream(), as temporal_accumulate_device: float32 tensors colour (h, w, 4), moments (h, w, 2), length
    (h, w), and hit (h, w, 4), surface (h, w, 11) int32 words as gbuffer_device returns them; all contiguous, on the device.  out: (outColour, outVariance or
    None) tensors to write into.  Returns (outColour, outVariance or None).  Raises RuntimeError when the library refuses the call."""
    planes = VarianceFilterPlanes(colour.data_ptr(), moments.data_ptr(), length.data_ptr(), hit.data_ptr(), surface.data_ptr())
    return _planes_device(lib, "RaylibAMD_FilterVarianceDevice", colour, (_variance_params(params), C.byref(planes)), ((4,), () if variance else None), out)


MAX_HITS = 16                                       # RAYLIB_AMD_MAX_HITS


def plan_ray_query_all(lib, scene, max_hits, count=False):
    """RaylibAMD_PlanRayQueryAll: (return code, plan dict)."""
    return _plan(lib, "RaylibAMD_PlanRayQueryAll", scene, int(max_hits), int(bool(count)))


def _rows(max_hits, dtype, count, *more):
    """The outputs of a call that writes rows: (n, max_hits) records, whatever `more` gives per row entry, and the count per input when asked for."""
    k = max(max_hits, 0)
    return lambda n: [((n, k), dtype)] + [((n, k),) + m for m in more] + [(n, np.uint32) if count else None]


def trace_rays_all(lib, scene, rays, max_hits, count=False, tree=None, device=False, host=False, ray_time=0.0):
    """Ordered multi-hit ray queries (RaylibAMD_TraceRaysAll / RaylibAMD_TraceRaysAllDevice / RaylibAMD_TraceRaysAllHost, statements M1 to M5).

    rays: an (n, 8) float32 array -- org xyz, tMin, dir xyz, tMax per row.  Returns the (n, max_hits) records, and with count=True the pair (records, counts).
    A NumPy array goes through the host-memory entry (host=True: through the oracle, which needs no device) and returns NumPy arrays: HITT_DTYPE records, uint32
    counts.  A float32 torch tensor on the device -- or a NumPy array with device=True, which is copied there and whose results are copied back -- goes through
    the device entry on torch.cuda.current_stream(), as trace_rays: enqueued on a stream of the caller's, synchronous on torch's default stream (synchronised
    first); a tensor in gives tensors out, (n, max_hits, 4) int32 words and (n,) int32 counts.  tree: RAYLIB_QUERY_TREE for this call (2, 4 or 8; None leaves the
    environment alone).  Raises RuntimeError when the library refuses the call."""
    max_hits = int(max_hits)
    saved = os.environ.get("RAYLIB_QUERY_TREE")
    if tree is not None:
        os.environ["RAYLIB_QUERY_TREE"] = str(int(tree))
    try:
        hits, counts = _query(lib, scene, rays, 8, "RaylibAMD_TraceRaysAll", _rows(max_hits, HITT_DTYPE, count), mid=(float(ray_time), max_hits), host=host, device=device,
                              type_error=_RAYS_TYPE_ERROR, host_error="host=True takes a NumPy array and no device")
        return (hits, counts) if count else hits
    finally:
        if tree is not None:
            if saved is None:
                os.environ.pop("RAYLIB_QUERY_TREE", None)
            else:
                os.environ["RAYLIB_QUERY_TREE"] = saved


NEAREST_WITHIN, NEAREST_CLOSEST = 0, 1              # RAYLIB_AMD_NEAREST_*
NEAREST_QUERY_DTYPE = np.dtype([("pos", "f4", 3), ("maxDist", "f4")])                          # RaylibAMDNearestQuery
NEAREST_DTYPE = np.dtype([("dist2", "f4"), ("prim", "i4"), ("b1", "f4"), ("b2", "f4")])        # RaylibAMDNearestHit


def plan_nearest(lib, scene, kind):
    """RaylibAMD_PlanNearest: (return code, plan dict)."""
    return _plan(lib, "RaylibAMD_PlanNearest", scene, int(kind))


def nearest_points(lib, scene, points, kind, host=False):
    """Batched nearest-point queries (RaylibAMD_NearestPoints / RaylibAMD_NearestPointsDevice / RaylibAMD_NearestPointsHost).

    points: an (n, 4) float32 array -- pos xyz, maxDist per row.  A NumPy array goes through the host entry (host=True: through the oracle, which needs no
    device) and returns a NumPy array: uint32 for NEAREST_WITHIN, NEAREST_DTYPE for NEAREST_CLOSEST.  A float32 torch tensor on the device goes through the
    device entry on torch.cuda.current_stream(), as trace_rays: enqueued on a stream of the caller's, synchronous on torch's default stream (synchronised
    first).  It returns a tensor: (n,) int32 for WITHIN (0 / 1), (n, 4) int32 words for CLOSEST.  Raises RuntimeError when the library refuses the call."""
    kind = int(kind)
    if kind not in (NEAREST_WITHIN, NEAREST_CLOSEST):
        raise ValueError("unknown nearest kind %r" % kind)
    dtype = NEAREST_DTYPE if kind == NEAREST_CLOSEST else np.dtype("u4")
    return _query(lib, scene, points, 4, "RaylibAMD_NearestPoints", lambda n: [(n, dtype)], pre=(kind,), host=host, type_error=_POINTS_TYPE_ERROR)[0]


MAX_NEAREST = 16                                    # RAYLIB_AMD_MAX_NEAREST


def plan_nearest_all(lib, scene, max_hits, count=False):
    """RaylibAMD_PlanNearestAll: (return code, plan dict)."""
    return _plan(lib, "RaylibAMD_PlanNearestAll", scene, int(max_hits), int(bool(count)))


def nearest_points_all(lib, scene, points, max_hits, count=False, host=False):
    """The K nearest triangles and the count in range (RaylibAMD_NearestPointsAll / RaylibAMD_NearestPointsAllDevice / RaylibAMD_NearestPointsAllHost,
    statements K1 to K5).

    points: as nearest_points'.  Returns the (n, max_hits) rows, and with count=True the pair (rows, counts).  A NumPy array goes through the host entry
    (host=True: through the oracle, which needs no device) and returns NumPy arrays: NEAREST_DTYPE records, uint32 counts.  A float32 torch tensor on the
    device goes through the device entry on torch.cuda.current_stream(), as nearest_points; it returns tensors: (n, max_hits, 4) int32 words and (n,) int32
    counts.  Raises RuntimeError when the library refuses the call."""
    max_hits = int(max_hits)
    rows, counts = _query(lib, scene, points, 4, "RaylibAMD_NearestPointsAll", _rows(max_hits, NEAREST_DTYPE, count), mid=(max_hits,), host=host, type_error=_POINTS_TYPE_ERROR)
    return (rows, counts) if count else rows


SWEEP_ANY, SWEEP_CLOSEST = 0, 1                     # RAYLIB_AMD_SWEEP_*
SWEEP_QUERY_DTYPE = np.dtype([("origin", "f4", 3), ("radius", "f4"), ("delta", "f4", 3), ("reserved", "u4")])                                           # RaylibAMDSweepQuery
SWEEP_HIT_DTYPE = np.dtype([("t", "f4"), ("prim", "i4"), ("feature", "i4"), ("reserved0", "u4"), ("point", "f4", 3), ("reserved1", "u4")])   # RaylibAMDSweepHit


def plan_sweep(lib, scene, kind):
    """RaylibAMD_PlanSweep: (return code, plan dict)."""
    return _plan(lib, "RaylibAMD_PlanSweep", scene, int(kind))


def sweep_spheres(lib, scene, queries, kind, host=False):
    """Batched swept-sphere queries (RaylibAMD_SweepSpheres / RaylibAMD_SweepSpheresDevice / RaylibAMD_SweepSpheresHost, statements W1 to W7).

    queries: an (n, 8) float32 array -- origin xyz, radius, delta xyz and a word that is not read per row -- or a NumPy array of SWEEP_QUERY_DTYPE.  A NumPy
    array goes through the host entry (host=True: through the oracle, which needs no device) and returns a NumPy array: uint32 for SWEEP_ANY, SWEEP_HIT_DTYPE
    for SWEEP_CLOSEST.  A float32 torch tensor on the device goes through the device entry on torch.cuda.current_stream(), as nearest_points: enqueued on a
    stream of the caller's, synchronous on torch's default stream (synchronised first).  It returns a tensor: (n,) int32 for ANY (0 / 1), (n, 8) int32 words
    for CLOSEST.  Raises RuntimeError when the library refuses the call."""
    kind = int(kind)
    if kind not in (SWEEP_ANY, SWEEP_CLOSEST):
        raise ValueError("unknown sweep kind %r" % kind)
    dtype = SWEEP_HIT_DTYPE if kind == SWEEP_CLOSEST else np.dtype("u4")
    return _query(lib, scene, queries, 8, "RaylibAMD_SweepSpheres", lambda n: [(n, dtype)], pre=(kind,), host=host, records=SWEEP_QUERY_DTYPE, type_error=_QUERIES_TYPE_ERROR)[0]


SDF_UNSIGNED, SDF_SIGN_X, SDF_SIGN_Y, SDF_SIGN_Z, SDF_SIGN_MAJORITY = 0, 1, 2, 3, 4   # RAYLIB_AMD_SDF_*


class DistanceFieldParams(C.Structure):
    """include/raylib_amd.h RaylibAMDDistanceFieldParams."""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("dims", C.c_int32 * 3), ("maxDist", C.c_float), ("sign", C.c_int32)]


def distance_field_params(origin, spacing, dims, max_dist, sign):
    p = DistanceFieldParams()
    p.origin[:] = [float(x) for x in origin]
    p.spacing[:] = [float(x) for x in spacing]
    p.dims[:] = [int(x) for x in dims]
    p.maxDist = float(max_dist)
    p.sign = int(sign)
    return p


def plan_distance_field(lib, scene, origin, spacing, dims, max_dist, sign):
    """RaylibAMD_PlanDistanceField: (return code, the distance kernel's plan dict, the row kernel's plan dict)."""
    near, rows = QueryPlan(), QueryPlan()
    r = lib.RaylibAMD_PlanDistanceField(scene, C.byref(distance_field_params(origin, spacing, dims, max_dist, sign)), C.byref(near), C.byref(rows))
    return r, near.as_dict(), rows.as_dict()


def bake_distance_field(lib, scene, origin, spacing, dims, max_dist, sign, prim=False, host=False, device=False, stream=None):
    """A signed distance field on a regular grid (RaylibAMD_BakeDistanceField / RaylibAMD_BakeDistanceFieldDevice / RaylibAMD_BakeDistanceFieldHost, statements
    V1 to V7).

    dims = (nx, ny, nz); the result is indexed [k, j, i] (voxel (i, j, k) at (k * ny + j) * nx + i).  Returns the float32 distances, and with prim=True the pair
    (distances, int32 nearest-triangle indices).  By default the host-memory entry runs on the device and NumPy arrays come back; host=True goes through the
    oracle, which needs no device.  device=True goes through the device entry on torch tensors it allocates on the current device and returns them: enqueued on
    `stream` (a torch stream; None: torch.cuda.current_stream()), synchronous on torch's default stream (synchronised first), as nearest_points.  Raises
    RuntimeError when the library refuses the call."""
    p = distance_field_params(origin, spacing, dims, max_dist, sign)
    nx, ny, nz = (int(x) for x in dims)
    shape = (max(nz, 0), max(ny, 0), max(nx, 0))
    if not device:
        dist = np.zeros(shape, np.float32)
        prims = np.zeros(shape, np.int32) if prim else None
        name = "RaylibAMD_BakeDistanceFieldHost" if host else "RaylibAMD_BakeDistanceField"
        if getattr(lib, name)(scene, C.byref(p), dist.ctypes.data, prims.ctypes.data if prim else None) != 1:
            raise RuntimeError(name + " refused the bake")
        return (dist, prims) if prim else dist
    import torch
    if host:
        raise TypeError("host=True runs the oracle: no device entry")
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        dist = torch.empty(shape, dtype=torch.float32, device="cuda")
        prims = torch.empty(shape, dtype=torch.int32, device="cuda") if prim else None
    if lib.RaylibAMD_BakeDistanceFieldDevice(scene, C.byref(p), C.c_void_p(dist.data_ptr()), C.c_void_p(prims.data_ptr()) if prim else None, _ordered(st)) != 1:
        raise RuntimeError("RaylibAMD_BakeDistanceFieldDevice refused the bake")
    return (dist, prims) if prim else dist


OVERLAP_ANY, OVERLAP_LIST = 0, 1                    # RAYLIB_AMD_OVERLAP_*
OVERLAP_SKIP_SHARED = 1                             # RAYLIB_AMD_OVERLAP_SKIP_SHARED
MAX_OVERLAPS = 16                                   # RAYLIB_AMD_MAX_OVERLAPS
OVERLAP_QUERY_DTYPE = np.dtype([("v0", "f4", 3), ("reserved0", "u4"), ("v1", "f4", 3), ("reserved1", "u4"), ("v2", "f4", 3), ("reserved2", "u4")])   # RaylibAMDOverlapQuery


def overlap_queries(v0, v1, v2):
    """OVERLAP_QUERY_DTYPE records from three (n, 3) vertex arrays."""
    q = np.zeros(len(v0), OVERLAP_QUERY_DTYPE)
    q["v0"], q["v1"], q["v2"] = v0, v1, v2
    return q


def plan_overlap(lib, scene, kind):
    """RaylibAMD_PlanOverlap: (return code, plan dict)."""
    return _plan(lib, "RaylibAMD_PlanOverlap", scene, int(kind))


def overlap_triangles(lib, scene, queries, kind, flags=0, max_hits=MAX_OVERLAPS, host=False, count=True):
    """Batched triangle-overlap queries (RaylibAMD_OverlapTriangles / RaylibAMD_OverlapTrianglesDevice / RaylibAMD_OverlapTrianglesHost, statements O1 to O6).

    queries: OVERLAP_QUERY_DTYPE records (or an (n, 12) float32 array of the same 48 bytes).  A NumPy array goes through the host entry (host=True: through the
    oracle, which needs no device) and returns NumPy arrays: uint32 words for OVERLAP_ANY; for OVERLAP_LIST the (n, max_hits) int32 rows, and with count=True the
    pair (rows, uint32 counts).  An (n, 12) float32 torch tensor on the device goes through the device entry on torch.cuda.current_stream(), as nearest_points:
    enqueued on a stream of the caller's, synchronous on torch's default stream (synchronised first); it returns int32 tensors of the same shapes.  Raises
    RuntimeError when the library refuses the call."""
    kind, flags, max_hits = int(kind), int(flags), int(max_hits)
    if kind not in (OVERLAP_ANY, OVERLAP_LIST):
        raise ValueError("unknown overlap kind %r" % kind)
    want_count = kind == OVERLAP_LIST and count
    specs = _rows(max_hits, np.int32, want_count) if kind == OVERLAP_LIST else (lambda n: [(n, np.uint32), None])
    out, counts = _query(lib, scene, queries, 12, "RaylibAMD_OverlapTriangles", specs, pre=(kind, flags), mid=(max_hits,), host=host, records=OVERLAP_QUERY_DTYPE,
                         type_error=_QUERIES_TYPE_ERROR)
    return (out, counts) if want_count else out


CONTACT_NONE, CONTACT_SEGMENT, CONTACT_GAP, CONTACT_NO_CROSSING = 0, 1, 2, 3        # RAYLIB_AMD_CONTACT_*
CONTACT_DTYPE = np.dtype([("p0", "f4", 3), ("kind", "u4"), ("p1", "f4", 3), ("features", "u4")])   # RaylibAMDContact


def plan_overlap_contacts(lib, scene):
    """RaylibAMD_PlanOverlapContacts: (return code, plan dict)."""
    return _plan(lib, "RaylibAMD_PlanOverlapContacts", scene)


def overlap_contacts(lib, scene, queries, flags=0, max_hits=MAX_OVERLAPS, host=False, count=True):
    """The overlapping pairs of OVERLAP_LIST and the segment along which each pair crosses (RaylibAMD_OverlapContacts / RaylibAMD_OverlapContactsDevice /
    RaylibAMD_OverlapContactsHost, statements C1 to C6).

    queries: as overlap_triangles.  A NumPy array goes through the host entry (host=True: through the oracle, which needs no device) and returns
    (rows, contacts, counts): (n, max_hits) int32, (n, max_hits) CONTACT_DTYPE records, n uint32 (None with count=False).  An (n, 12) float32 torch tensor on the
    device goes through the device entry on torch.cuda.current_stream(), as overlap_triangles; the contacts are then an (n, max_hits, 8) float32 tensor of the
    same 32 bytes per record (kind and features: .view(torch.int32)[..., 3] and [..., 7]).  Raises RuntimeError when the library refuses the call."""
    flags, max_hits = int(flags), int(max_hits)
    return tuple(_query(lib, scene, queries, 12, "RaylibAMD_OverlapContacts", _rows(max_hits, np.int32, count, (CONTACT_DTYPE, True)), pre=(flags,), mid=(max_hits,),
                        host=host, records=OVERLAP_QUERY_DTYPE, type_error=_QUERIES_TYPE_ERROR))


BOX_ANY, BOX_LIST, BOX_MARK = 0, 1, 2               # RAYLIB_AMD_BOX_*
BOX_QUERY_DTYPE = np.dtype([("center", "f4", 3), ("reserved", "u4"), ("axis", [("dir", "f4", 3), ("half", "f4")], 3)])   # RaylibAMDBoxQuery


def box_queries(center, half, axes=None):
    """BOX_QUERY_DTYPE records from (n, 3) centres, (n, 3) half extents and (n, 3, 3) axes (row k: axis k's direction; None: the identity, axis-aligned boxes)."""
    q = np.zeros(len(center), BOX_QUERY_DTYPE)
    q["center"] = center
    q["axis"]["dir"] = np.eye(3, dtype=np.float32) if axes is None else axes
    q["axis"]["half"] = half
    return q


def plan_overlap_boxes(lib, scene, kind):
    """RaylibAMD_PlanOverlapBoxes: (return code, plan dict)."""
    return _plan(lib, "RaylibAMD_PlanOverlapBoxes", scene, int(kind))


def overlap_boxes(lib, scene, q, kind, k=MAX_OVERLAPS, count=True, host=False):
    """Oriented-box range queries (RaylibAMD_OverlapBoxes / RaylibAMD_OverlapBoxesDevice / RaylibAMD_OverlapBoxesHost, statements B1 to B6).

    q: BOX_QUERY_DTYPE records (or an (n, 16) float32 array of the same 64 bytes).  A NumPy array goes through the host entry (host=True: through the oracle,
    which needs no device) and returns NumPy arrays: uint32 words for BOX_ANY; for BOX_LIST the (n, k) int32 rows, and with count=True the pair (rows, uint32
    counts); for BOX_MARK the call's mask, (numTriangles + 31) // 32 uint32 words.  An (n, 16) float32 torch tensor on the device goes through the device entry
    on torch.cuda.current_stream(), as overlap_triangles: enqueued on a stream of the caller's, synchronous on torch's default stream (synchronised first); it
    returns int32 tensors of the same shapes.  Raises RuntimeError when the library refuses the call."""
    kind, k = int(kind), int(k)
    if kind not in (BOX_ANY, BOX_LIST, BOX_MARK):
        raise ValueError("unknown box kind %r" % kind)
    want_count = kind == BOX_LIST and count
    if kind == BOX_LIST:
        specs = _rows(k, np.int32, want_count)
    elif kind == BOX_MARK:
        words = (lib.RaylibAMD_SceneNumTriangles(scene) + 31) // 32
        specs = lambda n: [(words, np.uint32), None]
    else:
        specs = lambda n: [(n, np.uint32), None]
    out, counts = _query(lib, scene, q, 16, "RaylibAMD_OverlapBoxes", specs, pre=(kind,), mid=(k,), host=host, records=BOX_QUERY_DTYPE, type_error=_QUERIES_TYPE_ERROR)
    return (out, counts) if want_count else out


def move_triangles(lib, scene, first, positions, normals=None):
    """Move triangles [first, first + n) of a finalized scene (RaylibAMD_SceneMoveTriangles / RaylibAMD_SceneMoveTrianglesDevice).

    positions: (n, 9) float32 -- v0 v1 v2 per triangle, RaylibAMD_SceneExportTriangles order; normals: the same shape (n0 n1 n2), or None to keep the shading
    normals.  NumPy arrays go through the host entry (synchronous).  float32 torch tensors on the device go through the device entry on
    torch.cuda.current_stream(), as trace_rays: enqueued on a stream of the caller's, synchronous on torch's default stream (synchronised first).
    Returns the library's answer: 1, or 0 when it refuses the move (nothing changed)."""
    if isinstance(positions, np.ndarray):
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
        nr = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 9)
        if nr is not None and len(nr) != len(p):
            raise ValueError("normals: one row per row of positions")
        return lib.RaylibAMD_SceneMoveTriangles(scene, int(first), len(p), _fp(p), None if nr is None else _fp(nr))
    import torch
    ok = lambda t: isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
    if not ok(positions) or not (normals is None or ok(normals)):
        raise TypeError("positions / normals: float32 NumPy arrays, or float32 torch tensors on the device")
    p = positions.reshape(-1, 9).contiguous()
    nr = None if normals is None else normals.reshape(-1, 9).contiguous()
    if nr is not None and nr.shape[0] != p.shape[0]:
        raise ValueError("normals: one row per row of positions")
    stream = torch.cuda.current_stream(p.device)
    if stream.cuda_stream == 0:
        stream.synchronize()   # (the library's stream is not ordered against torch's default stream: trace_rays)
    return lib.RaylibAMD_SceneMoveTrianglesDevice(scene, int(first), p.shape[0], C.c_void_p(p.data_ptr()), None if nr is None else C.c_void_p(nr.data_ptr()),
                                                  C.c_void_p(stream.cuda_stream))


def compare_trees(lib, scene):
    """RaylibAMD_SceneCompareTrees: (the library's answer, the mask of formats that differ -- 1 float-4, 2 grid-4, 4 leaf list, 8 8-wide, 16 records).
    (1, 0): every wide tree the device holds is, byte for byte, what the host's rule makes of the device's binary boxes; (0, 0): the check could not run."""
    mask = C.c_uint32(0)
    return lib.RaylibAMD_SceneCompareTrees(scene, C.byref(mask)), mask.value


class PathRay(C.Structure):
    """include/raylib_amd.h RaylibAMDPathRay (32 bytes): org, time, dir, stream."""
    _fields_ = [("org", C.c_float * 3), ("time", C.c_float), ("dir", C.c_float * 3), ("stream", C.c_uint32)]


class RadianceParams(C.Structure):
    """include/raylib_amd.h RaylibAMDRadianceParams."""
    _fields_ = [("maxPathLength", C.c_int32), ("rayTMin", C.c_float), ("sampleFirst", C.c_uint32), ("sampleCount", C.c_uint32),
                ("skipDraws", C.c_uint32), ("timeMin", C.c_float), ("timeMax", C.c_float)]


def plan_radiance(lib, scene, max_path=5, tmin=1e-4, sample_first=0, sample_count=1, skip_draws=3):
    """RaylibAMD_PlanRadiance: (return code, plan dict)."""
    prm = RadianceParams(int(max_path), float(tmin), int(sample_first), int(sample_count), int(skip_draws), 0.0, 0.0)
    return _plan(lib, "RaylibAMD_PlanRadiance", scene, C.byref(prm))


def trace_radiance(lib, scene, rays, max_path=5, tmin=1e-4, sample_first=0, sample_count=1, skip_draws=3):
    """Path-traced radiance along caller rays (RaylibAMD_TraceRadiance / RaylibAMD_TraceRadianceDevice).

    rays: (n, 8) float32 -- org xyz, time, dir xyz, and the stream index as the uint32 whose bits the last column holds (rays[:, 7].view(uint32)).
    A NumPy array goes through the host entry and returns an (n, 4) float32 array.  A float32 torch tensor on the device goes through the device entry,
    ordered after the work already queued on torch.cuda.current_stream() (on torch's default stream, whose handle the library reads as its own stream,
    that stream is synchronised first and the call is synchronous); the time interval handed to the library is the tensor's own minimum and maximum.  It
    returns an (n, 4) float32 tensor.  Raises RuntimeError when the library refuses the call."""
    prm = RadianceParams(int(max_path), float(tmin), int(sample_first), int(sample_count), int(skip_draws), 0.0, 0.0)
    if isinstance(rays, np.ndarray):
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(r)
        out = np.zeros((n, 4), np.float32)
        ok = lib.RaylibAMD_TraceRadiance(scene, C.byref(prm), r.ctypes.data_as(C.POINTER(PathRay)), n, out.ctypes.data_as(C.POINTER(C.c_float)))
        if ok != 1:
            raise RuntimeError("RaylibAMD_TraceRadiance refused the call")
        return out
    import torch
    if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32):
        raise TypeError("rays: a float32 NumPy array or a float32 torch tensor on the device")
    r = rays.reshape(-1, 8).contiguous()
    n = r.shape[0]
    out = torch.empty((n, 4), dtype=torch.float32, device=r.device)
    if n:
        prm.timeMin, prm.timeMax = float(r[:, 3].min()), float(r[:, 3].max())
    stream = torch.cuda.current_stream(r.device)
    if stream.cuda_stream == 0:
        stream.synchronize()   # (as trace_rays: the library's stream is not ordered against torch's default stream)
    ok = lib.RaylibAMD_TraceRadianceDevice(scene, C.byref(prm), C.cast(C.c_void_p(r.data_ptr()), C.POINTER(PathRay)), n,
                                           C.cast(C.c_void_p(out.data_ptr()), C.POINTER(C.c_float)), C.c_void_p(stream.cuda_stream))
    if ok != 1:
        raise RuntimeError("RaylibAMD_TraceRadianceDevice refused the call")
    return out


class GatherPoint(C.Structure):
    """include/raylib_amd.h RaylibAMDGatherPoint (32 bytes): pos, time, normal, stream."""
    _fields_ = [("pos", C.c_float * 3), ("time", C.c_float), ("normal", C.c_float * 3), ("stream", C.c_uint32)]


class GatherParams(C.Structure):
    """include/raylib_amd.h RaylibAMDGatherParams."""
    _fields_ = [("kind", C.c_int32), ("maxPathLength", C.c_int32), ("rayTMin", C.c_float), ("sampleFirst", C.c_uint32), ("sampleCount", C.c_uint32),
                ("skipDraws", C.c_uint32), ("timeMin", C.c_float), ("timeMax", C.c_float)]


class GatherCut(C.Structure):
    """include/raylib_amd.h RaylibAMDGatherCut."""
    _fields_ = [("pointsPerLaunch", C.c_uint32), ("samplesPerLaunch", C.c_uint32), ("pointRanges", C.c_uint64), ("sampleRanges", C.c_uint64), ("launches", C.c_uint64),
                ("pointFirst", C.c_uint32), ("numPoints", C.c_uint32), ("sampleBase", C.c_uint32), ("numSamples", C.c_uint32), ("first", C.c_int32), ("last", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def plan_gather_cut(lib, kind, n, sample_count, launch=0):
    """RaylibAMD_PlanGatherCut: the cut of n points x sample_count samples into launches and launch `launch` of it, as a dict; None when the call refuses."""
    prm = GatherParams(int(kind), 5, 1e-4, 0, int(sample_count), 0, 0.0, 0.0)
    c = GatherCut()
    return c.as_dict() if lib.RaylibAMD_PlanGatherCut(C.byref(prm), int(n), int(launch), C.byref(c)) == 1 else None


GATHER_IRRADIANCE, GATHER_SH9 = 0, 1                  # RAYLIB_AMD_GATHER_*
_GATHER_FLOATS = {GATHER_IRRADIANCE: 4, GATHER_SH9: 27}


def gather(lib, scene, points, kind, max_path=5, tmin=1e-4, sample_first=0, sample_count=1, skip_draws=0):
    """Irradiance or SH9 probes gathered at points (RaylibAMD_Gather / RaylibAMD_GatherDevice).

    points: (n, 8) float32 -- pos xyz, time, normal xyz, and the stream index as the uint32 whose bits the last column holds.  A NumPy array goes through the
    host entry and returns an (n, 4) (GATHER_IRRADIANCE) or (n, 27) (GATHER_SH9) float32 array; a float32 torch tensor on the device goes through the device
    entry under the rules of trace_radiance and returns a tensor of that shape.  Raises RuntimeError when the library refuses the call."""
    kind = int(kind)
    if kind not in _GATHER_FLOATS:
        raise ValueError("unknown gather kind %r" % kind)
    prm = GatherParams(kind, int(max_path), float(tmin), int(sample_first), int(sample_count), int(skip_draws), 0.0, 0.0)
    if isinstance(points, np.ndarray):
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 8)
        n = len(p)
        out = np.zeros((n, _GATHER_FLOATS[kind]), np.float32)
        ok = lib.RaylibAMD_Gather(scene, C.byref(prm), p.ctypes.data_as(C.POINTER(GatherPoint)), n, out.ctypes.data_as(C.POINTER(C.c_float)))
        if ok != 1:
            raise RuntimeError("RaylibAMD_Gather refused the call")
        return out
    import torch
    if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float32):
        raise TypeError("points: a float32 NumPy array or a float32 torch tensor on the device")
    p = points.reshape(-1, 8).contiguous()
    n = p.shape[0]
    out = torch.empty((n, _GATHER_FLOATS[kind]), dtype=torch.float32, device=p.device)
    if n:
        prm.timeMin, prm.timeMax = float(p[:, 3].min()), float(p[:, 3].max())
    stream = torch.cuda.current_stream(p.device)
    if stream.cuda_stream == 0:
        stream.synchronize()   # (as trace_rays: the library's stream is not ordered against torch's default stream)
    ok = lib.RaylibAMD_GatherDevice(scene, C.byref(prm), C.cast(C.c_void_p(p.data_ptr()), C.POINTER(GatherPoint)), n,
                                    C.cast(C.c_void_p(out.data_ptr()), C.POINTER(C.c_float)), C.c_void_p(stream.cuda_stream))
    if ok != 1:
        raise RuntimeError("RaylibAMD_GatherDevice refused the call")
    return out


def gather_directions_host(lib, points, kind, seed, sample=0, sample_first=0, skip_draws=0):
    """RaylibAMD_GatherDirectionsHost: the direction of sample `sample` of every point, (n, 3) float32, with the host's libm; no device."""
    prm = GatherParams(int(kind), 0, 0.0, int(sample_first), 1, int(skip_draws), 0.0, 0.0)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 8)
    out = np.zeros((len(p), 3), np.float32)
    ok = lib.RaylibAMD_GatherDirectionsHost(C.byref(prm), p.ctypes.data_as(C.POINTER(GatherPoint)), len(p), int(seed), int(sample), out.ctypes.data_as(C.POINTER(C.c_float)))
    if ok != 1:
        raise RuntimeError("RaylibAMD_GatherDirectionsHost refused the call")
    return out


class LightmapParams(C.Structure):
    """include/raylib_amd.h RaylibAMDLightmapParams."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("triFirst", C.c_int32), ("triCount", C.c_int32), ("dilate", C.c_int32), ("time", C.c_float),
                ("gather", GatherParams)]


class LightmapFilterParams(C.Structure):
    """include/raylib_amd.h RaylibAMDLightmapFilterParams."""
    _fields_ = [("iterations", C.c_int32), ("sigmaColor", C.c_float), ("sigmaNormal", C.c_float), ("sigmaPosition", C.c_float)]


def lightmap_filter_params(filter):
    """A LightmapFilterParams, or an (iterations, sigmaColor, sigmaNormal, sigmaPosition) tuple made into one."""
    if isinstance(filter, LightmapFilterParams):
        return filter
    k, sc, sn, sp = filter
    return LightmapFilterParams(int(k), float(sc), float(sn), float(sp))


def lightmap_params(w, h, kind=GATHER_IRRADIANCE, tri_first=0, tri_count=-1, dilate=0, time=0.0, max_path=5, tmin=1e-4, sample_first=0, sample_count=1, skip_draws=0):
    return LightmapParams(int(w), int(h), int(tri_first), int(tri_count), int(dilate), float(time),
                          GatherParams(int(kind), int(max_path), float(tmin), int(sample_first), int(sample_count), int(skip_draws), 0.0, 0.0))


def _uv_host(uv):
    if uv is None:
        return None, None
    a = np.ascontiguousarray(uv, np.float32).reshape(-1, 6)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def lightmap_points(lib, scene, w, h, uv=None, tri_first=0, tri_count=-1, time=0.0, host=False, capacity=None):
    """The gather points of the atlas' covered texels (RaylibAMD_LightmapPoints, or with host=True the oracle RaylibAMD_LightmapPointsHost).

    uv: None (the triangles' own) or (triangles of the range, 6) float32.  Returns (points (n, 8) float32 as binding.gather takes them, texel indices (n,) uint32,
    count); n = min(count, capacity), capacity defaulting to the atlas' texels.  Raises RuntimeError when the library refuses the call."""
    prm = lightmap_params(w, h, tri_first=tri_first, tri_count=tri_count, time=time)
    cap = int(w) * int(h) if capacity is None else int(capacity)
    keep, uvp = _uv_host(uv)
    pts = np.zeros((max(cap, 1), 8), np.float32)
    tex = np.zeros(max(cap, 1), np.uint32)
    fn = lib.RaylibAMD_LightmapPointsHost if host else lib.RaylibAMD_LightmapPoints
    n = fn(scene, C.byref(prm), uvp, pts.ctypes.data_as(C.POINTER(GatherPoint)), tex.ctypes.data_as(C.POINTER(C.c_uint32)), cap)
    if n < 0:
        raise RuntimeError("%s refused the call" % ("RaylibAMD_LightmapPointsHost" if host else "RaylibAMD_LightmapPoints"))
    k = min(int(n), cap)
    return pts[:k], tex[:k], int(n)


def bake_lightmap(lib, scene, w, h, uv=None, kind=GATHER_IRRADIANCE, tri_first=0, tri_count=-1, dilate=0, time=0.0, max_path=5, tmin=1e-4, sample_first=0,
                  sample_count=1, skip_draws=0, device=None, filter=None):
    """A lightmap of the scene's triangles (RaylibAMD_BakeLightmap / RaylibAMD_BakeLightmapDevice): (atlas (H, W, C) float32, coverage (H, W) uint8), C = 4 or 27.
    filter: None, or (iterations, sigmaColor, sigmaNormal, sigmaPosition) -- the edge-avoiding atlas filter between the gather and the dilation
    (RaylibAMD_BakeLightmapFiltered / RaylibAMD_BakeLightmapFilteredDevice).

    uv: None, a NumPy array (triangles of the range, 6) -- the host entry, NumPy results -- or a float32 torch tensor on the device -- the device entry on
    torch's current stream, torch results.  device: a torch device, for the device entry with uv=None.  Raises RuntimeError when the library refuses the call."""
    kind = int(kind)
    if kind not in _GATHER_FLOATS:
        raise ValueError("unknown gather kind %r" % kind)
    c = _GATHER_FLOATS[kind]
    prm = lightmap_params(w, h, kind, tri_first, tri_count, dilate, time, max_path, tmin, sample_first, sample_count, skip_draws)
    flt = None if filter is None else lightmap_filter_params(filter)
    if device is None and (uv is None or isinstance(uv, np.ndarray)):
        keep, uvp = _uv_host(uv)
        out = np.zeros((int(h), int(w), c), np.float32)
        cov = np.zeros((int(h), int(w)), np.uint8)
        outp, covp = out.ctypes.data_as(C.POINTER(C.c_float)), cov.ctypes.data_as(C.POINTER(C.c_uint8))
        if flt is not None:
            if lib.RaylibAMD_BakeLightmapFiltered(scene, C.byref(prm), C.byref(flt), uvp, outp, covp) != 1:
                raise RuntimeError("RaylibAMD_BakeLightmapFiltered refused the call")
        elif lib.RaylibAMD_BakeLightmap(scene, C.byref(prm), uvp, outp, covp) != 1:
            raise RuntimeError("RaylibAMD_BakeLightmap refused the call")
        return out, cov
    import torch
    if uv is not None:
        if not (isinstance(uv, torch.Tensor) and uv.is_cuda and uv.dtype == torch.float32):
            raise TypeError("uv: None, a float32 NumPy array or a float32 torch tensor on the device")
        uv = uv.reshape(-1, 6).contiguous()
        device = uv.device
    out = torch.empty((int(h), int(w), c), dtype=torch.float32, device=device)
    cov = torch.empty((int(h), int(w)), dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(out.device)
    if stream.cuda_stream == 0:
        stream.synchronize()   # (as gather: the library's stream is not ordered against torch's default stream)
    uvp = C.cast(C.c_void_p(uv.data_ptr()), C.POINTER(C.c_float)) if uv is not None else None
    outp, covp = C.cast(C.c_void_p(out.data_ptr()), C.POINTER(C.c_float)), C.cast(C.c_void_p(cov.data_ptr()), C.POINTER(C.c_uint8))
    if flt is not None:
        if lib.RaylibAMD_BakeLightmapFilteredDevice(scene, C.byref(prm), C.byref(flt), uvp, outp, covp, C.c_void_p(stream.cuda_stream)) != 1:
            raise RuntimeError("RaylibAMD_BakeLightmapFilteredDevice refused the call")
    elif lib.RaylibAMD_BakeLightmapDevice(scene, C.byref(prm), uvp, outp, covp, C.c_void_p(stream.cuda_stream)) != 1:
        raise RuntimeError("RaylibAMD_BakeLightmapDevice refused the call")
    return out, cov


def filter_lightmap(lib, scene, w, h, atlas, filter, uv=None, kind=GATHER_IRRADIANCE, tri_first=0, tri_count=-1, dilate=0, time=0.0, out=None):
    """An atlas the caller has, filtered again and dilated (RaylibAMD_FilterLightmap / RaylibAMD_FilterLightmapDevice): (atlas (H, W, C), coverage (H, W) uint8).

    atlas: (H, W, C) float32, a NumPy array -- the host entry, uv None or a NumPy array, NumPy results -- or a torch tensor on the device -- the device entry on
    torch's current stream, uv None or a device tensor, torch results.  out: None (a new array) or where the atlas goes; it may be `atlas`.  filter:
    (iterations, sigmaColor, sigmaNormal, sigmaPosition).  Raises RuntimeError when the library refuses the call."""
    kind = int(kind)
    if kind not in _GATHER_FLOATS:
        raise ValueError("unknown gather kind %r" % kind)
    c, w, h = _GATHER_FLOATS[kind], int(w), int(h)
    prm = lightmap_params(w, h, kind, tri_first, tri_count, dilate, time)
    flt = lightmap_filter_params(filter)
    if isinstance(atlas, np.ndarray):
        if atlas.dtype != np.float32 or atlas.size != h * w * c or not atlas.flags.c_contiguous:
            raise TypeError("atlas: a contiguous float32 array of H x W x C")
        keep, uvp = _uv_host(uv)
        if out is None:
            out = np.zeros((h, w, c), np.float32)
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.size == h * w * c and out.flags.c_contiguous):
            raise TypeError("out: a contiguous float32 array of H x W x C")
        cov = np.zeros((h, w), np.uint8)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        if lib.RaylibAMD_FilterLightmap(scene, C.byref(prm), C.byref(flt), uvp, fp(atlas), fp(out), cov.ctypes.data_as(C.POINTER(C.c_uint8))) != 1:
            raise RuntimeError("RaylibAMD_FilterLightmap refused the call")
        return out, cov
    import torch
    ok_t = lambda t: isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    if not (ok_t(atlas) and atlas.numel() == h * w * c):
        raise TypeError("atlas: a contiguous float32 NumPy array or torch tensor on the device, H x W x C")
    if uv is not None:
        if not (isinstance(uv, torch.Tensor) and uv.is_cuda and uv.dtype == torch.float32):
            raise TypeError("uv: None or a float32 torch tensor on the atlas' device")
        uv = uv.reshape(-1, 6).contiguous()
    if out is None:
        out = torch.empty((h, w, c), dtype=torch.float32, device=atlas.device)
    if not (ok_t(out) and out.numel() == h * w * c):
        raise TypeError("out: a contiguous float32 torch tensor on the device, H x W x C")
    cov = torch.empty((h, w), dtype=torch.uint8, device=atlas.device)
    stream = torch.cuda.current_stream(atlas.device)
    if stream.cuda_stream == 0:
        stream.synchronize()   # (as gather: the library's stream is not ordered against torch's default stream)
    fp = lambda t: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_float))
    ok = lib.RaylibAMD_FilterLightmapDevice(scene, C.byref(prm), C.byref(flt), fp(uv) if uv is not None else None, fp(atlas), fp(out),
                                            C.cast(C.c_void_p(cov.data_ptr()), C.POINTER(C.c_uint8)), C.c_void_p(stream.cuda_stream))
    if ok != 1:
        raise RuntimeError("RaylibAMD_FilterLightmapDevice refused the call")
    return out, cov


def filter_lightmap_host(lib, w, h, kind, filter, points, texel, values, in_place=False):
    """RaylibAMD_FilterLightmapHost: the filter alone on the host, in compacted form -- points (n, 8) and texel (n,) as lightmap_points returns them, values (n, C)
    float32; returns the filtered (n, C) float32 (in_place: written over `values`, which must then be a contiguous float32 array).  No device, no scene."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 8)
    t = np.ascontiguousarray(texel, np.uint32).reshape(-1)
    v = values if in_place else np.ascontiguousarray(values, np.float32)
    if in_place and not (isinstance(v, np.ndarray) and v.dtype == np.float32 and v.flags.c_contiguous):
        raise TypeError("values: a contiguous float32 array for in_place")
    n = len(t)
    if int(kind) not in _GATHER_FLOATS:
        raise ValueError("unknown gather kind %r" % kind)
    if len(p) != n or v.size != n * _GATHER_FLOATS[int(kind)]:
        raise ValueError("points, texel and values do not describe the same number of texels")
    out = v if in_place else np.zeros_like(v)
    flt = lightmap_filter_params(filter)
    ok = lib.RaylibAMD_FilterLightmapHost(int(w), int(h), int(kind), C.byref(flt), p.ctypes.data_as(C.POINTER(GatherPoint)), t.ctypes.data_as(C.POINTER(C.c_uint32)), n,
                                          v.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)))
    if ok != 1:
        raise RuntimeError("RaylibAMD_FilterLightmapHost refused the call")
    return out


class GatherAdaptiveParams(C.Structure):
    """include/raylib_amd.h RaylibAMDGatherAdaptiveParams."""
    _fields_ = [("threshold", C.c_float), ("minSamples", C.c_uint32), ("passSamples", C.c_uint32)]


def gather_adaptive(lib, scene, points, kind, threshold, min_samples=4, pass_samples=4, max_path=5, tmin=1e-4, sample_first=0, sample_count=1, skip_draws=0,
                    want_samples=True):
    """Probes gathered in passes with per-point stopping (RaylibAMD_GatherAdaptive / RaylibAMD_GatherAdaptiveDevice; sample_count is the cap): (values, samples).

    points as for gather: a NumPy array goes through the host entry and returns ((n, 4) or (n, 27) float32, (n,) uint32); a float32 torch tensor on the device
    goes through the device entry on torch's current stream -- which the call waits for once per pass -- and returns tensors (samples as int32, holding the
    counts).  want_samples False passes a null outSamples and returns None in its place.  Raises RuntimeError when the library refuses the call."""
    kind = int(kind)
    if kind not in _GATHER_FLOATS:
        raise ValueError("unknown gather kind %r" % kind)
    prm = GatherParams(kind, int(max_path), float(tmin), int(sample_first), int(sample_count), int(skip_draws), 0.0, 0.0)
    ada = GatherAdaptiveParams(float(threshold), int(min_samples), int(pass_samples))
    u32 = C.POINTER(C.c_uint32)
    if isinstance(points, np.ndarray):
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 8)
        n = len(p)
        out = np.zeros((n, _GATHER_FLOATS[kind]), np.float32)
        cnt = np.zeros(n, np.uint32) if want_samples else None
        ok = lib.RaylibAMD_GatherAdaptive(scene, C.byref(prm), C.byref(ada), p.ctypes.data_as(C.POINTER(GatherPoint)), n, out.ctypes.data_as(C.POINTER(C.c_float)),
                                          cnt.ctypes.data_as(u32) if want_samples else None)
        if ok != 1:
            raise RuntimeError("RaylibAMD_GatherAdaptive refused the call")
        return out, cnt
    import torch
    if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float32):
        raise TypeError("points: a float32 NumPy array or a float32 torch tensor on the device")
    p = points.reshape(-1, 8).contiguous()
    n = p.shape[0]
    out = torch.empty((n, _GATHER_FLOATS[kind]), dtype=torch.float32, device=p.device)
    cnt = torch.zeros((n,), dtype=torch.int32, device=p.device) if want_samples else None
    if n:
        prm.timeMin, prm.timeMax = float(p[:, 3].min()), float(p[:, 3].max())
    stream = torch.cuda.current_stream(p.device)
    if stream.cuda_stream == 0:
        stream.synchronize()   # (as gather: the library's stream is not ordered against torch's default stream)
    ok = lib.RaylibAMD_GatherAdaptiveDevice(scene, C.byref(prm), C.byref(ada), C.cast(C.c_void_p(p.data_ptr()), C.POINTER(GatherPoint)), n,
                                            C.cast(C.c_void_p(out.data_ptr()), C.POINTER(C.c_float)),
                                            C.cast(C.c_void_p(cnt.data_ptr()), u32) if want_samples else None, C.c_void_p(stream.cuda_stream))
    if ok != 1:
        raise RuntimeError("RaylibAMD_GatherAdaptiveDevice refused the call")
    return out, cnt


def gather_adaptive_decide_host(lib, keys, threshold, min_samples=4, pass_samples=4, cap=None):
    """RaylibAMD_GatherAdaptiveDecideHost: statements A1 to A3 on keys (count, cap, 3) float32 -- the n at which each point stops, (count,) uint32; no device.
    cap defaults to keys' second dimension.  None when the call refuses."""
    k = np.ascontiguousarray(keys, np.float32)
    cap = k.shape[1] if cap is None else int(cap)
    count = k.shape[0]
    out = np.zeros(count, np.uint32)
    ada = GatherAdaptiveParams(float(threshold), int(min_samples), int(pass_samples))
    ok = lib.RaylibAMD_GatherAdaptiveDecideHost(C.byref(ada), cap, _fp(k), count, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out if ok == 1 else None


def gather_compact_test(lib, live, stopped, points, pad=8):
    """RaylibAMD_GatherCompactTest: (return code, outLive, outPoints, count).  live: ascending original indices; stopped: a byte per original point; points: the
    (numPoints, 8) float32 original records.  The output arrays have len(live) + pad entries, filled with COMPACT_SENTINEL (the records: its bits in every word)
    before the call, and the count is a 1-element array filled likewise: the caller sees what the library wrote and what it left alone."""
    live = np.ascontiguousarray(live, np.uint32)
    stopped = np.ascontiguousarray(stopped, np.uint8)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 8)
    u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    out_live = np.full(len(live) + pad, COMPACT_SENTINEL, np.uint32)
    out_points = np.full((len(live) + pad, 8), COMPACT_SENTINEL, np.uint32)
    count = np.full(1, COMPACT_SENTINEL, np.uint32)
    r = lib.RaylibAMD_GatherCompactTest(live.ctypes.data_as(u32), len(live), stopped.ctypes.data_as(u8), pts.ctypes.data_as(C.POINTER(GatherPoint)), len(pts),
                                        out_live.ctypes.data_as(u32), out_points.ctypes.data_as(C.POINTER(GatherPoint)), count.ctypes.data_as(u32))
    return r, out_live, out_points, count


def bake_lightmap_adaptive(lib, scene, w, h, threshold, min_samples=4, pass_samples=4, uv=None, kind=GATHER_IRRADIANCE, tri_first=0, tri_count=-1, dilate=0, time=0.0,
                           max_path=5, tmin=1e-4, sample_first=0, sample_count=1, skip_draws=0, device=None, want_samples=True):
    """An adaptive bake (RaylibAMD_BakeLightmapAdaptive / RaylibAMD_BakeLightmapAdaptiveDevice; sample_count is the cap): (atlas (H, W, C) float32, coverage (H, W)
    uint8, samples (H, W) uint32 -- int32 as a torch tensor -- or None).  uv and device as for bake_lightmap.  Raises RuntimeError when the library refuses."""
    kind = int(kind)
    if kind not in _GATHER_FLOATS:
        raise ValueError("unknown gather kind %r" % kind)
    c = _GATHER_FLOATS[kind]
    prm = lightmap_params(w, h, kind, tri_first, tri_count, dilate, time, max_path, tmin, sample_first, sample_count, skip_draws)
    ada = GatherAdaptiveParams(float(threshold), int(min_samples), int(pass_samples))
    u32 = C.POINTER(C.c_uint32)
    if device is None and (uv is None or isinstance(uv, np.ndarray)):
        keep, uvp = _uv_host(uv)
        out = np.zeros((int(h), int(w), c), np.float32)
        cov = np.zeros((int(h), int(w)), np.uint8)
        cnt = np.zeros((int(h), int(w)), np.uint32) if want_samples else None
        if lib.RaylibAMD_BakeLightmapAdaptive(scene, C.byref(prm), C.byref(ada), uvp, out.ctypes.data_as(C.POINTER(C.c_float)), cov.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              cnt.ctypes.data_as(u32) if want_samples else None) != 1:
            raise RuntimeError("RaylibAMD_BakeLightmapAdaptive refused the call")
        return out, cov, cnt
    import torch
    if uv is not None:
        if not (isinstance(uv, torch.Tensor) and uv.is_cuda and uv.dtype == torch.float32):
            raise TypeError("uv: None, a float32 NumPy array or a float32 torch tensor on the device")
        uv = uv.reshape(-1, 6).contiguous()
        device = uv.device
    out = torch.empty((int(h), int(w), c), dtype=torch.float32, device=device)
    cov = torch.empty((int(h), int(w)), dtype=torch.uint8, device=device)
    cnt = torch.empty((int(h), int(w)), dtype=torch.int32, device=device) if want_samples else None
    stream = torch.cuda.current_stream(out.device)
    if stream.cuda_stream == 0:
        stream.synchronize()   # (as gather: the library's stream is not ordered against torch's default stream)
    uvp = C.cast(C.c_void_p(uv.data_ptr()), C.POINTER(C.c_float)) if uv is not None else None
    if lib.RaylibAMD_BakeLightmapAdaptiveDevice(scene, C.byref(prm), C.byref(ada), uvp, C.cast(C.c_void_p(out.data_ptr()), C.POINTER(C.c_float)),
                                                C.cast(C.c_void_p(cov.data_ptr()), C.POINTER(C.c_uint8)),
                                                C.cast(C.c_void_p(cnt.data_ptr()), u32) if want_samples else None, C.c_void_p(stream.cuda_stream)) != 1:
        raise RuntimeError("RaylibAMD_BakeLightmapAdaptiveDevice refused the call")
    return out, cov, cnt


# Per-ray / per-unit algorithmic byte constants of the flat layout (csrc/rl_device.h)
NODE_B, TRI_B, SHADE_B, TEXEL_B, PIXEL_B = 64, 64, 64, 16, 16


def algorithmic_bytes(stats):
    """nodes*NODE_B + tris*TRI_B + shaded*SHADE_B + texels*TEXEL_B + pixels*16 (NODE_B = 80 when the 8-wide tree was walked)."""
    return (stats.nodesVisited * (getattr(stats, "nodeBytes", 0) or NODE_B) + stats.trisTested * TRI_B + stats.shadedHits * SHADE_B +
            stats.texFetches * TEXEL_B + stats.pixels * PIXEL_B)


_EXPORTS = {
    # name: (restype, argtypes)   -- include/raylib.h
    "Raylib_Initialize": (C.c_int32, []),
    "Raylib_Terminate": (C.c_int32, []),
    "Raylib_LoadOBJModel": (C.c_void_p, [C.c_char_p]),
    "Raylib_TransformOBJModel": (None, [C.c_void_p] + [C.c_float] * 9),
    "Raylib_FinalizeOBJModel": (None, [C.c_void_p]),
    "Raylib_UnloadOBJModel": (C.c_int32, [C.c_void_p]),
    "Raylib_LoadImage": (C.c_void_p, [C.c_char_p]),
    "Raylib_CreateScene": (C.c_void_p, []),
    "Raylib_AddSceneElement": (None, [C.c_void_p, C.c_void_p]),
    "Raylib_AddOBJModelToScene": (None, [C.c_void_p, C.c_void_p]),
    "Raylib_SetSkyPanorama": (None, [C.c_void_p, C.c_void_p]),
    "Raylib_SetSunIlluminance": (None, [C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "Raylib_SetSunDirection": (None, [C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "Raylib_FinalizeScene": (None, [C.c_void_p]),
    "Raylib_DestroyScene": (C.c_int32, [C.c_void_p]),
    "Raylib_CreateCamera": (C.c_void_p, []),
    "Raylib_CameraSetPosition": (None, [C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "Raylib_CameraSetLookAt": (None, [C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "Raylib_CameraSetPerspective": (None, [C.c_void_p, C.c_float, C.c_float]),
    "Raylib_CameraSetLens": (None, [C.c_void_p, C.c_float, C.c_float]),
    "Raylib_CameraSetMotion": (None, [C.c_void_p, C.c_float, C.c_float]),
    "Raylib_CameraCopy": (None, [C.c_void_p, C.c_void_p]),
    "Raylib_DestroyCamera": (C.c_int32, [C.c_void_p]),
    "Raylib_CreateImage": (C.c_void_p, [C.c_uint32, C.c_uint32]),
    "Raylib_DumpImageData": (None, [C.c_void_p, C.POINTER(C.c_float)]),
    "Raylib_DestroyImage": (C.c_int32, [C.c_void_p]),
    "Raylib_Render": (None, [C.POINTER(RendererSettings), C.c_void_p, C.c_void_p, C.c_void_p]),
    "Raylib_Denoise": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "Raylib_PostProcess": (None, [C.c_void_p]),
    "Raylib_IsDenoiserSupported": (C.c_int32, []),
    "Raylib_GetRenderModeString": (C.c_char_p, [C.c_uint32]),
    "Raylib_WriteImageToDisk": (C.c_int32, [C.c_void_p, C.c_char_p, C.c_uint32]),
    "Raylib_FlushLogThread": (None, []),
    # include/raylib_amd.h
    "RaylibAMD_SetSeed": (None, [C.c_uint64]),
    "RaylibAMD_GetSeed": (C.c_uint64, []),
    "RaylibAMD_GetLastStats": (None, [C.POINTER(Stats)]),
    "RaylibAMD_DeviceAvailable": (C.c_int32, []),
    "RaylibAMD_BuildId": (C.c_char_p, []),
    "RaylibAMD_RenderDevice": (C.c_int32, [C.POINTER(RendererSettings), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "RaylibAMD_RenderCellsHost": (C.c_int32, [C.POINTER(RendererSettings), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "RaylibAMD_CellBufferFloats": (C.c_uint64, [C.c_uint32] * 4),
    "RaylibAMD_NumCells": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "RaylibAMD_CreateMaterial": (C.c_void_p, [C.c_int32, C.POINTER(C.c_float), C.c_float, C.c_float, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float), C.c_float]),
    "RaylibAMD_DestroyMaterial": (C.c_int32, [C.c_void_p]),
    "RaylibAMD_CreateSphere": (C.c_void_p, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "RaylibAMD_CreateCube": (C.c_void_p, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float), C.c_void_p]),
    "RaylibAMD_CreateTriangle": (C.c_void_p, [C.POINTER(C.c_float)] * 7 + [C.c_void_p]),
    "RaylibAMD_DestroySceneElement": (C.c_int32, [C.c_void_p]),
    "RaylibAMD_EvalScatter": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.c_int32, C.c_uint64, C.POINTER(C.c_float)]),
    "RaylibAMD_EvalCameraRays": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.c_uint64, C.POINTER(C.c_float)]),
    "RaylibAMD_EvalTexture": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float)]),
    "RaylibAMD_EvalDeviceMath": (C.c_int32, [C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float)]),
    "RaylibAMD_ClosestHit": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_void_p]),
    "RaylibAMD_TraceRays": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "RaylibAMD_TraceRaysDevice": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_PlanRayQuery": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(QueryPlan)]),
    "RaylibAMD_RenderGBuffer": (C.c_int32, [C.POINTER(RendererSettings), C.c_void_p, C.c_void_p, C.POINTER(GBufferPlanes)]),
    "RaylibAMD_RenderGBufferDevice": (C.c_int32, [C.POINTER(RendererSettings), C.c_void_p, C.c_void_p, C.POINTER(GBufferPlanes), C.c_void_p]),
    "RaylibAMD_RenderGuides": (C.c_int32, [C.POINTER(RendererSettings), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_PlanGBuffer": (C.c_int32, [C.c_void_p, C.POINTER(QueryPlan)]),
    "RaylibAMD_RenderMotion": (C.c_int32, [C.POINTER(RendererSettings), C.c_void_p, C.c_void_p, C.POINTER(MotionParams), C.POINTER(MotionPlanes)]),
    "RaylibAMD_RenderMotionDevice": (C.c_int32, [C.POINTER(RendererSettings), C.c_void_p, C.c_void_p, C.POINTER(MotionParams), C.POINTER(MotionPlanes), C.c_void_p]),
    "RaylibAMD_MotionHost": (C.c_int32, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(MotionParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_PlanMotion": (C.c_int32, [C.c_void_p, C.POINTER(QueryPlan)]),
    "RaylibAMD_TemporalAccumulate": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(TemporalParams)] + [C.c_void_p] * 3 + [C.POINTER(TemporalFrame)] + [C.c_void_p] * 2),
    "RaylibAMD_TemporalAccumulateDevice": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(TemporalParams)] + [C.c_void_p] * 3 + [C.POINTER(TemporalFrame)] + [C.c_void_p] * 3),
    "RaylibAMD_TemporalAccumulateHost": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(TemporalParams)] + [C.c_void_p] * 3 + [C.POINTER(TemporalFrame)] + [C.c_void_p] * 2),
    "RaylibAMD_TemporalAccumulateMoments": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(TemporalParams)] + [C.c_void_p] * 3 + [C.POINTER(TemporalMomentsFrame)] + [C.c_void_p] * 3),
    "RaylibAMD_TemporalAccumulateMomentsDevice": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(TemporalParams)] + [C.c_void_p] * 3 + [C.POINTER(TemporalMomentsFrame)] + [C.c_void_p] * 4),
    "RaylibAMD_TemporalAccumulateMomentsHost": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(TemporalParams)] + [C.c_void_p] * 3 + [C.POINTER(TemporalMomentsFrame)] + [C.c_void_p] * 3),
    "RaylibAMD_FilterVariance": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(VarianceFilterParams), C.POINTER(VarianceFilterPlanes)] + [C.c_void_p] * 2),
    "RaylibAMD_FilterVarianceDevice": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(VarianceFilterParams), C.POINTER(VarianceFilterPlanes)] + [C.c_void_p] * 3),
    "RaylibAMD_FilterVarianceHost": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(VarianceFilterParams), C.POINTER(VarianceFilterPlanes)] + [C.c_void_p] * 2),
    "RaylibAMD_TraceRadiance": (C.c_int32, [C.c_void_p, C.POINTER(RadianceParams), C.POINTER(PathRay), C.c_int32, C.POINTER(C.c_float)]),
    "RaylibAMD_TraceRadianceDevice": (C.c_int32, [C.c_void_p, C.POINTER(RadianceParams), C.POINTER(PathRay), C.c_int32, C.POINTER(C.c_float), C.c_void_p]),
    "RaylibAMD_PlanRadiance": (C.c_int32, [C.c_void_p, C.POINTER(RadianceParams), C.POINTER(QueryPlan)]),
    "RaylibAMD_TraceRaysAll": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]),
    "RaylibAMD_TraceRaysAllDevice": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_TraceRaysAllHost": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]),
    "RaylibAMD_PlanRayQueryAll": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(QueryPlan)]),
    "RaylibAMD_NearestPoints": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "RaylibAMD_NearestPointsDevice": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "RaylibAMD_NearestPointsHost": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "RaylibAMD_PlanNearest": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(QueryPlan)]),
    "RaylibAMD_SweepSpheres": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "RaylibAMD_SweepSpheresDevice": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "RaylibAMD_SweepSpheresHost": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "RaylibAMD_PlanSweep": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(QueryPlan)]),
    "RaylibAMD_NearestPointsAll": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "RaylibAMD_NearestPointsAllDevice": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_NearestPointsAllHost": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "RaylibAMD_PlanNearestAll": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(QueryPlan)]),
    "RaylibAMD_BakeDistanceField": (C.c_int32, [C.c_void_p, C.POINTER(DistanceFieldParams), C.c_void_p, C.c_void_p]),
    "RaylibAMD_BakeDistanceFieldDevice": (C.c_int32, [C.c_void_p, C.POINTER(DistanceFieldParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_BakeDistanceFieldHost": (C.c_int32, [C.c_void_p, C.POINTER(DistanceFieldParams), C.c_void_p, C.c_void_p]),
    "RaylibAMD_PlanDistanceField": (C.c_int32, [C.c_void_p, C.POINTER(DistanceFieldParams), C.POINTER(QueryPlan), C.POINTER(QueryPlan)]),
    "RaylibAMD_OverlapTriangles": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "RaylibAMD_OverlapTrianglesDevice": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_OverlapTrianglesHost": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "RaylibAMD_PlanOverlap": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(QueryPlan)]),
    "RaylibAMD_OverlapContacts": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_OverlapContactsDevice": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_OverlapContactsHost": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_PlanOverlapContacts": (C.c_int32, [C.c_void_p, C.POINTER(QueryPlan)]),
    "RaylibAMD_OverlapBoxes": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "RaylibAMD_OverlapBoxesDevice": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_OverlapBoxesHost": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "RaylibAMD_PlanOverlapBoxes": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(QueryPlan)]),
    "RaylibAMD_Gather": (C.c_int32, [C.c_void_p, C.POINTER(GatherParams), C.POINTER(GatherPoint), C.c_int32, C.POINTER(C.c_float)]),
    "RaylibAMD_GatherDevice": (C.c_int32, [C.c_void_p, C.POINTER(GatherParams), C.POINTER(GatherPoint), C.c_int32, C.POINTER(C.c_float), C.c_void_p]),
    "RaylibAMD_GatherDirectionsHost": (C.c_int32, [C.POINTER(GatherParams), C.POINTER(GatherPoint), C.c_int32, C.c_uint64, C.c_uint32, C.POINTER(C.c_float)]),
    "RaylibAMD_PlanGatherCut": (C.c_int32, [C.POINTER(GatherParams), C.c_int32, C.c_uint64, C.POINTER(GatherCut)]),
    "RaylibAMD_GatherAdaptive": (C.c_int32, [C.c_void_p, C.POINTER(GatherParams), C.POINTER(GatherAdaptiveParams), C.POINTER(GatherPoint), C.c_int32, C.POINTER(C.c_float),
                                             C.POINTER(C.c_uint32)]),
    "RaylibAMD_GatherAdaptiveDevice": (C.c_int32, [C.c_void_p, C.POINTER(GatherParams), C.POINTER(GatherAdaptiveParams), C.POINTER(GatherPoint), C.c_int32, C.POINTER(C.c_float),
                                                   C.POINTER(C.c_uint32), C.c_void_p]),
    "RaylibAMD_GatherAdaptiveDecideHost": (C.c_int32, [C.POINTER(GatherAdaptiveParams), C.c_uint32, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_uint32)]),
    "RaylibAMD_GatherCompactTest": (C.c_int32, [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(GatherPoint), C.c_uint32, C.POINTER(C.c_uint32),
                                                C.POINTER(GatherPoint), C.POINTER(C.c_uint32)]),
    "RaylibAMD_BakeLightmapAdaptive": (C.c_int32, [C.c_void_p, C.POINTER(LightmapParams), C.POINTER(GatherAdaptiveParams), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                   C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]),
    "RaylibAMD_BakeLightmapAdaptiveDevice": (C.c_int32, [C.c_void_p, C.POINTER(LightmapParams), C.POINTER(GatherAdaptiveParams), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                         C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.c_void_p]),
    "RaylibAMD_LightmapPoints": (C.c_int64, [C.c_void_p, C.POINTER(LightmapParams), C.POINTER(C.c_float), C.POINTER(GatherPoint), C.POINTER(C.c_uint32), C.c_int64]),
    "RaylibAMD_LightmapPointsHost": (C.c_int64, [C.c_void_p, C.POINTER(LightmapParams), C.POINTER(C.c_float), C.POINTER(GatherPoint), C.POINTER(C.c_uint32), C.c_int64]),
    "RaylibAMD_BakeLightmap": (C.c_int32, [C.c_void_p, C.POINTER(LightmapParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8)]),
    "RaylibAMD_BakeLightmapDevice": (C.c_int32, [C.c_void_p, C.POINTER(LightmapParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_void_p]),
    "RaylibAMD_BakeLightmapFiltered": (C.c_int32, [C.c_void_p, C.POINTER(LightmapParams), C.POINTER(LightmapFilterParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8)]),
    "RaylibAMD_BakeLightmapFilteredDevice": (C.c_int32, [C.c_void_p, C.POINTER(LightmapParams), C.POINTER(LightmapFilterParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8),
                                                         C.c_void_p]),
    "RaylibAMD_FilterLightmap": (C.c_int32, [C.c_void_p, C.POINTER(LightmapParams), C.POINTER(LightmapFilterParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                             C.POINTER(C.c_uint8)]),
    "RaylibAMD_FilterLightmapDevice": (C.c_int32, [C.c_void_p, C.POINTER(LightmapParams), C.POINTER(LightmapFilterParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                   C.POINTER(C.c_uint8), C.c_void_p]),
    "RaylibAMD_FilterLightmapHost": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(LightmapFilterParams), C.POINTER(GatherPoint), C.POINTER(C.c_uint32), C.c_int64,
                                                 C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "RaylibAMD_VerifyExactMath": (C.c_int32, [C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "RaylibAMD_CullCells": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_float)]),
    "RaylibAMD_SceneNumTriangles": (C.c_int32, [C.c_void_p]),
    "RaylibAMD_SceneNumMaterials": (C.c_int32, [C.c_void_p]),
    "RaylibAMD_SceneNumTextures": (C.c_int32, [C.c_void_p]),
    "RaylibAMD_SceneExportTriangles": (None, [C.c_void_p, C.c_void_p]),
    "RaylibAMD_SceneExportTriOrder": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "RaylibAMD_SceneExportMaterials": (None, [C.c_void_p, C.c_void_p]),
    "RaylibAMD_SceneTextureSize": (None, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "RaylibAMD_SceneExportTexture": (None, [C.c_void_p, C.c_int32, C.POINTER(C.c_float)]),
    "RaylibAMD_SceneGetSun": (None, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "RaylibAMD_SceneBVHInfo": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "RaylibAMD_ParseFloat": (C.c_float, [C.c_char_p]),
    "RaylibAMD_ImageSize": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "RaylibAMD_SceneBVH4Info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "RaylibAMD_SceneBVH8Info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "RaylibAMD_SceneLeafListInfo": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "RaylibAMD_ScenePlain": (C.c_int32, [C.c_void_p]),
    "RaylibAMD_LastTracePlain": (C.c_int32, []),
    "RaylibAMD_SceneLazyRefl": (C.c_int32, [C.c_void_p]),
    "RaylibAMD_LastTraceLazy": (C.c_int32, []),
    "RaylibAMD_LastHitQueue": (C.c_int32, []),
    "RaylibAMD_LastLitMask": (C.c_int32, []),
    "RaylibAMD_VerifyLazyRefl": (C.c_int32, [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "RaylibAMD_VerifyLazyPdf": (C.c_int32, [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "RaylibAMD_VerifySamplerRanged": (C.c_int32, [C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "RaylibAMD_VerifyNormalizeRanged": (C.c_int32, [C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "RaylibAMD_PlanRender": (C.c_int32, [C.c_void_p, C.POINTER(RendererSettings), C.c_int32, C.c_int32, C.c_int32, C.POINTER(RenderPlan)]),
    "RaylibAMD_SceneWalk8Host": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "RaylibAMD_SceneWalkStackHost": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "RaylibAMD_SceneBVHHash": (C.c_uint64, [C.c_void_p]),
    "RaylibAMD_SceneTopologyHash": (C.c_uint64, [C.c_void_p]),
    "RaylibAMD_SceneExportBVHNodes": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "RaylibAMD_SceneMoveTriangles": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "RaylibAMD_SceneMoveTrianglesDevice": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "RaylibAMD_SceneRebuild": (C.c_int32, [C.c_void_p]),
    "RaylibAMD_SceneCheckTrees": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "RaylibAMD_SceneCompareTrees": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "RaylibAMD_CameraExport": (None, [C.c_void_p, C.POINTER(C.c_float)]),
    "RaylibAMD_CreateImageFromData": (C.c_void_p, [C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "RaylibAMD_DumpImageRGBA": (None, [C.c_void_p, C.POINTER(C.c_float)]),
    "RaylibAMD_OBJModelSetTexture": (C.c_int32, [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p]),
    "RaylibAMD_Denoise": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenoiseParams)]),
    "RaylibAMD_DenoiseHost": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                          C.POINTER(DenoiseParams), C.POINTER(C.c_float)]),
    "RaylibAMD_EnableDenoiser": (None, [C.c_int32]),
    "RaylibAMD_BeginProgressive": (C.c_size_t, [C.POINTER(RendererSettings), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ProgressiveParams)]),
    "RaylibAMD_ProgressiveStep": (C.c_int32, [C.c_size_t, C.c_uint32]),
    "RaylibAMD_ProgressiveExport": (C.c_int32, [C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "RaylibAMD_EndProgressive": (C.c_int32, [C.c_size_t]),
    "RaylibAMD_ProgressiveDecideHost": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                    C.POINTER(ProgressiveParams), C.POINTER(C.c_uint8)]),
    "RaylibAMD_ProgressiveCompactTest": (C.c_int32, [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_uint32,
                                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "RaylibAMD_RenderViews": (C.c_int32, [C.POINTER(RendererSettings), C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p)]),
    "RaylibAMD_RenderViewsDevice": (C.c_int32, [C.POINTER(RendererSettings), C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p]),
    "RaylibAMD_PlanViews": (C.c_int32, [C.c_void_p, C.POINTER(RendererSettings), C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.POINTER(RenderPlan), C.POINTER(C.c_uint8)]),
}
MAX_VIEWS = 64   # RAYLIB_AMD_MAX_VIEWS
RAYLIB_H_EXPORTS = [k for k in _EXPORTS if k.startswith("Raylib_")]
RAYLIB_AMD_H_EXPORTS = [k for k in _EXPORTS if k.startswith("RaylibAMD_")]


def load(path=LIB_PATH):
    if not os.path.exists(path):
        raise FileNotFoundError(path + " -- build it with `make -C software-raytracing_amd` (or __graft_entry__.build())")
    lib = C.CDLL(path)
    for name, (res, args) in _EXPORTS.items():
        if os.environ.get("RAYLIB_LIB") and name.startswith("RaylibAMD_") and not hasattr(lib, name):
            continue              # (an older build named by RAYLIB_LIB for an A/B run may lack a newer introspection hook; the tree's own library must export everything)
        fn = getattr(lib, name)   # AttributeError if the library does not export it
        fn.restype, fn.argtypes = res, args
    return lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def create_camera(lib, origin, look_at, fov, aspect, aperture=0.0, focal=1.0, shutter=(0.0, 0.0)):
    """A camera handle (Raylib_CreateCamera and its setters); the caller destroys it with Raylib_DestroyCamera."""
    cam = lib.Raylib_CreateCamera()
    lib.Raylib_CameraSetPosition(cam, *[float(x) for x in origin])
    lib.Raylib_CameraSetLookAt(cam, *[float(x) for x in look_at])
    lib.Raylib_CameraSetPerspective(cam, float(fov), float(aspect))
    lib.Raylib_CameraSetLens(cam, float(aperture), float(focal))
    lib.Raylib_CameraSetMotion(cam, float(shutter[0]), float(shutter[1]))
    return cam


def handle_array(handles):
    """A C array of handles (CameraHandle / ImageHandle) for RaylibAMD_RenderViews and RaylibAMD_PlanViews."""
    return (C.c_void_p * max(1, len(handles)))(*[h or None for h in handles])


def create_material(lib, mat):
    """mat: one record of the oracle's MAT_DTYPE layout (type, albedo, roughness, metallic, emissive, ior, transmission, fuzziness)."""
    return lib.RaylibAMD_CreateMaterial(int(mat["type"]), _f3(mat["albedo"]), float(mat["roughness"]), float(mat["metallic"]),
                                        _f3(mat["emissive"]), float(mat["ior"]), _f3(mat["transmission"]), float(mat["fuzziness"]))


def progressive_decide_host(lib, width, height, cell_samples, sum_y, sum_y2, threshold=None, min_samples=2):
    """RaylibAMD_ProgressiveDecideHost: one bool per cell (cellsY, cellsX); threshold None = no params (uniform).  None when the call refuses."""
    cells = np.ascontiguousarray(cell_samples, np.uint32)
    s1, s2 = np.ascontiguousarray(sum_y, np.float32), np.ascontiguousarray(sum_y2, np.float32)
    out = np.zeros(((height + 7) // 8, (width + 7) // 8), np.uint8)
    prm = None if threshold is None else C.byref(ProgressiveParams(float(threshold), int(min_samples)))
    ok = lib.RaylibAMD_ProgressiveDecideHost(width, height, cells.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(s1), _fp(s2), prm,
                                             out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out.astype(bool) if ok == 1 else None


COMPACT_SENTINEL = 0xDEADBEEF


def progressive_compact_test(lib, width, height, live, stopped, empty=None, num_cells=None, pad=8):
    """RaylibAMD_ProgressiveCompactTest: (return code, outLive, outTrace, counts).  The output arrays have len(live) + pad entries and the counts 4, all
    filled with COMPACT_SENTINEL before the call: the caller sees what the library wrote and what it left alone."""
    live = np.ascontiguousarray(live, np.uint32)
    stopped = np.ascontiguousarray(stopped, np.uint8)
    empty = None if empty is None else np.ascontiguousarray(empty, np.uint8)
    n = ((width + 7) // 8) * ((height + 7) // 8) if num_cells is None else int(num_cells)
    u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    out_live = np.full(len(live) + pad, COMPACT_SENTINEL, np.uint32)
    out_trace = np.full(len(live) + pad, COMPACT_SENTINEL, np.uint32)
    counts = np.full(4, COMPACT_SENTINEL, np.uint32)
    r = lib.RaylibAMD_ProgressiveCompactTest(live.ctypes.data_as(u32), len(live), stopped.ctypes.data_as(u8), None if empty is None else empty.ctypes.data_as(u8),
                                             n, int(width), int(height), out_live.ctypes.data_as(u32), out_trace.ctypes.data_as(u32), counts.ctypes.data_as(u32))
    return r, out_live, out_trace, counts


class Progressive:
    """A progressive session (include/raylib_amd.h RaylibAMD_BeginProgressive) on a session's scene and camera, rendering into its own image:
    step(n) -> live cells (0 = finished), frame() -> (H, W, 4) float32, export() -> (cell samples, stopped, S1, S2)."""

    def __init__(self, ses, w, h, spp, max_path=5, tmin=1e-4, mode=RENDERMODE_DEFAULT, threshold=None, min_samples=2, image=None):
        self.lib, self.w, self.h = ses.lib, int(w), int(h)
        st = RendererSettings(int(w), int(h), int(spp), int(max_path), float(tmin), int(mode))
        self.own_image = image is None
        self.image = self.lib.Raylib_CreateImage(w, h) if image is None else image
        prm = None if threshold is None else C.byref(ProgressiveParams(float(threshold), int(min_samples)))
        self.handle = self.lib.RaylibAMD_BeginProgressive(C.byref(st), ses.scene, ses.camera, self.image, prm)

    def step(self, samples):
        return self.lib.RaylibAMD_ProgressiveStep(self.handle, int(samples))

    def frame(self):
        out = np.zeros((self.h, self.w, 4), np.float32)
        self.lib.RaylibAMD_DumpImageRGBA(self.image, _fp(out))
        return out

    def export(self):
        cy, cx = (self.h + 7) // 8, (self.w + 7) // 8
        n = np.zeros((cy, cx), np.uint32)
        stopped = np.zeros((cy, cx), np.uint8)
        s1 = np.zeros((self.h, self.w), np.float32)
        s2 = np.zeros((self.h, self.w), np.float32)
        ok = self.lib.RaylibAMD_ProgressiveExport(self.handle, n.ctypes.data_as(C.POINTER(C.c_uint32)), stopped.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(s1), _fp(s2))
        assert ok == 1
        return n, stopped.astype(bool), s1, s2

    def close(self):
        r = self.lib.RaylibAMD_EndProgressive(self.handle) if self.handle else 0
        if self.own_image:
            self.lib.Raylib_DestroyImage(self.image)
        self.handle = 0
        return r


class ProceduralSession:
    """A scene made of analytic elements through the C-ABI (what the reference's CUI does with C++ objects,
    src/main.cc:913-984): materials -> spheres / cubes -> Raylib_AddSceneElement -> FinalizeScene."""

    def __init__(self, lib, materials, spheres=(), cubes=(), origin=(0, 0, 3), look_at=(0, 0, -1), fov=45.0, aspect=1.0,
                 sun=(0, 0, 0), sun_dir=(0.0, -1.0, -0.5), aperture=0.0, focal=1.0, shutter=(0.0, 0.0)):
        self.lib = lib
        self.mats = [create_material(lib, m) for m in materials]
        assert all(self.mats)
        self.scene = lib.Raylib_CreateScene()
        self.camera = lib.Raylib_CreateCamera()
        self.elems = []
        for s in spheres:
            e = lib.RaylibAMD_CreateSphere(float(s["center"][0]), float(s["center"][1]), float(s["center"][2]), float(s["radius"]), self.mats[int(s["material"])])
            self.elems.append(e); lib.Raylib_AddSceneElement(self.scene, e)
        for c in cubes:
            e = lib.RaylibAMD_CreateCube(_f3(c["minBounds"]), _f3(c["maxBounds"]), float(c["timeStartMove"]), _f3(c["velocity"]), self.mats[int(c["material"])])
            self.elems.append(e); lib.Raylib_AddSceneElement(self.scene, e)
        assert all(self.elems)
        lib.Raylib_SetSunIlluminance(self.scene, *[float(x) for x in sun])
        lib.Raylib_SetSunDirection(self.scene, *[float(x) for x in sun_dir])
        lib.Raylib_FinalizeScene(self.scene)
        lib.Raylib_CameraSetPosition(self.camera, *[float(x) for x in origin])
        lib.Raylib_CameraSetLookAt(self.camera, *[float(x) for x in look_at])
        lib.Raylib_CameraSetPerspective(self.camera, float(fov), float(aspect))
        lib.Raylib_CameraSetLens(self.camera, float(aperture), float(focal))
        lib.Raylib_CameraSetMotion(self.camera, float(shutter[0]), float(shutter[1]))

    settings = None

    def render(self, w, h, spp, max_path=5, tmin=1e-4, mode=RENDERMODE_DEFAULT):
        lib = self.lib
        st = RendererSettings(int(w), int(h), int(spp), int(max_path), float(tmin), int(mode))
        img = lib.Raylib_CreateImage(w, h)
        lib.Raylib_Render(C.byref(st), self.scene, self.camera, img)
        out = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, _fp(out))
        lib.Raylib_DestroyImage(img)
        return out

    def close(self):
        lib = self.lib
        lib.Raylib_DestroyScene(self.scene); lib.Raylib_DestroyCamera(self.camera)
        for e in self.elems:
            lib.RaylibAMD_DestroySceneElement(e)
        for m in self.mats:
            lib.RaylibAMD_DestroyMaterial(m)


class SceneSession:
    """The GUI's call sequence (reference gui-app/gui-app/MainForm.cs:121-256) as an object:
    LoadOBJ -> FinalizeOBJ -> CreateScene/Camera -> AddOBJ -> Sun -> FinalizeScene -> camera setters."""

    def __init__(self, lib, obj_path, origin, look_at, fov, aspect, sun=(0, 0, 0), sun_dir=(0.0, -1.0, -0.5),
                 aperture=0.0, focal=1.0, shutter=(0.0, 0.0), sky_image=None, textures=()):
        self.lib = lib
        self.obj = lib.Raylib_LoadOBJModel(obj_path.encode())
        if not self.obj:
            raise RuntimeError("Raylib_LoadOBJModel failed: " + obj_path)
        self._images = []
        for mat_name, slot, rgba in textures:
            rgba = np.ascontiguousarray(rgba, np.float32)
            ih = lib.RaylibAMD_CreateImageFromData(rgba.shape[1], rgba.shape[0], _fp(rgba))
            self._images.append(ih)
            if not lib.RaylibAMD_OBJModelSetTexture(self.obj, mat_name.encode(), slot, ih):
                raise RuntimeError("RaylibAMD_OBJModelSetTexture failed for " + mat_name)
        lib.Raylib_FinalizeOBJModel(self.obj)
        self.scene = lib.Raylib_CreateScene()
        self.camera = lib.Raylib_CreateCamera()
        lib.Raylib_AddOBJModelToScene(self.scene, self.obj)
        lib.Raylib_SetSunIlluminance(self.scene, *[float(x) for x in sun])
        lib.Raylib_SetSunDirection(self.scene, *[float(x) for x in sun_dir])
        self.has_sky = sky_image is not None
        if sky_image is not None:
            sky = np.ascontiguousarray(sky_image, np.float32)
            ih = lib.RaylibAMD_CreateImageFromData(sky.shape[1], sky.shape[0], _fp(sky))
            self._images.append(ih)
            lib.Raylib_SetSkyPanorama(self.scene, ih)
        lib.Raylib_FinalizeScene(self.scene)
        lib.Raylib_CameraSetPosition(self.camera, *[float(x) for x in origin])
        lib.Raylib_CameraSetLookAt(self.camera, *[float(x) for x in look_at])
        lib.Raylib_CameraSetPerspective(self.camera, float(fov), float(aspect))
        lib.Raylib_CameraSetLens(self.camera, float(aperture), float(focal))
        lib.Raylib_CameraSetMotion(self.camera, float(shutter[0]), float(shutter[1]))

    def settings(self, w, h, spp, max_path=5, tmin=1e-4, mode=RENDERMODE_DEFAULT):
        return RendererSettings(int(w), int(h), int(spp), int(max_path), float(tmin), int(mode))

    def render(self, w, h, spp, max_path=5, tmin=1e-4, mode=RENDERMODE_DEFAULT):
        """Raylib_Render into a fresh image; returns (H, W, 4) float32 RGBA."""
        lib = self.lib
        st = self.settings(w, h, spp, max_path, tmin, mode)
        img = lib.Raylib_CreateImage(w, h)
        lib.Raylib_Render(C.byref(st), self.scene, self.camera, img)
        out = np.zeros((h, w, 4), np.float32)
        lib.RaylibAMD_DumpImageRGBA(img, _fp(out))
        lib.Raylib_DestroyImage(img)
        return out

    def render_views(self, cameras, w, h, spp, max_path=5, tmin=1e-4, mode=RENDERMODE_DEFAULT):
        """RaylibAMD_RenderViews of camera handles (create_camera) into fresh images; returns (N, H, W, 4) float32 RGBA, view i as
        Raylib_Render of cameras[i] would give it."""
        lib = self.lib
        st = self.settings(w, h, spp, max_path, tmin, mode)
        imgs = [lib.Raylib_CreateImage(w, h) for _ in cameras]
        try:
            if lib.RaylibAMD_RenderViews(C.byref(st), self.scene, handle_array(cameras), len(cameras), handle_array(imgs)) != 1:
                raise RuntimeError("RaylibAMD_RenderViews failed")
            out = np.zeros((len(cameras), h, w, 4), np.float32)
            for i, ih in enumerate(imgs):
                lib.RaylibAMD_DumpImageRGBA(ih, _fp(out[i]))
        finally:
            for ih in imgs:
                lib.Raylib_DestroyImage(ih)
        return out

    def gbuffer(self, w, h, tmin=1e-4, planes=GBUFFER_PLANES):
        """RaylibAMD_RenderGBuffer of the session's scene and camera: a dict of NumPy arrays (gbuffer above)."""
        return gbuffer(self.lib, self.scene, self.camera, w, h, tmin, planes)

    def gbuffer_device(self, w, h, tmin=1e-4, planes=GBUFFER_PLANES, out=None):
        """RaylibAMD_RenderGBufferDevice on torch's current stream: a dict of tensors (gbuffer_device above)."""
        return gbuffer_device(self.lib, self.scene, self.camera, w, h, tmin, planes, out)

    def motion(self, w, h, prev_camera=None, first=0, prev_positions=None, tmin=1e-4, planes=("hit", "motion")):
        """RaylibAMD_RenderMotion of the session's scene and camera: a dict of NumPy arrays (motion above)."""
        return motion(self.lib, self.scene, self.camera, w, h, prev_camera, first, prev_positions, tmin, planes)

    def motion_device(self, w, h, prev_camera=None, first=0, prev_positions=None, tmin=1e-4, planes=("hit", "motion"), out=None):
        """RaylibAMD_RenderMotionDevice on torch's current stream: a dict of tensors (motion_device above)."""
        return motion_device(self.lib, self.scene, self.camera, w, h, prev_camera, first, prev_positions, tmin, planes, out)

    def motion_host(self, w, h, rays, hit, prev_camera=None, first=0, prev_positions=None):
        """RaylibAMD_MotionHost for the session's scene and camera (motion_host above)."""
        return motion_host(self.lib, self.scene, self.camera, w, h, rays, hit, prev_camera, first, prev_positions)

    def temporal_accumulate(self, colour, hit, motion, history=None, depth_tolerance=0.02, max_length=32.0, host=False):
        """RaylibAMD_TemporalAccumulate / ...Host on NumPy arrays (temporal_accumulate above; the call needs no scene)."""
        return temporal_accumulate(self.lib, colour, hit, motion, history, depth_tolerance, max_length, host)

    def temporal_accumulate_device(self, colour, hit, motion, history=None, depth_tolerance=0.02, max_length=32.0, out=None):
        """RaylibAMD_TemporalAccumulateDevice on torch's current stream (temporal_accumulate_device above)."""
        return temporal_accumulate_device(self.lib, colour, hit, motion, history, depth_tolerance, max_length, out)

    def temporal_accumulate_moments(self, colour, hit, motion, history=None, depth_tolerance=0.02, max_length=32.0, host=False):
        """RaylibAMD_TemporalAccumulateMoments / ...Host on NumPy arrays (temporal_accumulate_moments above; the call needs no scene)."""
        return temporal_accumulate_moments(self.lib, colour, hit, motion, history, depth_tolerance, max_length, host)

    def temporal_accumulate_moments_device(self, colour, hit, motion, history=None, depth_tolerance=0.02, max_length=32.0, out=None):
        """RaylibAMD_TemporalAccumulateMomentsDevice on torch's current stream (temporal_accumulate_moments_device above)."""
        return temporal_accumulate_moments_device(self.lib, colour, hit, motion, history, depth_tolerance, max_length, out)

    def filter_variance(self, colour, moments, length, hit, surface, params=None, variance=True, host=False):
        """RaylibAMD_FilterVariance / ...Host on NumPy arrays (filter_variance above; the call needs no scene)."""
        return filter_variance(self.lib, colour, moments, length, hit, surface, params, variance, host)

    def filter_variance_device(self, colour, moments, length, hit, surface, params=None, variance=True, out=None):
        """RaylibAMD_FilterVarianceDevice on torch's current stream (filter_variance_device above)."""
        return filter_variance_device(self.lib, colour, moments, length, hit, surface, params, variance, out)

    def render_cells(self, w, h, spp, rank, world, max_path=5, tmin=1e-4, mode=RENDERMODE_DEFAULT):
        """What rank `rank` of `world` renders: its cells back to back, (n_cells*64, 4) float32."""
        st = self.settings(w, h, spp, max_path, tmin, mode)
        n = self.lib.RaylibAMD_CellBufferFloats(w, h, rank, world)
        out = np.zeros(max(n, 4), np.float32)
        if self.lib.RaylibAMD_RenderCellsHost(C.byref(st), self.scene, self.camera, rank, world, _fp(out)) != 1:
            raise RuntimeError("RaylibAMD_RenderCellsHost failed")
        return out[:n].reshape(-1, 4)

    def stats(self):
        s = Stats()
        self.lib.RaylibAMD_GetLastStats(C.byref(s))
        return s

    def export_flat(self):
        """(triangles, materials) as numpy arrays with the oracle's record layouts."""
        from_tri = np.dtype([("v0", "f4", 3), ("v1", "f4", 3), ("v2", "f4", 3), ("n0", "f4", 3), ("n1", "f4", 3), ("n2", "f4", 3),
                             ("st", "f4", 6), ("material", "i4"), ("shape", "i4")])
        from_mat = np.dtype([("type", "i4"), ("albedo", "f4", 3), ("roughness", "f4"), ("metallic", "f4"), ("emissive", "f4", 3),
                             ("ior", "f4"), ("transmission", "f4", 3), ("fuzziness", "f4"),
                             ("texAlbedo", "i4"), ("texNormal", "i4"), ("texRoughness", "i4"), ("texMetallic", "i4"), ("texEmissive", "i4")])
        lib = self.lib
        tris = np.zeros(lib.RaylibAMD_SceneNumTriangles(self.scene), from_tri)
        mats = np.zeros(lib.RaylibAMD_SceneNumMaterials(self.scene), from_mat)
        lib.RaylibAMD_SceneExportTriangles(self.scene, tris.ctypes.data)
        lib.RaylibAMD_SceneExportMaterials(self.scene, mats.ctypes.data)
        return tris, mats

    def close(self):
        lib = self.lib
        # reference order: model, scene, camera, images (MainForm.cs:253-256)
        lib.Raylib_UnloadOBJModel(self.obj)
        lib.Raylib_DestroyScene(self.scene)
        lib.Raylib_DestroyCamera(self.camera)
        for ih in self._images:
            lib.Raylib_DestroyImage(ih)
