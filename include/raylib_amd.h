/*
 * raylib_amd.h -- ADDITIONAL exports of the MI355X raylib.  Nothing here exists in
 * the reference; raylib.h alone is the drop-in surface.  These exist because the
 * reference has no seed, no counters and no device boundary:
 *   - a deterministic seed (RendererSettings has no seed field and
 *     must not grow one, reference raylib_types.h:41-57)
 *   - ray / node / triangle counters (the reference cannot report Mrays/s,
 *     render/renderer.cc:114-208 has no counter)
 *   - a render entry that leaves the pixels in HBM and can restrict the work to a
 *     strided subset of the 8x8 cells (reference render/renderer.cc:21-22,305-319),
 *     which is how bench.py tiles an image over N ranks (one process per GPU)
 *   - host-logic introspection for CPU-only tests (flattened scene, BVH)
 *
 * Environment variables read by the library:
 *   RAYLIB_SEED    default seed (decimal, default 1) when RaylibAMD_SetSeed was not called
 *   RAYLIB_DEVICE  HIP device ordinal to use (default: LOCAL_RANK if set, else 0)
 *   RAYLIB_NUM_GPUS  N: Raylib_Render (and every whole-frame render) splits the frame's 8x8 cells round-robin over N devices of
 *                  this process -- devices RAYLIB_DEVICE .. RAYLIB_DEVICE + N - 1, or the list RAYLIB_GPU_MAP="d0,d1,..." (one
 *                  entry per rank; a device may be named more than once, which puts several ranks on it: tests) -- and gathers
 *                  the cells on the first device.  The frame is bit-identical to the one-device frame.  Default 1.
 *   RAYLIB_GATHER  rccl (default: grouped ncclSend / ncclRecv, librccl loaded at run time) | peer (hipMemcpyPeerAsync pushes)
 *   RAYLIB_DENOISER  1: the denoiser switch starts on (RaylibAMD_EnableDenoiser), so that unmodified front-ends get
 *                  Raylib_IsDenoiserSupported() == 1 and a working Raylib_Denoise.  Default 0: both return 0, as in the reference
 *                  builds without OIDN.
 */
#ifndef RAYLIB_AMD_H
#define RAYLIB_AMD_H

#include "raylib_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RaylibAMDStats {
	/* Every counter below counts work a KERNEL EXECUTED.  Camera samples of cells that were dropped from the job list (culledCells, below) are not in them. */
	uint64_t rays;            /* closest-hit + occlusion queries executed on the device (reference renderer.cc:129,194,70,79); a camera ray or sun ray that is
	                             decided by the root node's two boxes alone is one query that fetched one node record */
	uint64_t nodesVisited;    /* 64-byte BVH node records fetched (a float-box BVH4 node or a leaf-list record of four boxes counts as two) */
	uint64_t trisTested;      /* 64-byte triangle intersection records fetched */
	uint64_t shadedHits;      /* 64-byte triangle shading records fetched: one per shaded hit and one per cut-out candidate tested during a walk (the latter depends on the walk's order) */
	uint64_t texFetches;      /* 16-byte texels fetched (incl. the sky texel k_resolve looks up per sample of a cell outside the scene's silhouette) */
	uint64_t cameraSamples;   /* (pixel, sample) paths generated and traced by the megakernel (culledSamples are NOT in here: cameraSamples + culledSamples = pixels x spp) */
	uint64_t pixels;          /* pixels written (16 bytes each) */
	double   kernelMs;        /* HIP-event time of all kernels of the last render, on the library's stream */
	double   traceKernelMs;   /* ... of the path-tracing megakernel launches only */
	double   wallMs;          /* host wall clock of the last render call, incl. D2H copy when made */
	uint32_t traceLaunches;   /* megakernel launches in the last render (one per sample batch) */
	uint32_t numNodes;        /* BVH nodes of the scene */
	uint32_t numTriangles;
	uint32_t bvhDepth;
	uint64_t waveTrips;       /* bounce-loop trips summed over waves (a diagnostic: it depends on which wave drew which batch and differs from run to run) */
	uint32_t pathsPerWave;    /* schedule of the megakernel: 64 = k_trace (one path per lane), 128/192/256 = k_trace_pool */
	uint32_t ranks;           /* logical ranks (devices) that rendered the frame: 1, or RAYLIB_NUM_GPUS for a whole-frame render */
	/* ---- a whole-frame render over several ranks (RAYLIB_NUM_GPUS > 1): where the time went, so that a scaling loss can be attributed ---- */
	uint32_t gatherMode;      /* how the ranks' cells reached rank 0's device: 0 nothing to move (one rank, or every rank on rank 0's device),
	                             1 RCCL grouped ncclSend / ncclRecv, 2 hipMemcpyPeerAsync pushes (RAYLIB_GATHER=peer, or RCCL could not be initialised) */
	uint32_t rcclCommSize;    /* devices in the library's RCCL communicator (0: not initialised) */
	uint32_t devices;         /* distinct physical devices the ranks ran on */
	uint32_t jobHeads;        /* heads of the job list in the last megakernel launch: 8 = one per XCD (csrc/rl_dev_jobs.h TakeJobs), RAYLIB_JOB_HEADS overrides */
	double   gatherMs;        /* on rank 0's stream: from the end of rank 0's own kernels until every rank's cells are on its device (waiting for slower ranks included) */
	double   scatterMs;       /* k_scatter_cells: cell buffers -> row-major frame */
	double   rankKernelMs[16];/* per rank: HIP-event time of all its kernels (kernelMs is their maximum) */
	double   rankTraceMs[16]; /* per rank: ... of its megakernel launches (traceKernelMs is their maximum) */
	/* ---- cells outside the scene's silhouette (csrc/rl_cull.cc): dropped from the job list, filled with the miss shader's constant by k_resolve.
	 *      Nothing below was executed by any kernel; these are what the dropped samples WOULD have cost (one root-box query each, two with a sun),
	 *      kept apart so that a rate computed from `rays` is a rate of executed queries. ---- */
	uint32_t culledCells;     /* 8 x 8 cells left out of the job list (summed over ranks); RaylibAMD_CullCells on the same view returns this number */
	uint32_t listedCells;     /* cells in the job list (culledCells + listedCells = the frame's cells) */
	uint64_t culledSamples;   /* camera samples of those cells: pixels of the culled cells x spp */
	uint64_t culledRays;      /* queries (= root node records) those samples stand for: culledSamples x (2 with a sun, else 1) */
	/* ---- which tree the megakernel walked ---- */
	uint32_t treeWidth;       /* children per node: 2, 4 (64-byte grid nodes), 8 (80-byte grid nodes, octant-ordered children; scenes whose rays are expected to take
	                             many steps, RAYLIB_BVH8=0|1 overrides) or 0 = no tree (the leaf list of a scene of few leaves) */
	uint32_t nodeBytes;       /* bytes of one record counted in nodesVisited: 64, or 80 for the 8-wide tree */
	/* ---- the leaf-list kernel's lazy-reflectance instance (RaylibAMD_LastTraceLazy): 0 for every other kernel ---- */
	uint64_t litPaths;        /* traced paths that ended with light in them (or met a vertex whose reflectance may not be skipped): the ones whose reflectances were evaluated */
	uint64_t litFoldedInPlace;/* ... of them, those folded in place by their own lane instead of from an entry of the lit list by a whole wave (the lit list was full, or the path had more vertices than an entry holds) */
} RaylibAMDStats;

/* Seed of the per-(pixel, sample) streams of include/raylib_amd_rng.h. */
RAYLIB_API void     RaylibAMD_SetSeed(uint64_t seed);
RAYLIB_API uint64_t RaylibAMD_GetSeed(void);

/* Stats of the last call that reports them: Raylib_Render, RaylibAMD_RenderDevice, RaylibAMD_RenderCellsHost, RaylibAMD_RenderViews, a RaylibAMD_ProgressiveStep
 * that rendered, and the synchronous RaylibAMD_TraceRays, RaylibAMD_TraceRadiance, RaylibAMD_Gather, RaylibAMD_GatherAdaptive, RaylibAMD_BakeLightmap,
 * RaylibAMD_BakeLightmapAdaptive, RaylibAMD_BakeLightmapFiltered and RaylibAMD_FilterLightmap (the host entries, and the ...Device entries with a null stream).  A ...Device entry on a caller's stream reports nothing and leaves
 * the previous call's numbers in place.  With several ranks a Raylib_Render returns with its frame in flight: this call waits for it, and reports its counters
 * and times complete -- unless one of the synchronous calls above came after the render: then the numbers are that call's (ranks = 1), whenever the frame
 * completes.  One state per process. */
RAYLIB_API void RaylibAMD_GetLastStats(RaylibAMDStats* outStats);

/* 1 when a gfx950-capable HIP device is present and the kernels are loadable. */
RAYLIB_API int32_t RaylibAMD_DeviceAvailable(void);
/* 16 hex digits: SHA-256 prefix of the device sources + build flags this library was made from (software-raytracing_amd/Makefile BUILD_ID).
 * Hardware-counter profiles kept under profiles/ carry the id of the library they were taken from; bench.py compares. */
RAYLIB_API const char* RaylibAMD_BuildId(void);

/*
 * Render the cells {cellFirst, cellFirst + cellStride, ...} (8x8-pixel cells numbered
 * row-major over ceil(W/8) x ceil(H/8)) and leave RGBA float pixels in device memory.
 *   outDevice: device pointer; when cellStride == 1 && cellFirst == 0 it receives the
 *              row-major W*H*4-float image; otherwise it receives the rank's cells
 *              back to back, 64 pixels (row-major inside the cell) * 4 floats each.
 *              Must hold RaylibAMD_CellBufferFloats(...) floats.  May be 0: the
 *              library then renders into its own buffer (bench timing without output).
 * Returns 1 on success, 0 on failure (no device, bad handle).  Synchronous: the
 * library's stream has been synchronised when it returns.
 */
RAYLIB_API int32_t RaylibAMD_RenderDevice(const RendererSettings* settings, SceneHandle scene,
	CameraHandle camera, uint32_t cellFirst, uint32_t cellStride, void* outDevice);
/* Same, but the result is copied to host memory (RaylibAMD_CellBufferFloats(...) floats). */
RAYLIB_API int32_t RaylibAMD_RenderCellsHost(const RendererSettings* settings, SceneHandle scene,
	CameraHandle camera, uint32_t cellFirst, uint32_t cellStride, float* outHost);
RAYLIB_API uint64_t RaylibAMD_CellBufferFloats(uint32_t width, uint32_t height, uint32_t cellFirst, uint32_t cellStride);
RAYLIB_API uint32_t RaylibAMD_NumCells(uint32_t width, uint32_t height);

/* Closest-hit queries on the flat BVH (rays: n*6 floats o,d; out: n*11 words
 * {hit, t, p[3], n[3], paramU, paramV, material} as in oracle/flat_scene.h FlatHit). */
RAYLIB_API int32_t RaylibAMD_ClosestHit(SceneHandle scene, const float* rays, int32_t n, float tMin, void* outHits);

/* ---- batched ray queries ----------------------------------------------------------------------
 * A ray's result is what the reference's Scene::Hit(ray, tMin, tMax) returns, under the renderer's own-box and tie rules:
 * a triangle counts when tMin <= t <= tMax (Triangle::Hit), a sphere when tMin < t < tMax (Sphere::Hit), a cube when tMin <= t <= tMax (Cube::Hit).
 * With tMax = FLT_MAX and rayTime = 0 a SURFACE record is RaylibAMD_ClosestHit's, byte for byte, on every tree -- with one exception: the wide trees'
 * box tests replace an infinite 1/d by +-1e30, so a ray with a zero direction component whose other components are tiny (hits beyond about 1e20) may
 * miss on the grid-4 or 8-wide tree what the binary tree finds (RAYLIB_QUERY_TREE=2 walks the binary tree).  A NaN bound gives a miss.  Cut-out
 * triangles are alpha-tested during the walk, as in the render.
 * A query never reports a hit behind the origin: tMin < 0 (-inf included) is read as +0, and -0.0 is 0; a NaN tMin stays a NaN.  (The slack of the own-box
 * rule and of the walks' box tests is a factor above 1 and assumes t >= 0.)  A triangle at exactly tMin or exactly tMax counts, so [t, t] finds the surface at t;
 * tMin > tMax is empty.  Each primitive is held to its own interval: a sphere at exactly tMax is out of range and hides nothing, so a cube or a triangle at
 * that same t is reported.  Checked against a loop over every primitive: tests/test_gpu_ray_query_intervals.py, tests/test_gpu_analytic_edges.py. */
typedef struct RaylibAMDRay {          /* 32 bytes; on the device entry an array of them must be 16-byte aligned */
	float org[3]; float tMin;
	float dir[3]; float tMax;
} RaylibAMDRay;
typedef struct RaylibAMDHitT {         /* 16 bytes; a miss: prim = -1, t = b1 = b2 = 0 */
	float t;
	int32_t prim;                      /* the triangle's index in RaylibAMD_SceneExportTriangles order, RAYLIB_AMD_PRIM_SPHERE | k, or RAYLIB_AMD_PRIM_CUBE | k */
	float b1, b2;                      /* the walk's barycentric pair: p = v0 + b1 (v1 - v0) + b2 (v2 - v0); 0 for spheres and cubes */
} RaylibAMDHitT;
#define RAYLIB_AMD_QUERY_ANY     0     /* out: uint32_t per ray, 1 when anything is hit in the interval (may stop at the first accepted candidate) */
#define RAYLIB_AMD_QUERY_CLOSEST 1     /* out: RaylibAMDHitT per ray */
#define RAYLIB_AMD_QUERY_SURFACE 2     /* out: the 44-byte record of RaylibAMD_ClosestHit per ray; outPrim (may be null): int32_t primitive per ray, -1 for a miss */
#define RAYLIB_AMD_PRIM_SPHERE 0x10000000
#define RAYLIB_AMD_PRIM_CUBE   0x20000000
/* n rays from host memory, results to host memory; synchronous.  rayTime: the shutter time at which moving cubes are placed.  The library keeps its
 * device staging buffers and grows them; a warm call allocates nothing.  Returns 1 (n == 0 included), or 0 with nothing written when a pointer is null with
 * n > 0, n < 0, the scene is not finalized, the kind is unknown, rayTime is not finite, the scene's BVH is deeper than 64 levels, or there is no device.
 * RaylibAMD_GetLastStats then reports rays, nodesVisited, trisTested, shadedHits, texFetches, kernelMs, wallMs and the tree walked. */
RAYLIB_API int32_t RaylibAMD_TraceRays(SceneHandle scene, int32_t kind, const RaylibAMDRay* rays, int32_t n, float rayTime, void* out, int32_t* outPrim);
/* The same on device pointers (rays, out, outPrim on rank 0's device; other pointers are refused).  rays must be 16-byte aligned, out 16-byte aligned for
 * CLOSEST and 4-byte aligned otherwise, outPrim 4-byte aligned (refused otherwise).  stream == NULL: the library's stream, synchronous, with
 * stats.  A non-null hipStream_t: the scene's upload (and a tree or table the query needs for the first time) happens first and synchronously, then the
 * query is enqueued on that stream and the call returns; the stats are left alone.  With RAYLIB_NUM_GPUS > 1 queries run on rank 0's device. */
RAYLIB_API int32_t RaylibAMD_TraceRaysDevice(SceneHandle scene, int32_t kind, const RaylibAMDRay* rays, int32_t n, float rayTime, void* out, int32_t* outPrim,
        void* stream);
/* Which tree and kernel instance a query of this kind would walk under the current environment (csrc/rl_plan.cc PlanQuery; RAYLIB_QUERY_TREE=2|4|8 forces a
 * tree, and a tree the scene lacks falls back to the next of 8-wide, grid-4, binary).  No device needed.  Returns 1, -1 when the BVH is deeper than 64 levels,
 * 0 for a bad argument, an unknown kind or a scene not finalized. */
typedef struct RaylibAMDQueryPlan {
	int32_t tree;             /* as RaylibAMDRenderPlan.tree: 1 binary, 3 4-wide grid nodes, 4 8-wide */
	uint32_t treeWidth;       /* 2, 4 or 8 */
	uint32_t nodeBytes;       /* bytes of one record counted in nodesVisited */
	int32_t stack;            /* the instance's traversal stack */
	int32_t prims;            /* the scene holds spheres or cubes */
	int32_t early;            /* the occlusion query stops at its first accepted candidate */
} RaylibAMDQueryPlan;
RAYLIB_API int32_t RaylibAMD_PlanRayQuery(SceneHandle scene, int32_t kind, RaylibAMDQueryPlan* out);

/* ---- primary-hit G-buffer ----------------------------------------------------------------------------
 * What is in each pixel: depth, primitive, barycentrics, world position, normal and material index, and the five deterministic debug modes as planes, from ONE
 * walk of each pixel's camera ray on the tree the ray queries prefer (csrc/rl_k_gbuffer.inl; k_aov walks the binary tree once per mode).
 * G1  Ray.  Pixel (x, y) of a W x H frame uses the ray the debug render modes use: the stream is raylib_rng_begin(seed, y * W + x, 0) and the ray is
 *     CameraRay(camera, (float)x / (float)W, (float)y / (float)H, stream) -- origin, direction and shutter time; not jittered.  The seed is RaylibAMD_GetSeed()
 *     at the call.  It is what RaylibAMD_EvalCameraRays returns for record i = y * W + x with uv = (x / W, y / H).
 * G2  Hit.  The closest hit the render finds for that ray, with settings->rayTMin used as the render uses it: not raised to 0 and without the ray queries'
 *     widened own-box rule (the two agree wherever no surface lies within rayTMin of the camera).  Cut-outs are alpha-tested in the walk; spheres and cubes
 *     are placed at the ray's time.  The hit does not depend on the tree walked, with the ray queries' caveat for the wide trees'
 *     +-1e30 reciprocal (hits beyond about 1e20).
 * G3  Planes, row-major, W * H records each; any subset may be asked for (a null pointer: not asked for, nothing written):
 *       hit            16 bytes  RaylibAMDHitT {t, prim, b1, b2}: prim in RaylibAMD_SceneExportTriangles order, RAYLIB_AMD_PRIM_SPHERE | k or
 *                                RAYLIB_AMD_PRIM_CUBE | k; a miss is {0, -1, 0, 0}
 *       surface        44 bytes  the RaylibAMD_ClosestHit record {hit, t, p[3], n[3], paramU, paramV, material}; a miss is zeros with material -1
 *       albedo         16 bytes  what Raylib_Render writes for the pixel in RAYLIB_RENDERMODE_Albedo, bit for bit, alpha 1 -- the second walk along the
 *                                reflection off a mirror-like surface included; a miss is (0, 0, 0, 1)
 *       surfaceNormal, microNormal, texcoord, emission   16 bytes each: as Raylib_Render in RAYLIB_RENDERMODE_SurfaceNormal, _MicrosurfaceNormal, _Texcoord,
 *                                _Emission, bit for bit, alpha 1; a miss is (0, 0, 0, 1)
 *     "Raylib_Render" means the same settings apart from renderMode, the same scene, camera and seed.  The surface record and the colour planes come from one
 *     surface interaction: the debug modes build it with its tangent frame and RaylibAMD_ClosestHit without, and the frame changes no other field.
 * G4  samplesPerPixel, maxPathLength and renderMode of the settings are not read: the debug modes are one sample.
 * G5  No output bit depends on the tree walked, on how pixels are dealt to lanes and waves, on which other planes were asked for, or on whether the trees are
 *     fresh or refitted by RaylibAMD_SceneMoveTriangles; after a move the call sees the moved triangles.
 * G6  Refused (0, nothing written): a null settings, scene, camera or planes struct; no plane asked for; W or H equal to 0, or W * H above 2^31 - 1; a rayTMin
 *     that is not finite; a scene that is not finalized; a BVH deeper than 64 levels; no device; on the device entry a plane pointer off rank 0's device, a
 *     16-byte plane that is not 16-byte aligned or `surface` not 4-byte aligned; on the images entry a handle that is unknown, or the same image twice.
 * Still out: the Reflectance mode (it draws random numbers behind the camera's, and the reference reads an uninitialised frame there); jittered samples
 * s >= 1; a views-batch twin; splitting the frame over ranks.  (RaylibAMD_Denoise has no depth or position guide -- it would change that filter's statement;
 * RaylibAMD_FilterVariance, statements S3 to S7, is the filter guided by this G-buffer's `hit` and `surface` planes.) */
typedef struct RaylibAMDGBufferPlanes {
	RaylibAMDHitT* hit; void* surface;
	float *albedo, *surfaceNormal, *microNormal, *texcoord, *emission;   /* 4 floats per pixel each */
} RaylibAMDGBufferPlanes;
/* Planes in host memory; synchronous.  The library keeps its device staging buffers and grows them, as the query entries do.  RaylibAMD_GetLastStats then
 * reports rays (the albedo plane's mirror follow-ups included), nodesVisited, trisTested, shadedHits, texFetches, cameraSamples = pixels = W * H, kernelMs,
 * wallMs, treeWidth, nodeBytes and ranks = 1. */
RAYLIB_API int32_t RaylibAMD_RenderGBuffer(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, const RaylibAMDGBufferPlanes* hostPlanes);
/* The same on device pointers, under RaylibAMD_TraceRaysDevice's rules: stream == NULL is the library's stream, synchronous, with stats; with a hipStream_t the
 * uploads (the scene with its textures, a tree or the slot table needed for the first time) happen first and synchronously, then the launch is enqueued on that
 * stream -- behind a RaylibAMD_SceneMoveTrianglesDevice enqueued there -- and the call returns; the stats are left alone.  With RAYLIB_NUM_GPUS > 1 it runs on
 * rank 0's device, behind frames in flight. */
RAYLIB_API int32_t RaylibAMD_RenderGBufferDevice(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, const RaylibAMDGBufferPlanes* devicePlanes,
        void* stream);
/* The denoiser's two guides in one launch: each image given is resized to the viewport as Raylib_Render does and holds its plane on the device afterwards, as
 * after Raylib_Render in that mode -- Raylib_Denoise, RaylibAMD_Denoise, Raylib_PostProcess and Raylib_DumpImageData work on it unchanged.  Either handle may
 * be 0, not both.  Synchronous, with stats. */
RAYLIB_API int32_t RaylibAMD_RenderGuides(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, ImageHandle albedo, ImageHandle microNormal);
/* The tree and instance a G-buffer would walk: RaylibAMD_PlanRayQuery's answer for RAYLIB_AMD_QUERY_SURFACE under the current environment (one planner,
 * csrc/rl_plan.cc), early = 0.  No device needed.  Returns 1, -1 when the BVH is deeper than 64 levels, 0 for a null argument or a scene not finalized. */
RAYLIB_API int32_t RaylibAMD_PlanGBuffer(SceneHandle scene, RaylibAMDQueryPlan* out);

/* ---- temporal reprojection: per-pixel motion and an accumulated history ---------------------------------
 * Where each pixel's surface point was in the previous frame (a motion plane, a finish stage on the G-buffer's walk: csrc/rl_k_motion.inl), and a blend of
 * this frame's colour with what the previous result holds there, rejected where the surface differs (csrc/rl_temporal.hip).  The library remembers nothing:
 * the caller holds last frame's positions (it gave them to RaylibAMD_SceneMoveTriangles), last frame's camera and last frame's outputs.
 * Arithmetic: float, single IEEE operations without FMA, a / b and sqrt correctly rounded; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z;
 * cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x); one source for the device and the host (csrc/rl_motion.h, csrc/rl_temporal.h).
 * T1  Ray and hit.  G1 and G2 unchanged: the `hit` plane is RaylibAMD_RenderGBuffer's `hit` plane byte for byte, on every tree.
 * T2  Previous point.  A hit on triangle i of [first, first + count) with the walk's pair (b1, b2), on the vertices p0, p1, p2 = prevPositions + 9 (i - first):
 *     P' = (p0 + b1 * (p1 - p0)) + b2 * (p2 - p0) per component, and e = P' - o'.  Every other hit (a triangle outside the range, a sphere, a cube -- a
 *     moving cube is taken where the ray found it): P' = o + t * d with the ray's own origin, and e = P' - o'.  A miss: the point at infinity, e = d.
 * T3  Projection.  The previous camera's origin, top_left, horizontal, vertical as RaylibAMD_CameraExport gives them (o', c, h, v); a thin-lens camera is
 *     projected through its lens centre o'.  w = cross(h, v), a = c - o', lambda = dot(a, w) / dot(e, w), q = lambda * e - a,
 *     s = dot(q, h) / dot(h, h), u = dot(q, v) / dot(v, v), prevX = s * (float)W, prevY = (1.0f - u) * (float)H: the units in which pixel x has s = x / W
 *     (G1), so an unmoved point lands on its own integer coordinates, up to rounding.  prevT = sqrt(dot(e, e)) for a hit -- the t the previous frame's hit
 *     plane holds there --, 0 for a miss.
 * T4  Status.  RAYLIB_AMD_MOTION_NONE with the three floats +0 when lambda is not finite or not > 0 (the point is behind or in the plane of the previous
 *     camera); else RAYLIB_AMD_MOTION_SURFACE for a hit, RAYLIB_AMD_MOTION_SKY for a miss.  prevX, prevY may lie outside the frame: the consumer decides.
 * T5  No bit of the motion plane depends on the tree walked, on the lanes, on whether `hit` was asked for, or on fresh against refitted trees.
 * T6  Refused (0, nothing written): G6's list; both planes null; first < 0, count < 0 or first + count past the scene's triangles; count > 0 with null
 *     positions; on the host entry a previous position that is not finite (scanned first); a prevCamera that is not a camera; on the device entry a plane or
 *     the positions off rank 0's device, a plane not 16-byte aligned, positions not 4-byte aligned.
 * T7  Accumulation, per pixel p = (x, y) with motion record m and hit record c.  Reset -- outColour = (colour.rgb, 1), outLength = 1 -- when m.status is
 *     NONE, when there is no history, when floor(prevX) or floor(prevY) is outside [-1, 2^31], or when Wsum below is 0.  Else fx = floor(m.prevX),
 *     wx = m.prevX - fx, ox = 1 - wx, likewise y; the taps (fx + i, fy + j) in the order (0,0), (1,0), (0,1), (1,1) with weights ox * oy, wx * oy, ox * wy,
 *     wx * wy.  A tap counts when it lies in the frame, its weight is > 0, history.length > 0 there, history.hit.prim == c.prim (-1, the sky, matches -1),
 *     and, for SURFACE, |history.hit.t - m.prevT| <= depthTolerance * m.prevT.  In tap order from 0: Wsum += w, S.rgb += w * history.colour.rgb,
 *     L += w * history.length.  hist = S / Wsum, n = L / Wsum, n' = min(n + 1, maxLength), outColour.rgb = hist + (colour - hist) / n', alpha 1,
 *     outLength = n'.  With identity motion this is the running mean of the frames bit for bit; after a disocclusion it restarts.
 * T8  Accumulation refused (0, nothing written): a null params, colour, hit, motion, outColour or outLength; a history with a null member; W or H equal to 0 or
 *     W * H above 2^31 - 1; depthTolerance not finite or < 0; maxLength not finite or < 1; an output plane that is one of the history's planes (the taps read
 *     neighbours, so in place is a race); no device; on the device entry a pointer off rank 0's device, a colour, hit or motion plane not 16-byte aligned or
 *     a length plane not 4-byte aligned.
 * Still out: neighbourhood colour clamping; an ImageHandle entry; a views-batch twin; motion for spheres and moving cubes; splitting over ranks.  (Moment
 * planes and the variance-guided filter: statements S1 to S7 below.) */
typedef struct RaylibAMDMotion { float prevX, prevY, prevT; uint32_t status; } RaylibAMDMotion;   /* 16 bytes */
#define RAYLIB_AMD_MOTION_NONE    0   /* no previous position: zeros */
#define RAYLIB_AMD_MOTION_SURFACE 1
#define RAYLIB_AMD_MOTION_SKY     2
typedef struct RaylibAMDMotionPlanes { RaylibAMDHitT* hit; RaylibAMDMotion* motion; } RaylibAMDMotionPlanes;   /* either may be NULL, not both */
typedef struct RaylibAMDMotionParams {
	CameraHandle prevCamera;          /* 0: the current camera */
	int32_t first, count;             /* triangles [first, first + count) in RaylibAMD_SceneExportTriangles order had other vertices last frame */
	const float* prevPositions;       /* count x 9 floats, RaylibAMD_SceneMoveTriangles' layout; host memory on the host entry, rank 0's device memory on the
	                                     device entry; NULL with count == 0 */
} RaylibAMDMotionParams;
/* Planes and previous positions in host memory; synchronous, with RaylibAMD_RenderGBuffer's stats (rays, cameraSamples = pixels = W * H, kernelMs, ...). */
RAYLIB_API int32_t RaylibAMD_RenderMotion(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, const RaylibAMDMotionParams* params,
        const RaylibAMDMotionPlanes* hostPlanes);
/* The same on device pointers, under RaylibAMD_RenderGBufferDevice's rules for the stream, the ordering behind a move enqueued there, the stats and the ranks. */
RAYLIB_API int32_t RaylibAMD_RenderMotionDevice(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, const RaylibAMDMotionParams* params,
        const RaylibAMDMotionPlanes* devicePlanes, void* stream);
/* T2 to T4 on the host, without a device and without a walk: `rays` holds W * H records of 7 floats as RaylibAMD_EvalCameraRays returns them (origin,
 * direction, time; the time is not read) and `hit` the frame's hit plane.  `camera` is the previous camera when params->prevCamera is 0.  The scene gives the
 * range its bound and nothing else.  Refusals: T6's that need no device. */
RAYLIB_API int32_t RaylibAMD_MotionHost(uint32_t width, uint32_t height, SceneHandle scene, CameraHandle camera, const RaylibAMDMotionParams* params,
        const float* rays, const RaylibAMDHitT* hit, RaylibAMDMotion* outMotion);
/* RaylibAMD_PlanGBuffer's answer: the motion launch walks what the G-buffer walks. */
RAYLIB_API int32_t RaylibAMD_PlanMotion(SceneHandle scene, RaylibAMDQueryPlan* out);

typedef struct RaylibAMDTemporalParams { float depthTolerance; float maxLength; } RaylibAMDTemporalParams;   /* relative, finite, >= 0;  >= 1, finite */
typedef struct RaylibAMDTemporalFrame { const float* colour; const RaylibAMDHitT* hit; const float* length; } RaylibAMDTemporalFrame;   /* W*H*4 floats, W*H records, W*H floats */
/* T7 on arrays in host memory; synchronous, with stats (pixels = W * H, kernelMs, wallMs, ranks = 1).  colour: W * H * 4 floats (what RaylibAMD_RenderDevice
 * leaves at cellFirst 0, cellStride 1, or any such plane); history: the previous call's outColour, that frame's hit plane and its outLength, or NULL for the
 * first frame. */
RAYLIB_API int32_t RaylibAMD_TemporalAccumulate(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
        const RaylibAMDMotion* motion, const RaylibAMDTemporalFrame* history, float* outColour, float* outLength);
/* The same on pointers of rank 0's device: stream == NULL is the library's stream, synchronous, with stats; with a hipStream_t the launch is enqueued there --
 * behind a RaylibAMD_RenderMotionDevice enqueued there, with no host synchronisation between them -- and the stats are left alone. */
RAYLIB_API int32_t RaylibAMD_TemporalAccumulateDevice(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
        const RaylibAMDMotion* motion, const RaylibAMDTemporalFrame* history, float* outColour, float* outLength, void* stream);
/* The host oracle: the same arrays, no device. */
RAYLIB_API int32_t RaylibAMD_TemporalAccumulateHost(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
        const RaylibAMDMotion* motion, const RaylibAMDTemporalFrame* history, float* outColour, float* outLength);

/* ---- variance-guided filter: temporal moments and an a-trous pass on planes ----------------------------
 * The stage behind the accumulation: the luminance moments carried through the same reprojection, a per-pixel variance derived from them, and an edge-avoiding
 * a-trous filter whose colour tolerance is that variance and whose guides are the G-buffer's own `hit` and `surface` planes (SVGF's core: Schied et al. 2017).
 * Albedo is the caller's: divide by the G-buffer's albedo plane before the accumulation and multiply behind the filter.  Arithmetic: float, single IEEE
 * operations without FMA, a / b and sqrt correctly rounded, expf the library's exact one (csrc/rl_glibc_math.h expf_); a + b + c is (a + b) + c; sums run in
 * the stated tap order from +0; one source for the device and the host (csrc/rl_temporal.h, csrc/rl_variance.h).
 * S1  Moments.  For this frame's pixel Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b and m = (Y, Y * Y).  Wherever T7 resets, outMoments = m.  Wherever T7
 *     blends, on the very taps and weights T7 counted and in T7's tap order from 0: Mk += w * history.moments[k], k = 0, 1; then M = Mk / Wsum and
 *     outMoments = M + (m - M) / n'.
 * S2  outColour and outLength of RaylibAMD_TemporalAccumulateMoments are RaylibAMD_TemporalAccumulate's bytes for the same inputs.  Refused: T8's list, a null
 *     outMoments, a history with a null member (moments included), an output that is one of the history's planes, and on the device entry a moments plane that
 *     is off rank 0's device or not 8-byte aligned.
 * S3  Participants.  A pixel whose hit.prim is -1 passes through -- outColour = (colour.rgb, 1), outVariance = +0 -- and is never a tap.  Every other pixel
 *     takes part, with P and n its surface record's p and n.  A colour channel that is not finite is read as 0, everywhere.
 * S4  Guide distance between a centre p and a tap q: g = dn + dp.  dn = ((e.x e.x + e.y e.y) + e.z e.z) * invN with e = n(q) - n(p).  With d = P(q) - P(p),
 *     dd = (d.x d.x + d.y d.y) + d.z d.z and nd = (n(p).x d.x + n(p).y d.y) + n(p).z d.z: dp = (nd * nd) / dd * invPl, and 0 where dd == 0.
 *     invN = 1 / (sigmaNormal * sigmaNormal), invPl = 1 / (sigmaPlane * sigmaPlane), computed once on the host for both paths.  dp is a ratio -- the squared
 *     sine of the angle between d and p's tangent plane -- and so has no scene scale.
 * S5  Initial variance of a participant.  Where length >= historyLength: v0 = max(0, m2 - m1 * m1) with the pixel's own moments.  Elsewhere, over the 7 x 7
 *     window q = p + (dx, dy), dy outer and dx inner, both -3 .. 3, the participants inside the frame: w = expf(-g), sums of w, w * m1(q), w * m2(q);
 *     M1 = S1 / Sw, M2 = S2 / Sw and v0 = max(0, M2 - M1 * M1) * (historyLength / max(length, 1)).  max(0, v) is v where v > 0, else +0 (a NaN is 0).
 * S6  Iteration i = 0 .. K - 1, step s = 2^i, on I_0 = colour and var_0 = v0.  gv(p): var_i under the 3 x 3 kernel at step 1 (dy outer, dx inner; weights
 *     1/4 at the centre, 1/8 on the edges, 1/16 at the corners) over the participants inside the frame, divided by the sum of the weights used.
 *     lambda = 1 / (sigmaLuminance * sqrt(gv(p)) + 1e-6f).  Taps q = p + s * (dx, dy), dy outer and dx inner, both -2 .. 2, k = {1/16, 1/4, 3/8, 1/4, 1/16};
 *     taps outside the frame or not participating are skipped.  dl = |Y(I_i(q)) - Y(I_i(p))| * lambda, w = (k[dx+2] * k[dy+2]) * expf(-(dl + g)).
 *     I_{i+1}(p) = sum(w * I_i(q)) / sum(w) per channel, var_{i+1}(p) = sum((w * w) * var_i(q)) / (sum(w) * sum(w)).  The centre tap always counts
 *     (w = 9/64), so the divisor is >= 9/64.  outColour = (I_K, 1), outVariance = var_K.
 * S7  No output bit depends on how pixels are dealt to lanes, tiles or launches, nor on whether outVariance was asked for.
 * Filter refused (0, nothing written): a null planes struct, a null colour, moments, length, hit, surface or outColour; W or H equal to 0, or W * H above
 *     2^31 - 1; iterations outside 1 .. 6; sigmaLuminance, sigmaNormal or sigmaPlane not finite or outside [1e-3, 1e3]; historyLength not finite or < 1;
 *     outColour equal to colour; no device; on the device entry a pointer off rank 0's device, colour, hit or outColour not 16-byte aligned, moments not 8-byte
 *     aligned, surface, length or outVariance not 4-byte aligned.
 * Still out: albedo demodulation inside the call, neighbourhood colour clamping, an ImageHandle entry, a motion launch that emits `surface`, splitting over
 * ranks. */
typedef struct RaylibAMDTemporalMomentsFrame {      /* RaylibAMDTemporalFrame and the previous call's outMoments: W * H * 2 floats */
	const float* colour; const RaylibAMDHitT* hit; const float* length; const float* moments;
} RaylibAMDTemporalMomentsFrame;
/* T7 with S1 on arrays in host memory; synchronous, with RaylibAMD_TemporalAccumulate's stats.  outMoments: W * H * 2 floats. */
RAYLIB_API int32_t RaylibAMD_TemporalAccumulateMoments(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
        const RaylibAMDMotion* motion, const RaylibAMDTemporalMomentsFrame* history, float* outColour, float* outLength, float* outMoments);
/* The same on pointers of rank 0's device, under RaylibAMD_TemporalAccumulateDevice's rules for the stream, the stats and the ranks. */
RAYLIB_API int32_t RaylibAMD_TemporalAccumulateMomentsDevice(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
        const RaylibAMDMotion* motion, const RaylibAMDTemporalMomentsFrame* history, float* outColour, float* outLength, float* outMoments, void* stream);
/* The host oracle: the same arrays, no device. */
RAYLIB_API int32_t RaylibAMD_TemporalAccumulateMomentsHost(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
        const RaylibAMDMotion* motion, const RaylibAMDTemporalMomentsFrame* history, float* outColour, float* outLength, float* outMoments);

typedef struct RaylibAMDVarianceFilterParams {      /* NULL: 5, 4, 0.35, 0.1, 4 */
	int32_t iterations;                             /* K, 1 .. 6 */
	float sigmaLuminance, sigmaNormal, sigmaPlane;  /* each finite, in [1e-3, 1e3] */
	float historyLength;                            /* finite, >= 1: the length from which the temporal variance is trusted (S5) */
} RaylibAMDVarianceFilterParams;
typedef struct RaylibAMDVarianceFilterPlanes {      /* W * H records each, row-major; all required */
	const float* colour;                            /* 4 floats per pixel: the accumulation's outColour */
	const float* moments;                           /* 2 floats per pixel: its outMoments */
	const float* length;                            /* 1 float per pixel: its outLength */
	const RaylibAMDHitT* hit;                       /* the frame's hit plane, as RaylibAMD_RenderGBuffer or RaylibAMD_RenderMotion writes it */
	const void* surface;                            /* the G-buffer's 44-byte surface records */
} RaylibAMDVarianceFilterPlanes;
/* S3 to S7 on arrays in host memory; synchronous, with stats (pixels = W * H, kernelMs over all 2 + K launches, traceLaunches = 2 + K, wallMs, ranks = 1).
 * outColour: W * H * 4 floats; outVariance: W * H floats, or NULL.  The library keeps its scratch (48 bytes per pixel on the device, and a host call's
 * staging) and grows it; a warm call allocates nothing. */
RAYLIB_API int32_t RaylibAMD_FilterVariance(uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams* params, const RaylibAMDVarianceFilterPlanes* planes,
        float* outColour, float* outVariance);
/* The same on pointers of rank 0's device, under RaylibAMD_TemporalAccumulateDevice's rules for the stream, the stats and the ranks: on a hipStream_t the
 * launches are enqueued there, behind a RaylibAMD_TemporalAccumulateMomentsDevice enqueued there, with no host synchronisation between them.  Calls on
 * different streams share the scratch and are ordered one behind the other by an event of the library's. */
RAYLIB_API int32_t RaylibAMD_FilterVarianceDevice(uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams* params, const RaylibAMDVarianceFilterPlanes* planes,
        float* outColour, float* outVariance, void* stream);
/* The host oracle: the same arrays, no device. */
RAYLIB_API int32_t RaylibAMD_FilterVarianceHost(uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams* params, const RaylibAMDVarianceFilterPlanes* planes,
        float* outColour, float* outVariance);

/* ---- ordered multi-hit ray queries -------------------------------------------------------------
 * The first maxHits surfaces a ray crosses, in order, and how many it crosses in all: ordered transparency and depth peeling, thickness and x-ray views,
 * shell and CSG tests, the inside / outside parity of a point -- in one walk of the tree, where peeling with CLOSEST walks it once per layer.
 * RaylibAMD_TraceRays keeps refusing kind 3; these are entries of their own (csrc/rl_k_multihit.inl is the walk, RaylibAMD_TraceRaysAllHost the oracle).
 *   M1. Accepted set.  Triangle k is accepted for a ray exactly when a CLOSEST query on [tMin, tMax] could return it: its plane t lies in [max(tMin, 0), tMax]
 *        (tMin < 0 is read as +0, as above), the barycentric test passes, the renderer's own-box rule passes under the ray's own tMin (with the ray queries'
 *        widened "own box ends before tMin"), and the cut-out test passes.  The set is a property of the ray and the triangle alone.  A NaN bound or
 *        tMin > tMax gives the empty set.
 *   M2. Order.  The accepted triangles are sorted by (t, slot) ascending, slot being the triangle's place in the scene's leaf order -- the key CLOSEST breaks
 *        ties with.  Row i of outHits holds the first min(maxHits, |set|) of them as {t, prim, b1, b2}, prim the index in RaylibAMD_SceneExportTriangles order,
 *        and behind them miss records {0, -1, 0, 0}.  So outHits[i * maxHits] is CLOSEST's record byte for byte, and maxHits == 1 is CLOSEST.  Within an
 *        exact-t tie the order follows the slots: the same on every tree of one build; it may change with RaylibAMD_SceneRebuild, as CLOSEST's winner does.
 *   M3. Count.  With outCount non-null, outCount[i] = |set|: every crossing of the interval, however small maxHits is.  With outCount null the walk may
 *        prune with its maxHits-th key and visits less.
 *   M4. Independence.  The result does not depend on the tree walked, the order of the walk, how the call is cut into waves, or whether the trees were built
 *        fresh or refitted by RaylibAMD_SceneMoveTriangles (the host oracle refreshes the host's triangles after a move first).
 *   M5. Refusals (0, nothing written): rays or outHits null with n > 0; n < 0; maxHits outside 1 .. RAYLIB_AMD_MAX_HITS; a rayTime that is not finite; a scene
 *        that is not finalized; a scene that holds spheres or cubes (a sphere has two crossings and the walk's sphere test reports one: out of scope, and
 *        refused rather than answered in part); a BVH deeper than 64 levels; n * maxHits above 2^31 - 1; no device (the plain and the device entry; the host
 *        entry needs none); on the device entry a pointer off rank 0's device, rays or outHits not 16-byte aligned, outCount not 4-byte aligned.  n == 0 returns 1.
 * Still out: spheres and cubes, more than RAYLIB_AMD_MAX_HITS records per ray (the count is complete all the same), a walk on the grid-4 tree.
 * Checked against peeling through the brute-force oracle: tests/test_ray_query_all_host.py, tests/test_gpu_ray_query_all.py. */
#define RAYLIB_AMD_MAX_HITS 16
/* n rays from host memory, results to host memory; synchronous, on the device.  outHits: n * maxHits RaylibAMDHitT, row i = ray i; outCount: n uint32_t, or null.
 * rayTime is checked and otherwise unused (triangles do not move with the shutter).  RaylibAMD_GetLastStats then reports rays, nodesVisited, trisTested,
 * kernelMs, wallMs and the tree walked. */
RAYLIB_API int32_t RaylibAMD_TraceRaysAll(SceneHandle scene, const RaylibAMDRay* rays, int32_t n, float rayTime, int32_t maxHits, RaylibAMDHitT* outHits, uint32_t* outCount);
/* The same on device pointers, with the pointer, alignment, stream, stats and multi-rank rules of RaylibAMD_TraceRaysDevice: stream == NULL is the library's
 * stream, synchronous, with stats; a non-null hipStream_t gets the call enqueued behind the synchronous uploads.  The call is ordered behind a move of the
 * scene's triangles and behind multi-rank frames in flight as a ray query is. */
RAYLIB_API int32_t RaylibAMD_TraceRaysAllDevice(SceneHandle scene, const RaylibAMDRay* rays, int32_t n, float rayTime, int32_t maxHits, RaylibAMDHitT* outHits, uint32_t* outCount,
        void* stream);
/* The oracle: statements M1 to M3 over every triangle, no tree, no device. */
RAYLIB_API int32_t RaylibAMD_TraceRaysAllHost(SceneHandle scene, const RaylibAMDRay* rays, int32_t n, float rayTime, int32_t maxHits, RaylibAMDHitT* outHits, uint32_t* outCount);
/* Which tree and kernel instance those calls would walk under the current environment (csrc/rl_plan.cc PlanQueryAll): the 8-wide tree where PlanRayQuery
 * would take it, else the binary tree -- there is no grid-4 instance, so RAYLIB_QUERY_TREE=4 gives the binary tree as =2 does.  wantCount (outCount non-null)
 * selects the instance that never prunes; the tree is the same.  `early` is 0.  No device needed.  Returns 1, -1 when the BVH is deeper than 64 levels, 0 for a
 * null argument, maxHits outside 1 .. RAYLIB_AMD_MAX_HITS, a scene not finalized or one that holds spheres or cubes. */
RAYLIB_API int32_t RaylibAMD_PlanRayQueryAll(SceneHandle scene, int32_t maxHits, int32_t wantCount, RaylibAMDQueryPlan* out);

/* ---- batched nearest-point queries ---------------------------------------------------------------
 * Which triangle of the scene is nearest to a point, how far away, and where on it -- for contact and collision behind RaylibAMD_SceneMoveTriangles, distance
 * fields, snapping points onto geometry, attribute transfer.  The result equals a loop over every triangle bit for bit, with no slack factor anywhere, on
 * every tree, fresh or refitted (csrc/rl_nearest.h holds the statements for the host oracle and the kernel alike; csrc/rl_k_nearest.inl is the walk).
 * Everything is float, without FMA.  1.0f / x and a / b are the IEEE values.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 * For point p and triangle k, in RaylibAMD_SceneExportTriangles order, with vertices v0 v1 v2:
 *   N1. Closest point (Ericson's regions; the first condition that holds decides):
 *        ab = v1 - v0, ac = v2 - v0, ap = p - v0; d1 = dot(ab, ap), d2 = dot(ac, ap).  If d1 <= 0 && d2 <= 0: (b1, b2) = (0, 0).
 *        bp = p - v1; d3 = dot(ab, bp), d4 = dot(ac, bp).  If d3 >= 0 && d4 <= d3: (1, 0).
 *        vc = d1*d4 - d3*d2.  If vc <= 0 && d1 >= 0 && d3 <= 0: (d1 / (d1 - d3), 0).
 *        cp = p - v2; d5 = dot(ab, cp), d6 = dot(ac, cp).  If d6 >= 0 && d5 <= d6: (0, 1).
 *        vb = d5*d2 - d1*d6.  If vb <= 0 && d2 >= 0 && d6 <= 0: (0, d2 / (d2 - d6)).
 *        va = d3*d6 - d5*d4; e = d4 - d3, g = d5 - d6.  If va <= 0 && e >= 0 && g >= 0: w = e / (e + g), (1.0f - w, w).
 *        Otherwise den = 1.0f / ((va + vb) + vc), (vb*den, vc*den).
 *        q = (v0 + b1*ab) + b2*ac; r = p - q; E = dot(r, r).
 *   N2. Own box.  lo, hi are the componentwise least and greatest of the three vertices, found by comparisons.  Per axis: t = lo - p, u = p - hi,
 *        d = t > 0 ? t : (u > 0 ? u : 0).  B = (dx*dx + dy*dy) + dz*dz.
 *   N3. The triangle's distance.  D = (E >= B) ? E : B.  A NaN E from a degenerate triangle therefore yields B.
 *        In exact arithmetic E >= B always holds, so the rule only moves D at rounding level.  It buys this: the binary tree's float boxes are nested exactly
 *        (a parent is the min / max of its children), the grid boxes of the 4-wide nodes contain them exactly (csrc/rl_grid.h), and statement N2 is monotone
 *        under nesting because every operation rounds monotonically -- hence a node whose N2 distance exceeds the best D found so far cannot hold a winner, and
 *        no widening factor is needed.  (Without N3 a tight leaf box can drop the true nearest triangle: its E may round below its own box's B.)
 *   N4. Result.  A point takes part when every pos component is finite and maxDist >= 0 (+inf is allowed; NaN and negative values are not; -0.0 is 0).
 *        R2 = maxDist * maxDist.  Triangle k is a candidate when D_k <= R2.  CLOSEST returns the candidate with the least (D, k) in lexicographic order -- ties go
 *        to the lower export index, whatever the tree -- and writes {D, k, b1, b2} of that triangle.  WITHIN returns 1 exactly when a candidate exists.  A point
 *        that does not take part, or has no candidate, misses.
 *   N5. Independence.  The result does not depend on the tree walked, the order of the walk, how the call is cut into waves, or whether the trees were built
 *        fresh or refitted by RaylibAMD_SceneMoveTriangles.  After a move the query sees the moved triangles, as every other call on the scene does; the host
 *        oracle refreshes the host's stale copies first.
 * Refusals (0, nothing written): a null pointer with n > 0; n < 0; an unknown kind; a scene that is not finalized; a scene that holds spheres or cubes (out
 * of scope here, and refused rather than silently ignored); a BVH deeper than 64 levels; no device (the device and plain entries); on the device entry a pointer
 * off rank 0's device, points not 16-byte aligned, out not 16-byte aligned for CLOSEST or not 4-byte aligned for WITHIN.  n == 0 returns 1.
 * Checked against a loop over every triangle: tests/test_nearest_host.py, tests/test_gpu_nearest.py. */
typedef struct RaylibAMDNearestQuery { float pos[3]; float maxDist; } RaylibAMDNearestQuery;        /* 16 bytes, one 16-byte load */
typedef struct RaylibAMDNearestHit   { float dist2; int32_t prim; float b1, b2; } RaylibAMDNearestHit; /* 16 bytes; a miss: dist2 = b1 = b2 = 0, prim = -1 */
#define RAYLIB_AMD_NEAREST_WITHIN  0   /* out: uint32_t per point, 1 when a triangle lies within maxDist (may stop at the first one) */
#define RAYLIB_AMD_NEAREST_CLOSEST 1   /* out: RaylibAMDNearestHit per point */
/* n points from host memory, results to host memory; synchronous, on the device.  The library keeps its device staging buffers and grows them.
 * RaylibAMD_GetLastStats then reports rays (= points), nodesVisited, trisTested, kernelMs, wallMs and the tree walked. */
RAYLIB_API int32_t RaylibAMD_NearestPoints(SceneHandle scene, int32_t kind, const RaylibAMDNearestQuery* points, int32_t n, void* out);
/* The same on device pointers (rank 0's device).  The stream, stats and multi-rank rules are RaylibAMD_TraceRaysDevice's: stream == NULL is the library's
 * stream, synchronous, with stats; a non-null hipStream_t gets the call enqueued behind the synchronous uploads (the scene, a tree or table needed for the first
 * time) and the stats are left alone.  The call is ordered behind a move of the scene's triangles and behind multi-rank frames in flight as a ray query is. */
RAYLIB_API int32_t RaylibAMD_NearestPointsDevice(SceneHandle scene, int32_t kind, const RaylibAMDNearestQuery* points, int32_t n, void* out, void* stream);
/* The oracle: statements N1 to N4 over every triangle, no tree, no device. */
RAYLIB_API int32_t RaylibAMD_NearestPointsHost(SceneHandle scene, int32_t kind, const RaylibAMDNearestQuery* points, int32_t n, void* out);
/* Which tree and kernel instance those calls would walk under the current environment (csrc/rl_plan.cc PlanNearest): the grid-4 tree when the scene has one
 * (worst-case stack within 64), else the binary tree; RAYLIB_QUERY_TREE=2 forces the binary tree, =8 falls through to 4 (there is no 8-wide nearest walk yet).
 * `early` is 1 for WITHIN.  No device needed.  Returns 1, -1 when the BVH is deeper than 64 levels, 0 for a null argument, an unknown kind, a scene not
 * finalized or one that holds spheres or cubes. */
RAYLIB_API int32_t RaylibAMD_PlanNearest(SceneHandle scene, int32_t kind, RaylibAMDQueryPlan* out);

/* ---- the K nearest triangles and the count in range ------------------------------------------------
 * Every triangle within a point's radius, the nearest first, and how many there are: the contact step behind RaylibAMD_SceneMoveTriangles (all triangles
 * within a particle's radius), attribute transfer and smooth distance fields (a blend over the K nearest), a sphere broad phase (the count) -- in one walk of
 * the tree.  CLOSEST cannot be peeled into this: a point query has no lower bound to raise, and an exact-distance tie would be lost.  RaylibAMD_NearestPoints
 * keeps refusing kinds other than 0 and 1; these are entries of their own (csrc/rl_k_nearest_all.inl is the walk, RaylibAMD_NearestPointsAllHost the oracle).
 *   K1. Set.  For a point that takes part (N4), triangle k is in the set exactly when D_k <= R2, with D_k of N1 to N3 and R2 = maxDist * maxDist.  A point
 *        that does not take part has the empty set, and no walk is made for it.  Membership depends on the point and the triangle alone.
 *   K2. Order.  The set is sorted by (D, k) ascending, k being the index in RaylibAMD_SceneExportTriangles order -- the key CLOSEST breaks ties with.  Row i of
 *        outHits holds the first min(maxHits, |set|) triangles as {D, k, b1, b2}, with b1, b2 of N1 for that triangle, and behind them miss records
 *        {0, -1, 0, 0}.  So outHits[i * maxHits] is CLOSEST's record byte for byte, and maxHits == 1 is CLOSEST.  The order inside an exact-D tie follows the
 *        export index: RaylibAMD_SceneRebuild does not change it, unlike the multi-hit ray queries' slot order.
 *   K3. Count.  With outCount non-null, outCount[i] = |set|, however small maxHits is.  With outCount null the walk may prune with its maxHits-th key once the
 *        list is full, and visits less.  A count with maxDist = +inf visits every triangle of the scene for every point: a loop over the scene, on the device.
 *   K4. Independence.  The result does not depend on the tree walked, the order of the walk, how the call is cut into waves, or whether the trees were built
 *        fresh or refitted by RaylibAMD_SceneMoveTriangles (as N5).  After a move the host oracle refreshes the host's stale triangles first.
 *   K5. Refusals (0, nothing written): points or outHits null with n > 0; n < 0; maxHits outside 1 .. RAYLIB_AMD_MAX_NEAREST; n * maxHits above 2^31 - 1; a
 *        scene that is not finalized; a scene that holds spheres or cubes; a BVH deeper than 64 levels; no device (the plain and the device entry; the host
 *        entry needs none); on the device entry a pointer off rank 0's device, points or outHits not 16-byte aligned, outCount not 4-byte aligned.
 *        n == 0 returns 1.
 * Still out: spheres and cubes, more than RAYLIB_AMD_MAX_NEAREST records per point (the count is complete all the same), an 8-wide walk, query primitives
 * other than points.  (Signed distance is RaylibAMD_BakeDistanceField's, below.)
 * Checked against a loop over every triangle: tests/test_nearest_all_host.py, tests/test_gpu_nearest_all.py. */
#define RAYLIB_AMD_MAX_NEAREST 16
/* n points from host memory, results to host memory; synchronous, on the device.  outHits: n * maxHits RaylibAMDNearestHit, row i = point i; outCount: n
 * uint32_t, or null.  RaylibAMD_GetLastStats then reports rays (= points), nodesVisited, trisTested, kernelMs, wallMs and the tree walked. */
RAYLIB_API int32_t RaylibAMD_NearestPointsAll(SceneHandle scene, const RaylibAMDNearestQuery* points, int32_t n, int32_t maxHits, RaylibAMDNearestHit* outHits, uint32_t* outCount);
/* The same on device pointers (rank 0's device), with the stream, stats, move-ordering and multi-rank rules of RaylibAMD_NearestPointsDevice: stream == NULL
 * is the library's stream, synchronous, with stats; a non-null hipStream_t gets the call enqueued behind the synchronous uploads and the stats are left alone. */
RAYLIB_API int32_t RaylibAMD_NearestPointsAllDevice(SceneHandle scene, const RaylibAMDNearestQuery* points, int32_t n, int32_t maxHits, RaylibAMDNearestHit* outHits, uint32_t* outCount,
        void* stream);
/* The oracle: statements K1 to K3 over every triangle, no tree, no device. */
RAYLIB_API int32_t RaylibAMD_NearestPointsAllHost(SceneHandle scene, const RaylibAMDNearestQuery* points, int32_t n, int32_t maxHits, RaylibAMDNearestHit* outHits, uint32_t* outCount);
/* Which tree and kernel instance those calls would walk under the current environment (csrc/rl_plan.cc PlanNearestAll): the tree and the stack
 * RaylibAMD_PlanNearest gives CLOSEST.  wantCount (outCount non-null) selects the instance that never prunes with the list; the tree is the same.  `early` is 0.
 * No device needed.  Returns 1, -1 when the BVH is deeper than 64 levels, 0 for a null argument, maxHits outside 1 .. RAYLIB_AMD_MAX_NEAREST, a scene not
 * finalized or one that holds spheres or cubes. */
RAYLIB_API int32_t RaylibAMD_PlanNearestAll(SceneHandle scene, int32_t maxHits, int32_t wantCount, RaylibAMDQueryPlan* out);

/* ---- signed distance fields baked on the device ------------------------------------------------------
 * A regular grid of distances to the scene's triangles, with the sign of inside / outside: collision against a moved mesh, sphere tracing, offsetting, torch
 * pipelines that consume an SDF grid.  It is RaylibAMD_NearestPoints CLOSEST at every voxel centre and the parity of RaylibAMD_TraceRaysAll's crossing count
 * along one ray per ROW of voxels, put together on the device: no point, ray or result record is materialised (a 256^3 volume would take 268 MB of points,
 * as many bytes of results and 537 MB of rays), and a voxel costs 4 bytes of output (8 with outPrim).  Every output bit is fixed by the statements below; the
 * result equals the host oracle, a loop over every triangle, byte for byte (csrc/rl_k_sdf.inl holds the kernels).  Everything is float, without FMA.
 *   V1. Centres.  Per axis a and index i: t_a(i) = ((float)i + 0.5f) * spacing[a] and c_a(i) = origin[a] + t_a(i).  (float)i rounds to nearest; t_a and c_a do
 *        not decrease in i, because every operation rounds monotonically.
 *   V2. Distance.  The voxel's point is (c_x(i), c_y(j), c_z(k)), its radius maxDist (-0.0 is read as +0.0).  {D, prim} is what RAYLIB_AMD_NEAREST_CLOSEST
 *        returns for that point under N1 to N4, tie rule included.  On a hit m = sqrt(D), the correctly rounded IEEE square root (sqrt(+inf) = +inf).  On a
 *        miss -- outside the band, a point that does not take part, an empty scene -- m = maxDist.  outPrim, when given, is prim, or -1 on a miss.
 *   V3. Row rays.  For sign axis a there is one ray per pair of indices on the other two axes b < c: origin[a] on axis a and the centres c_b, c_c on the others;
 *        the direction is the unit vector of axis a; tMin = 0, tMax = FLT_MAX.  Its accepted set is M1's, exactly -- the plane t, the barycentric test, the
 *        own-box rule and the cut-out test -- so a cut-out card is open where the renderer sees through it.
 *   V4. Inside bit.  Voxel i of the row is inside along axis a exactly when the number of accepted crossings with t > t_a(i) is odd.  The ray's point at
 *        parameter t_a(i) is c_a(i) by the same expression, so a crossing exactly at a centre is not "ahead" of it.  t_a does not decrease in i, so a crossing
 *        is ahead of a prefix of the row, i < #{i : t_a(i) < t}, and toggles that prefix -- which is how the device computes the bits.
 *   V5. Value.  UNSIGNED: outDist = m.  SIGN_X, SIGN_Y, SIGN_Z: outDist = inside ? -m : m along that axis.  SIGN_MAJORITY: inside when at least two of the
 *        three axes say so.  Where m == 0 and the voxel is inside the value is -0.0f; a miss inside is -maxDist (-inf for an unbounded band).
 *   V6. Independence.  The result does not depend on the trees walked, the order of the walks, how voxels and rows are dealt to lanes and waves, or whether the
 *        trees were built fresh or refitted by RaylibAMD_SceneMoveTriangles (as N5 and M4).  After a move the bake sees the moved triangles; the host oracle
 *        refreshes the host's stale copies first.
 *   V7. Refusals (0, nothing written): a null scene, params or outDist; a dim < 1 or a voxel count above 2^31 - 1; a spacing that is not finite or <= 0; an
 *        origin that is not finite; a last centre c_a(dims[a] - 1) that is not finite; maxDist NaN or negative; an unknown sign; a scene that is not finalized;
 *        a scene that holds spheres or cubes; a BVH deeper than 64 levels; no device (the plain and the device entry; the host entry needs none); on the
 *        device entry outDist or outPrim off rank 0's device or not 4-byte aligned.
 * The sign is a property of these statements, not of the mesh's topology.  On a closed, consistently tessellated surface the parity is the inside.  An open
 * mesh, or a row ray that grazes an edge two triangles share (the reference's barycentric test is not watertight: such a ray may be accepted by both, or by
 * neither), gives whatever parity V3 and V4 give, for the whole prefix of that row.  SIGN_MAJORITY exists to outvote one such axis; it costs three sets of rows.
 * Still out: spheres and cubes; generalized winding numbers or pseudo-normal signs for open meshes; sparse or narrow-band storage (the band bounds the walk,
 * not the memory); gradients; seeding a voxel's bound from its neighbour's distance (no slack-free form of it is known).
 * Checked against a loop over every triangle: tests/test_sdf_host.py, tests/test_gpu_sdf.py. */
#define RAYLIB_AMD_SDF_UNSIGNED      0
#define RAYLIB_AMD_SDF_SIGN_X        1
#define RAYLIB_AMD_SDF_SIGN_Y        2
#define RAYLIB_AMD_SDF_SIGN_Z        3
#define RAYLIB_AMD_SDF_SIGN_MAJORITY 4
typedef struct RaylibAMDDistanceFieldParams {
    float    origin[3];    /* the lower corner of voxel (0, 0, 0) */
    float    spacing[3];   /* voxel size per axis, finite and > 0 */
    int32_t  dims[3];      /* nx, ny, nz, each >= 1; nx * ny * nz <= 2^31 - 1 */
    float    maxDist;      /* the band, as N4's maxDist: >= 0, +inf allowed, -0.0 is 0 */
    int32_t  sign;         /* RAYLIB_AMD_SDF_* */
} RaylibAMDDistanceFieldParams;
/* Host memory out: outDist, and outPrim when non-null, hold nx * ny * nz words, voxel (i, j, k) at (k * ny + j) * nx + i.  Synchronous, on the device.  The
 * library keeps its staging buffers and the bit volumes of the sign axes (ceil((n_a + 1) / 32) words per row of axis a) and grows them.
 * RaylibAMD_GetLastStats then reports rays (= voxels + row rays), nodesVisited, trisTested (both walks together), kernelMs, wallMs and the distance walk's tree. */
RAYLIB_API int32_t RaylibAMD_BakeDistanceField(SceneHandle scene, const RaylibAMDDistanceFieldParams* params, float* outDist, int32_t* outPrim);
/* The same on device pointers (rank 0's device), with the stream, stats, move-ordering and multi-rank rules of RaylibAMD_NearestPointsDevice: stream == NULL
 * is the library's stream, synchronous, with stats; a non-null hipStream_t gets the kernels enqueued behind the synchronous uploads and the stats are left
 * alone.  The bit volumes are the library's: a bake enqueued on one stream waits for the bake before it, whatever stream that one ran on. */
RAYLIB_API int32_t RaylibAMD_BakeDistanceFieldDevice(SceneHandle scene, const RaylibAMDDistanceFieldParams* params, float* outDist, int32_t* outPrim, void* stream);
/* The oracle: statements V1 to V5 over every triangle, no tree, no device. */
RAYLIB_API int32_t RaylibAMD_BakeDistanceFieldHost(SceneHandle scene, const RaylibAMDDistanceFieldParams* params, float* outDist, int32_t* outPrim);
/* Which trees and kernel instances a bake would walk under the current environment: outNearest is RaylibAMD_PlanNearest's CLOSEST plan (the distance
 * kernel: the grid-4 or the binary tree), outRows RaylibAMD_PlanRayQueryAll's (the row kernel: the 8-wide or the binary tree; filled for UNSIGNED too, which
 * traces no row).  Either may be null.  No device needed.  Returns 1, -1 when the BVH is deeper than 64 levels, 0 for what V7 refuses before it. */
RAYLIB_API int32_t RaylibAMD_PlanDistanceField(SceneHandle scene, const RaylibAMDDistanceFieldParams* params, RaylibAMDQueryPlan* outNearest, RaylibAMDQueryPlan* outRows);

/* ---- batched triangle-overlap queries -------------------------------------------------------------
 * Which triangles of the scene does a triangle intersect -- the question a collision step asks behind RaylibAMD_SceneMoveTriangles, and, with a mesh's own
 * triangles as the queries, whether the mesh intersects itself (cloth, skinned characters, lightmap charts that fold over).  The result equals a loop over
 * every triangle bit for bit, with no slack anywhere, on every tree, fresh or refitted (csrc/rl_overlap.h holds the statements for the host oracle and the
 * kernel alike; csrc/rl_k_overlap.inl is the walk).
 * Everything is float, single IEEE operations without FMA.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  cross(a, b) is the lightmap section's:
 * (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x).  The least and greatest of three values (a, b, c) are found by comparisons, in this order:
 * m = b < a ? b : a, then c < m ? c : m for the least; m = a < b ? b : a, then m < c ? c : m for the greatest.
 * For query Q = (q0, q1, q2) and scene triangle T = (v0, v1, v2), in RaylibAMD_SceneExportTriangles order:
 *   O1. Taking part.  A query takes part when all nine of its floats are finite.  One that does not gets 0 (ANY), or a row of -1 with count 0 (LIST), without a
 *        walk.
 *   O2. Own boxes.  lo and hi of each triangle are the componentwise least and greatest of its vertices (v0, v1, v2 in that order).  The boxes meet when, on
 *        every axis, loQ <= hiT && loT <= hiQ (closed).  If they do not meet, T is not accepted.
 *   O3. Shared vertices.  With RAYLIB_AMD_OVERLAP_SKIP_SHARED set, T is not accepted when one of its vertices equals one of Q's.  A vertex equals another when
 *        all three components compare ==, so -0 == +0.  This is the self-intersection rule: a mesh's own triangle, passed as a query, reports neither itself
 *        nor its neighbours across an edge or a vertex.
 *   O4. Separating axes.  Edges: eQ0 = q1 - q0, eQ1 = q2 - q1, eQ2 = q0 - q2, and eT0..2 likewise.  Normals: nQ = cross(eQ0, eQ1), nT = cross(eT0, eT1).
 *        The 17 axes, in this order: nQ; nT; cross(eQi, eTj) with i outer and j inner; cross(nQ, eQi); cross(nT, eTj).
 *        For an axis a, Q projects to {+0, dot(a, q1 - q0), dot(a, q2 - q0)} and T projects to {dot(a, v0 - q0), dot(a, v1 - q0), dot(a, v2 - q0)}; least and
 *        greatest of each triple as above.  The axis separates when maxQ < minT || maxT < minQ.  T is accepted when no axis separates.
 *        Touching counts as meeting.  Coplanar pairs are decided by the last six axes.  A NaN projection, from a degenerate triangle or an overflow, compares
 *        false and separates nothing.  The verdict is a property of (Q, T) alone; it is not promised to be symmetric in Q and T at rounding level (every
 *        projection is taken relative to q0).
 *   O5. Result.  ANY: 1 exactly when some T is accepted.  LIST: the accepted triangles' export indices ascending, the first min(maxHits, count) of them, with
 *        -1 behind them; outCount[i] is the number of all accepted triangles, however small maxHits is.
 *   O6. Independence.  The result does not depend on the tree walked, the order of the walk, how the call is cut into waves, or whether the trees were built
 *        fresh or refitted by RaylibAMD_SceneMoveTriangles.  O2 is pure comparisons, a triangle's own box lies in its leaf's box, a binary node's boxes are the
 *        min / max of its children's and a decoded grid box contains the float box it was quantised from (csrc/rl_grid.h): a node whose box does not meet Q's
 *        box under the same closed comparison holds no triangle whose own box does, so the walk needs no widening.
 * Refusals (0, nothing written): q or out null with n > 0; n < 0; an unknown kind; a flag bit other than bit 0; LIST with maxHits outside
 * 1 .. RAYLIB_AMD_MAX_OVERLAPS or n * maxHits above 2^31 - 1; ANY with a non-null outCount (maxHits is not read); a scene that is not finalized; a scene that
 * holds spheres or cubes; a BVH deeper than 64 levels; no device (the plain and the device entry; the host entry needs none); on the device entry a pointer
 * off rank 0's device, q not 16-byte aligned, out or outCount not 4-byte aligned.  n == 0 returns 1.
 * Still out: spheres and cubes; more than RAYLIB_AMD_MAX_OVERLAPS indices per query (the count is complete all the same); an 8-wide walk; query primitives
 * other than triangles and oriented boxes (RaylibAMD_OverlapBoxes, below).  The contact geometry of the listed pairs (the intersection segment) is the next section's, RaylibAMD_OverlapContacts; penetration depth
 * is not a property of a triangle pair in a soup and stays out.
 * Checked against a loop over every triangle and an edge-piercing reference in double precision: tests/test_overlap_host.py, tests/test_gpu_overlap.py. */
typedef struct RaylibAMDOverlapQuery {      /* 48 bytes, three 16-byte loads; 16-byte aligned on the device entry */
	float v0[3]; uint32_t reserved0;        /* the reserved words are not read */
	float v1[3]; uint32_t reserved1;
	float v2[3]; uint32_t reserved2;
} RaylibAMDOverlapQuery;
#define RAYLIB_AMD_OVERLAP_ANY   0          /* out: uint32_t per query, 1 when some scene triangle is accepted (may stop at the first) */
#define RAYLIB_AMD_OVERLAP_LIST  1          /* out: maxHits int32_t per query, row i = query i; outCount (may be NULL): uint32_t per query */
#define RAYLIB_AMD_OVERLAP_SKIP_SHARED 1u   /* flags bit 0, statement O3 */
#define RAYLIB_AMD_MAX_OVERLAPS 16
/* n queries from host memory, results to host memory; synchronous, on the device.  RaylibAMD_GetLastStats then reports rays (= queries), nodesVisited,
 * trisTested, kernelMs, wallMs and the tree walked. */
RAYLIB_API int32_t RaylibAMD_OverlapTriangles(SceneHandle scene, int32_t kind, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, void* out,
        uint32_t* outCount);
/* The same on device pointers (rank 0's device), with the stream, stats, move-ordering and multi-rank rules of RaylibAMD_NearestPointsDevice: stream == NULL
 * is the library's stream, synchronous, with stats; a non-null hipStream_t gets the call enqueued behind the synchronous uploads and the stats are left alone. */
RAYLIB_API int32_t RaylibAMD_OverlapTrianglesDevice(SceneHandle scene, int32_t kind, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, void* out,
        uint32_t* outCount, void* stream);
/* The oracle: statements O1 to O5 over every triangle, no tree, no device.  After a move it refreshes the host's stale triangles first. */
RAYLIB_API int32_t RaylibAMD_OverlapTrianglesHost(SceneHandle scene, int32_t kind, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, void* out,
        uint32_t* outCount);
/* Which tree and kernel instance those calls would walk under the current environment (csrc/rl_plan.cc PlanOverlap): the grid-4 tree when the scene has one and
 * its worst-case stack is within 32, else the binary tree, which the self-intersection pass walks faster than the 64-deep grid instance;
 * RAYLIB_QUERY_TREE=2 forces the binary tree, =4 the grid-4 tree up to a worst-case stack of 64, =8 falls through to 4 (there is no 8-wide overlap walk).
 * `early` is 1 for ANY.  No device needed.  Returns 1, -1 when the BVH is deeper than 64 levels, 0 for a null argument, an unknown kind, a scene not finalized or one that
 * holds spheres or cubes. */
RAYLIB_API int32_t RaylibAMD_PlanOverlap(SceneHandle scene, int32_t kind, RaylibAMDQueryPlan* out);

/* ---- contact segments of the overlapping pairs -----------------------------------------------------
 * RAYLIB_AMD_OVERLAP_LIST says that query i meets scene triangle k; this entry also says where: for every pair a LIST query reports, the segment along which
 * the two triangles cross, computed on the device in the same launch (csrc/rl_contact.h holds the statements for the host oracle and the kernel alike).
 * Everything is float, single IEEE operations without FMA; dot and cross are the section's above, a / b is the IEEE quotient.
 * For a pair (Q, T) that O1 to O4 accept under the call's flags:
 *   C1. Plane values.  nQ = cross(eQ0, eQ1) and nT = cross(eT0, eT1), as in O4.  a_k = dot(nT, q_k - v0) and b_k = dot(nQ, v_k - q0), for k = 0..2.
 *   C2. Crossing edges.  Q's edge i (q_i to q_j, j = (i + 1) mod 3) crosses T's plane when (a_i <= 0 && 0 < a_j) || (a_j <= 0 && 0 < a_i); T's edges
 *        likewise with b.  A vertex exactly on the plane counts with the non-positive side, so a sign change is counted once.  Without a NaN a triangle has
 *        0 or 2 crossing edges.  If either triangle does not have exactly 2, the pair is NO_CROSSING: coplanar pairs, a touch from the non-positive side of
 *        the plane (a touch from the positive side has two crossing edges that meet at the touching vertex, and gives a segment of one point), a degenerate
 *        triangle or an overflow that gives NaN.
 *   C3. Piercing points.  For a crossing edge: w = a_i / (a_i - a_j) and p = q_i + w * (q_j - q_i), componentwise; the difference is the edge vector of O4
 *        (eQ0 = q1 - q0, eQ1 = q2 - q1, eQ2 = q0 - q2).  The denominator cannot be 0, and 0 <= w <= 1 holds in float because the subtraction rounds
 *        monotonically.  Q gives PQ[0] and PQ[1], the lower edge index first; T gives PT[0] and PT[1] likewise.  A point's feature: 0..2 Q's edge i, 3..5 T's
 *        edge j.
 *   C4. Parameter axis.  d = cross(nQ, nT).  m = 0 if |d.x| >= |d.y| && |d.x| >= |d.z|, else 1 if |d.y| >= |d.z|, else 2 (a NaN therefore falls to 2).  A
 *        point's parameter is its m-th coordinate.
 *   C5. Clip by selection.  Each triangle's two points ordered by parameter, swapped when param(P[1]) < param(P[0]): (loQ, hiQ) and (loT, hiT).
 *        start = param(loT) > param(loQ) ? loT : loQ.  end = param(hiT) < param(hiQ) ? hiT : hiQ.  A NaN compares false and keeps Q's point.  The kind is
 *        SEGMENT when param(start) <= param(end), else GAP: both triangles straddle each other's plane and O4 accepted the pair, but at rounding level the
 *        two intervals on the common line miss; the two facing ends are still written.  No endpoint is interpolated a second time: each is one of the four
 *        piercing points, carried with its feature.
 *   C6. Record.  p0 = start, p1 = end, features = feature(p0) | feature(p1) << 8.  NO_CROSSING: points +0, features 0.  A row entry behind the count
 *        (outIndex -1): kind NONE, all 32 bytes zero.
 * Promises.  The index rows and counts are RAYLIB_AMD_OVERLAP_LIST's, byte for byte, for the same arguments.  Entry e of row i describes the pair (query i,
 * outIndex[i * maxHits + e]).  A record is a property of the ordered pair (Q, T) alone: no tree, walk order, wave cut, or refit versus rebuild shows in it (as
 * O6).  After RaylibAMD_SceneMoveTriangles the records are those of the moved triangles.  Every endpoint of a SEGMENT or GAP lies on the edge its feature
 * names, with w in [0, 1].  It is not promised that (T, Q) gives the mirrored record.
 * Refusals (0, nothing written): those of RAYLIB_AMD_OVERLAP_LIST, outIndex in the place of out; outContact null with n > 0; on the device entry outContact
 * not 16-byte aligned or off rank 0's device.  n == 0 returns 1.
 * Still out: penetration depth; contact normals beyond what nT gives the caller; a symmetric verdict for (T, Q); spheres and cubes; more than
 * RAYLIB_AMD_MAX_OVERLAPS pairs per query.
 * Checked against a NumPy restatement byte for byte and an edge-piercing reference in double precision: tests/test_contact_host.py, tests/test_gpu_contact.py. */
typedef struct RaylibAMDContact {           /* 32 bytes, written as two 16-byte stores; 16-byte aligned on the device entry */
	float p0[3]; uint32_t kind;             /* RAYLIB_AMD_CONTACT_* */
	float p1[3]; uint32_t features;         /* feature(p0) | feature(p1) << 8 */
} RaylibAMDContact;
#define RAYLIB_AMD_CONTACT_NONE        0    /* a row entry behind the count: all 32 bytes zero */
#define RAYLIB_AMD_CONTACT_SEGMENT     1
#define RAYLIB_AMD_CONTACT_GAP         2
#define RAYLIB_AMD_CONTACT_NO_CROSSING 3    /* points +0, features 0 */
/* n queries from host memory, results to host memory; synchronous, on the device; stats as RaylibAMD_OverlapTriangles.  outIndex: n * maxHits int32_t, outContact:
 * n * maxHits records, outCount (may be NULL): n uint32_t. */
RAYLIB_API int32_t RaylibAMD_OverlapContacts(SceneHandle scene, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, int32_t* outIndex,
        RaylibAMDContact* outContact, uint32_t* outCount);
/* The same on device pointers, with the stream, stats, move-ordering and multi-rank rules of RaylibAMD_OverlapTrianglesDevice. */
RAYLIB_API int32_t RaylibAMD_OverlapContactsDevice(SceneHandle scene, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, int32_t* outIndex,
        RaylibAMDContact* outContact, uint32_t* outCount, void* stream);
/* The oracle: O1 to O5 then C1 to C6 over every triangle, no tree, no device.  After a move it refreshes the host's stale triangles first. */
RAYLIB_API int32_t RaylibAMD_OverlapContactsHost(SceneHandle scene, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, int32_t* outIndex,
        RaylibAMDContact* outContact, uint32_t* outCount);
/* RaylibAMD_PlanOverlap's answer for RAYLIB_AMD_OVERLAP_LIST: the same tree and stack; the instance walked is the contacts one (k_overlap_contacts). */
RAYLIB_API int32_t RaylibAMD_PlanOverlapContacts(SceneHandle scene, RaylibAMDQueryPlan* out);

/* ---- oriented-box range queries: any, list and mark -----------------------------------------------
 * Which triangles of the scene lie in this box -- region selection and streaming, conservative surface voxelisation (one box per voxel, ANY), trigger
 * volumes, culling against a portal or a cell, and the broad phase in front of anything that is not a triangle, a point or a sphere.  The first of the query
 * primitives other than triangles that the overlap section left out.  The result equals a loop over every triangle bit for bit, with no slack anywhere, on
 * every tree, fresh or refitted (csrc/rl_box.h holds the statements for the host oracle and the kernel alike; csrc/rl_k_overlap_box.inl is the walk).
 * Everything is float, single IEEE operations without FMA.  dot, cross, and the least and greatest of three values are the overlap section's (O).
 * For query box Q and scene triangle T = (v0, v1, v2), in RaylibAMD_SceneExportTriangles order:
 *   B1. Taking part.  A query takes part when all 15 of its floats are finite and every half >= 0 (-0.0 is 0).  The axes are used as given, neither normalised
 *        nor checked for orthogonality; identity axes make the box axis-aligned, and then every frame coordinate of B3 is exactly v - center.  A query that
 *        does not take part gets 0 (ANY), a row of -1 with count 0 (LIST), and sets no bit (MARK), without a walk.
 *   B2. Enclosing box.  e.x = (|axis0.dir.x| * half0 + |axis1.dir.x| * half1) + |axis2.dir.x| * half2, and e.y, e.z likewise.  loQ = center - e,
 *        hiQ = center + e.  Infinite values are fine; no NaN can arise.  T's own box is O2's.  T is not accepted unless the two boxes meet under O2's closed
 *        comparison.  In exact arithmetic, with orthonormal axes, this removes nothing the next statements accept; at rounding level it may.  This is W5's
 *        trade: the verdict is defined so that the tree cull is exact without a slack factor.
 *   B3. Box frame.  d_k = v_k - center; p_k = (dot(axis0.dir, d_k), dot(axis1.dir, d_k), dot(axis2.dir, d_k)); h = (half0, half1, half2).
 *   B4. Thirteen axes, in this order.
 *        The three faces.  For i = 0..2, with the least and greatest of (p0[i], p1[i], p2[i]): the face separates when least > h[i] || greatest < -h[i].
 *        The triangle's plane.  e0 = p1 - p0, e1 = p2 - p1, e2 = p0 - p2.  n = cross(e0, e1).  r = (h[0]*|n.x| + h[1]*|n.y|) + h[2]*|n.z| and
 *        s = dot(n, p0).  The plane separates when s > r || s < -r.
 *        The nine edge axes, i outer (box axis) and j inner (edge).  (u, w) is (1, 2), (2, 0), (0, 1) for i = 0, 1, 2.
 *        proj(p) = p[w]*e_j[u] - p[u]*e_j[w], taken for p0, p1, p2.  r = h[u]*|e_j[w]| + h[w]*|e_j[u]|.  The axis separates when
 *        least > r || greatest < -r.
 *        T is accepted when no axis separates.  Touching counts as meeting.  A NaN (overflow) compares false and separates nothing, as in O4.  A zero half
 *        extent is a rectangle, a segment or a point, and needs no special case.
 *   B5. Result.  ANY: 1 exactly when some T is accepted.  LIST: RAYLIB_AMD_OVERLAP_LIST's contract -- the accepted triangles' export indices ascending, the
 *        first min(maxHits, count) of them, with -1 behind them; outCount[i] is complete however small maxHits is.  MARK: one mask for the whole call,
 *        (numTriangles + 31) / 32 words; bit k % 32 of word k / 32 is set exactly when some query accepts triangle k.  The call writes the whole mask: it
 *        clears it first, on the call's stream, then ORs into it; bits at and above numTriangles are 0; n == 0 leaves it all zero.  An OR has no order, so the
 *        mask is the same however the call is cut.
 *   B6. Independence.  O6's paragraph, with loQ / hiQ of B2 as the box that drives the walk: a node whose box does not meet B2's box holds no triangle whose
 *        own box does.  The result is the same on the binary and the grid-4 tree, fresh or refitted, for every cut into waves.
 * Refusals (0, nothing written -- for MARK that includes the clear): q or out null with n > 0; n < 0; an unknown kind; LIST with maxHits outside
 * 1 .. RAYLIB_AMD_MAX_OVERLAPS or n * maxHits above 2^31 - 1; ANY or MARK with a non-null outCount (maxHits is not read); a scene that is not finalized; a
 * scene that holds spheres or cubes; a BVH deeper than 64 levels; no device (the plain and the device entry; the host entry needs none); on the device entry a
 * pointer off rank 0's device, q not 16-byte aligned, out or outCount not 4-byte aligned.  n == 0 returns 1.
 * Still out: spheres and cubes as targets; more than RAYLIB_AMD_MAX_OVERLAPS indices per query (MARK is the uncapped form); the 8-wide tree; capsules and
 * frusta as query volumes; per-query masks; clipping the accepted triangles to the box.
 * Checked against a NumPy restatement byte for byte and a 13-axis test in double precision: tests/test_box_host.py, tests/test_gpu_boxes.py. */
typedef struct RaylibAMDBoxQuery {                   /* 64 bytes, four 16-byte loads; 16-byte aligned on the device entry */
	float center[3]; uint32_t reserved;              /* reserved is not read */
	struct { float dir[3]; float half; } axis[3];    /* the box's three axes, each with its half extent */
} RaylibAMDBoxQuery;
#define RAYLIB_AMD_BOX_ANY  0   /* out: uint32_t per query, 1 when some scene triangle is accepted (may stop at the first) */
#define RAYLIB_AMD_BOX_LIST 1   /* out: maxHits int32_t per query (1 .. RAYLIB_AMD_MAX_OVERLAPS), outCount (may be NULL): uint32_t per query */
#define RAYLIB_AMD_BOX_MARK 2   /* out: (numTriangles + 31) / 32 uint32_t for the whole call: bit k % 32 of word k / 32 is set when some query accepts triangle k */
/* n queries from host memory, results to host memory; synchronous, on the device; stats as RaylibAMD_OverlapTriangles. */
RAYLIB_API int32_t RaylibAMD_OverlapBoxes(SceneHandle scene, int32_t kind, const RaylibAMDBoxQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount);
/* The same on device pointers, with the stream, stats, move-ordering and multi-rank rules of RaylibAMD_OverlapTrianglesDevice. */
RAYLIB_API int32_t RaylibAMD_OverlapBoxesDevice(SceneHandle scene, int32_t kind, const RaylibAMDBoxQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount,
        void* stream);
/* The oracle: statements B1 to B5 over every triangle, no tree, no device.  After a move it refreshes the host's stale triangles first. */
RAYLIB_API int32_t RaylibAMD_OverlapBoxesHost(SceneHandle scene, int32_t kind, const RaylibAMDBoxQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount);
/* RaylibAMD_PlanOverlap's answer (csrc/rl_plan.cc PlanOverlapBoxes): the same trees, the same stacks, the same RAYLIB_QUERY_TREE knob.  `early` is 1 for ANY
 * only.  Returns as RaylibAMD_PlanOverlap; an unknown kind is 0. */
RAYLIB_API int32_t RaylibAMD_PlanOverlapBoxes(SceneHandle scene, int32_t kind, RaylibAMDQueryPlan* out);

/* ---- swept-sphere queries: the first time of impact ------------------------------------------------
 * The continuous member of the collision family: a sphere of radius r moves from origin to origin + delta, and the call says when, where and on which
 * triangle it first touches the scene -- the "sphere cast" or "sweep test" of physics and navigation layers, for particles, probes and character spheres that
 * move farther in a step than their radius.  The result equals a loop over every triangle bit for bit, with no slack factor anywhere, on every tree, fresh or
 * refitted (csrc/rl_sweep.h holds the statements for the host oracle and the kernel alike, with every operation spelled out; csrc/rl_k_sweep.inl is the walk).
 * Everything is float, without FMA; a / b, 1.0f / x and sqrt are the IEEE values; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  c(t) = origin + t * delta.
 *   W1. Who takes part.  origin, delta and radius are finite and radius >= 0 (-0.0 is 0).  The reciprocal of each delta component is taken once; a component
 *        whose reciprocal is not finite (0, or a denormal below 2^-128) is read as 0 everywhere.  Every other query misses.
 *   W2. The time bound of a box, Bt(lo, hi): the entry time of c's path into the box grown by radius, by slabs -- per axis with delta != 0 near / far =
 *        ((lo - r) - o) * inv and ((hi + r) - o) * inv, the pair picked by delta's sign; an axis with delta == 0 passes when (lo - r) <= o && o <= (hi + r).
 *        entry = max(0, nears), exit = min(fars), Bt = every such axis passes && entry <= exit ? entry : +inf.  Every operation rounds monotonically, so a
 *        box that contains another has Bt no larger, and an outer miss implies an inner miss: the walk culls by time with no widening factor.
 *   W3. Touching at the start.  With D of N1 to N3 (the nearest-point statements above) at p = origin: when D <= r * r, t = 0, feature 7, and point is N1's q.
 *   W4. The first impact otherwise: the least t in [0, 1] over seven features in a fixed order, the lower feature number winning ties.  The face: with
 *        n = cross(ab, ac), len = sqrt(dot(n, n)), s = dot(n, o - v0), a candidate when |s| > r * len and the centre approaches the plane, at
 *        t = (|s| - r * len) / |dot(n, delta)|; the point is c(t) moved r along the unit normal towards the plane, accepted when it passes the three edge
 *        functions.  The edges: the ray against the infinite cylinder of radius r about the edge, the smaller root (-b - sqrt(disc)) / a when a > 0 && disc >= 0,
 *        accepted when the axial parameter lies in [0, 1]; the point is that point of the edge.  The vertices: the ray against the sphere of radius r, the same
 *        root; the point is the vertex.  (disc is formed from the closest-approach vector, where the difference does not cancel: csrc/rl_sweep.h.)  A NaN
 *        anywhere (a degenerate triangle) fails its comparison and drops that feature only.  delta == 0 leaves W3 alone.
 *   W5. The triangle's time.  T = t >= Bt(own box) ? t : Bt(own box), the own box as in N2.  Triangle k is a candidate when T <= 1.  In exact arithmetic
 *        t >= Bt always holds; the rule moves T at rounding level only and buys that a node with Bt > the best T holds no winner.
 *   W6. Result.  CLOSEST returns the candidate with the least (T, k) -- ties go to the lower export index -- and writes {T, k, feature, point}.  ANY returns 1
 *        exactly when a candidate exists.  feature: 0 the face; 1, 2, 3 the edges v0v1, v1v2, v2v0; 4, 5, 6 the vertices v0, v1, v2; 7 the sphere touches at
 *        the start.  point is the point of the triangle that is touched; the contact normal is (origin + T * delta - point) / radius, the caller's division.
 *   W7. Independence.  The result does not depend on the tree walked, the order of the walk, how the call is cut into waves, or whether the trees were built
 *        fresh or refitted by RaylibAMD_SceneMoveTriangles.  After a move the query sees the moved triangles; the host oracle refreshes the host's stale copies first.
 * radius == 0 is accepted: a segment test whose edge and vertex features are degenerate.  It carries no watertightness promise; RaylibAMD_TraceRays is the
 * entry for rays.  A zero move answers as RAYLIB_AMD_NEAREST_WITHIN with maxDist = radius does, up to W5 at rounding level.
 * Refusals (0, nothing written): those of RaylibAMD_NearestPoints, word for word -- a null pointer with n > 0; n < 0; an unknown kind; a scene that is not
 * finalized; a scene that holds spheres or cubes; a BVH deeper than 64 levels; no device (the device and plain entries); on the device entry a pointer off
 * rank 0's device, queries not 16-byte aligned, out not 16-byte aligned for CLOSEST or not 4-byte aligned for ANY.  n == 0 returns 1.
 * Out of scope: capsules and swept triangles; spheres and cubes as targets; moving targets (a sweep against a scene mid-move is the caller's change of frame);
 * every impact along the move; slide or depenetration response; the 8-wide tree; spreading a batch over devices.
 * Checked against a loop over every triangle and a float64 geometry check: tests/test_sweep_host.py, tests/test_gpu_sweep.py. */
typedef struct RaylibAMDSweepQuery { float origin[3]; float radius; float delta[3]; uint32_t reserved; } RaylibAMDSweepQuery; /* 32 bytes, two 16-byte loads; reserved is not read */
typedef struct RaylibAMDSweepHit   { float t; int32_t prim; int32_t feature; uint32_t reserved0; float point[3]; uint32_t reserved1; } RaylibAMDSweepHit; /* 32 bytes; a miss: prim = -1, every other word 0 */
#define RAYLIB_AMD_SWEEP_ANY     0   /* out: uint32_t per query, 1 when the move touches a triangle (may stop at the first) */
#define RAYLIB_AMD_SWEEP_CLOSEST 1   /* out: RaylibAMDSweepHit per query: the first impact */
/* n queries from host memory, results to host memory; synchronous, on the device.  RaylibAMD_GetLastStats then reports rays (= queries), nodesVisited,
 * trisTested, kernelMs, wallMs and the tree walked. */
RAYLIB_API int32_t RaylibAMD_SweepSpheres(SceneHandle scene, int32_t kind, const RaylibAMDSweepQuery* q, int32_t n, void* out);
/* The same on device pointers (rank 0's device), with the stream, stats, move-ordering and multi-rank rules of RaylibAMD_NearestPointsDevice: stream == NULL
 * is the library's stream, synchronous, with stats; a non-null hipStream_t gets the call enqueued behind the synchronous uploads and the stats are left alone. */
RAYLIB_API int32_t RaylibAMD_SweepSpheresDevice(SceneHandle scene, int32_t kind, const RaylibAMDSweepQuery* q, int32_t n, void* out, void* stream);
/* The oracle: statements W1 to W6 over every triangle, no tree, no device. */
RAYLIB_API int32_t RaylibAMD_SweepSpheresHost(SceneHandle scene, int32_t kind, const RaylibAMDSweepQuery* q, int32_t n, void* out);
/* Which tree and kernel instance those calls would walk under the current environment (csrc/rl_plan.cc PlanSweep): RaylibAMD_PlanNearest's trees and stacks
 * under the same RAYLIB_QUERY_TREE, with RaylibAMD_PlanOverlap's default -- the grid-4 tree while its worst-case stack fits the 32-deep instance, else the
 * binary tree (measured: profiles/sweep_time.log).  `early` is 1 for ANY.  No device needed.  Returns 1, -1 when the BVH is deeper than 64 levels, 0 for a null argument, an
 * unknown kind, a scene not finalized or one that holds spheres or cubes. */
RAYLIB_API int32_t RaylibAMD_PlanSweep(SceneHandle scene, int32_t kind, RaylibAMDQueryPlan* out);

/* ---- path-traced radiance along caller rays -----------------------------------------------------
 * outRGBA[i] = (the mean over the samples of TraceScene(rays[i], depth 0, maxPathLength, rayTMin), 1): the reference's path tracer (render/renderer.cc:114-208)
 * with the scene's sun and sky panorama as a render sees them, on rays that need not come from a camera.  The ray is used as given: neither normalised nor
 * jittered (the caller owns the jitter).  The RGB is the float sum of the samples in sample order, from +0, times 1.0f / sampleCount -- the renderer's
 * accumulation.
 * The stream contract for caller rays (include/raylib_amd_rng.h): sample s of ray i draws from the stream (RaylibAMD_GetSeed() at the call, rays[i].stream,
 * s) with its first skipDraws draws discarded; rays[i].stream stands where the contract has the pixel index.  Rays that share a stream value share their
 * random numbers.  Hence: the rays a camera generates (RaylibAMD_EvalCameraRays), with stream = y * W + x, sampleFirst = s and skipDraws = 3 for s = 0 (2 lens
 * draws, 1 shutter-time draw) or 5 for s >= 1 (2 jitter draws before them), give bit for bit the samples Raylib_Render accumulates for that pixel
 * (tests/test_gpu_radiance.py).
 * rayTMin is used as the render uses it: not raised, and a hit's own-box rule is not widened (the ray queries above differ in both).
 * time: the shutter time of the ray, at which moving cubes are placed; every bounce of the path inherits it, as in the render. */
typedef struct RaylibAMDPathRay {      /* 32 bytes; on the device entry an array of them must be 16-byte aligned (a ray is read as two 16-byte loads) */
	float org[3]; float time;
	float dir[3]; uint32_t stream;
} RaylibAMDPathRay;
typedef struct RaylibAMDRadianceParams {
	int32_t  maxPathLength;            /* as RendererSettings.maxPathLength; 0: every result is (0, 0, 0, 1); at most 32768 */
	float    rayTMin;                  /* as RendererSettings.rayTMin; finite and >= 0 */
	uint32_t sampleFirst, sampleCount; /* ray i is traced sampleCount (>= 1) times: sample k on the stream (seed, rays[i].stream, sampleFirst + k) */
	uint32_t skipDraws;                /* draws discarded from each stream before the first bounce (<= 64) */
	float    timeMin, timeMax;         /* device entry only: the interval every ray's time lies in (a time outside it, or NaN, is clamped into it); the host entry
	                                      scans the times itself and ignores these */
} RaylibAMDRadianceParams;
/* n rays from host memory, n x 4 floats to host memory; synchronous.  Moving cubes' boxes are rebuilt when the rays' times leave the interval they were built
 * for (as RaylibAMD_TraceRays does for rayTime).  The library keeps its device staging buffers and grows them.  Returns 1 (n == 0 included), or 0 with
 * nothing written when a pointer is null with n > 0, n < 0, the scene is not finalized, maxPathLength < 0 or > 32768, sampleCount == 0, skipDraws > 64, rayTMin is
 * negative or not finite, a ray's time is not finite, the scene's BVH is deeper than 64 levels, or there is no device.
 * RaylibAMD_GetLastStats then reports rays, nodesVisited, trisTested, shadedHits, texFetches, kernelMs, wallMs, treeWidth, nodeBytes and
 * cameraSamples = n x sampleCount. */
RAYLIB_API int32_t RaylibAMD_TraceRadiance(SceneHandle scene, const RaylibAMDRadianceParams* params, const RaylibAMDPathRay* rays, int32_t n, float* outRGBA);
/* The same on device pointers (rank 0's device; both 16-byte aligned; refused otherwise).  Also refused: timeMin > timeMax or a bound that is not finite.
 * stream == NULL: the library's stream, synchronous, with stats.  A non-null hipStream_t: uploads (the scene, a tree, the sky) happen first and synchronously,
 * then the call is enqueued on that stream and returns; the stats are left alone.
 * Scratch memory (the ray counter and the path stack: maxPathLength records of 32 bytes per resident lane of the grid, kept and grown) is one per
 * library, guarded by an event chain: every launch records an event behind itself and waits, on its own stream, for the event of the launch before it, so two
 * calls enqueued on two streams run one after the other on the device and never share the scratch.  Growing the path stack waits for the device.
 * The path stack is held to 256 MiB: where the full grid's would be larger (maxPathLength above about 32 on a full device) the call runs on a smaller grid,
 * with the same results. */
RAYLIB_API int32_t RaylibAMD_TraceRadianceDevice(SceneHandle scene, const RaylibAMDRadianceParams* params, const RaylibAMDPathRay* rays, int32_t n, float* outRGBA,
        void* stream);
/* Which tree and kernel instance those calls would walk under the current environment (csrc/rl_plan.cc PlanRadiance): the grid-4 tree when the scene has one
 * (triangles only, worst-case stack within 64), else the binary tree; RAYLIB_QUERY_TREE=2 forces the binary tree, =8 falls through to 4 (the 8-wide walk is not
 * fused with shading).  No device needed.  Returns 1, -1 when the BVH is deeper than 64 levels, 0 for a null argument, a scene not finalized or params the
 * calls above would refuse.  `early` is 0. */
RAYLIB_API int32_t RaylibAMD_PlanRadiance(SceneHandle scene, const RaylibAMDRadianceParams* params, RaylibAMDQueryPlan* out);

/* ---- irradiance and SH probes gathered at caller points ---------------------------------------------
 * What a lightmap or probe baker does with RaylibAMD_TraceRadiance -- radiance integrated over a hemisphere or a sphere of directions at every point -- with the
 * directions drawn on the device, n x sampleCount paths dealt to the lanes as (point, sample) pairs (1 point x 65536 samples fills the device as 65536 points
 * x 1 sample do), and the mean and the projection taken there: no ray record is materialised and none of the sampling is restated on the host.
 * Everything is float, without FMA.  Sample s of point i draws from the stream (RaylibAMD_GetSeed() at the call, points[i].stream, sampleFirst + s) after
 * skipDraws draws have been discarded:
 *   1. Direction.  w = RandomInUnitSphere(stream): two draws u1, u2; z = 1 - 2 u1, r = sqrt(max(0, 1 - z z)), phi = 2 * 3.141592f * u2, w = (r cos phi, r sin phi, z).
 *        IRRADIANCE: if ((double)dot(w, N) < 0.0) w = -w; Wi = normalize(w) -- the Lambertian material's three statements (RaylibAMD_EvalScatter is its oracle).
 *        SH9:        Wi = normalize(w); the normal is ignored.
 *      (dot(a, b) = a.x b.x + a.y b.y + a.z b.z summed left to right; normalize(w) = w * (1.0f / sqrt(dot(w, w))).)
 *   2. Radiance.  L = TraceScene(ray(pos, Wi, time), depth 0, maxPathLength, rayTMin), the bounces taking the stream's next draws: bit for bit the sample
 *      RaylibAMD_TraceRadiance returns for the ray (pos, Wi, time, stream) with skipDraws + 2, sampleFirst + s and sampleCount 1.
 *   3. Sample value.  IRRADIANCE: v = L * fmaxf(0.0f, dot(N, Wi)).  SH9: v_j = L * Y_j, with x, y, z = Wi and
 *        Y0 = 0.282095f              Y1 = 0.488603f*y            Y2 = 0.488603f*z                          Y3 = 0.488603f*x         Y4 = 1.092548f*(x*y)
 *        Y5 = 1.092548f*(y*z)        Y6 = 0.315392f*(3.0f*(z*z) - 1.0f)                                    Y7 = 1.092548f*(x*z)     Y8 = 0.546274f*(x*x - y*y)
 *   4. Result.  The sum of the values in sample order, from +0; times 1.0f / (float)sampleCount; times the solid angle of the directions' domain: 6.2831855f
 *      (bits 0x40C90FDB) for IRRADIANCE, 12.566371f (bits 0x41490FDB) for SH9.  The directions are uniform on the hemisphere about N or on the sphere, so
 *      IRRADIANCE is the irradiance estimate and SH9 holds the radiance's coefficients in the real orthonormal basis above.
 * The result does not depend on how the call is cut into launches (below). */
typedef struct RaylibAMDGatherPoint {   /* 32 bytes; on the device entry an array of them must be 16-byte aligned */
	float pos[3];    float time;        /* as RaylibAMDPathRay.org / .time */
	float normal[3]; uint32_t stream;   /* the normal is used as given, not normalised; stream stands where the contract has the pixel index */
} RaylibAMDGatherPoint;
#define RAYLIB_AMD_GATHER_IRRADIANCE 0  /* out: 4 floats per point (E.r, E.g, E.b, 1) */
#define RAYLIB_AMD_GATHER_SH9        1  /* out: 27 floats per point, out[27*i + 3*j + c], j = 0..8, c = r,g,b */
typedef struct RaylibAMDGatherParams {
	int32_t  kind;                                     /* RAYLIB_AMD_GATHER_* */
	int32_t  maxPathLength; float rayTMin;             /* as RaylibAMDRadianceParams; maxPathLength 0: zeros (and alpha 1 for IRRADIANCE) */
	uint32_t sampleFirst, sampleCount, skipDraws;      /* skipDraws <= 62 (the direction's two draws follow them) */
	float    timeMin, timeMax;                         /* device entry only, as for radiance */
} RaylibAMDGatherParams;
/* n points from host memory, n x 4 or n x 27 floats to host memory; synchronous.  Returns 1 (n == 0 included), or 0 with nothing written for what
 * RaylibAMD_TraceRadiance refuses (a point's time standing for a ray's), an unknown kind or skipDraws > 62; n == 0 is a success without a device too.  The tree and the kernel instance are those of
 * RaylibAMD_PlanRadiance, which answers for a gather too.  RaylibAMD_GetLastStats reports what a radiance call reports, with cameraSamples = n x sampleCount,
 * traceLaunches = the trace launches made, traceKernelMs their time and kernelMs the whole call's -- the resolves, the per-launch clearing of the ray counter
 * and the gaps between the kernels included (calls of more than 4096 launches: both the whole call's). */
RAYLIB_API int32_t RaylibAMD_Gather(SceneHandle scene, const RaylibAMDGatherParams* params, const RaylibAMDGatherPoint* points, int32_t n, float* out);
/* The same on device pointers and a stream, under the rules of RaylibAMD_TraceRadianceDevice: points 16-byte aligned; out 16-byte aligned for IRRADIANCE, 4-byte
 * for SH9.  Scratch: the radiance calls' counter and path stack, under the same event chain -- gather and radiance calls run one after the other on the
 * device -- and a sample buffer (16 bytes per (point, sample) pair of a launch for IRRADIANCE, 32 for SH9) held to 256 MiB, with 3 or 27 floats of running sums
 * per point of a launch.  A call with more pairs than the buffer holds runs as several launches over sample ranges, and over point ranges as well when one
 * sample of every point does not fit; the sums carry from launch to launch, so the order of the sum is kept.  RAYLIB_GATHER_BATCH=<slots> (read at every
 * call) sets the pairs per launch instead. */
RAYLIB_API int32_t RaylibAMD_GatherDevice(SceneHandle scene, const RaylibAMDGatherParams* params, const RaylibAMDGatherPoint* points, int32_t n, float* out,
        void* stream);
/* Host only, no device: the direction Wi of sample `sample` of every point (statement 1 with the stream (seed, points[i].stream, sampleFirst + sample) and
 * the host's sqrtf, sinf, cosf and 1.0f / x), n x 3 floats.  Returns 1, or 0 with nothing written for a null argument with n > 0, n < 0, an unknown kind or
 * skipDraws > 62. */
RAYLIB_API int32_t RaylibAMD_GatherDirectionsHost(const RaylibAMDGatherParams* params, const RaylibAMDGatherPoint* points, int32_t n, uint64_t seed, uint32_t sample,
        float* outDirs);

/* Host only, no device: how a call of n points under `params` would be cut into launches under the current environment (csrc/rl_plan.cc PlanGatherCut: the
 * 256 MiB of sample buffer, or RAYLIB_GATHER_BATCH), and which points and samples launch `launchIndex` of it takes.  Launch k is sample range k % sampleRanges of
 * point range k / sampleRanges.  sampleCount may be any uint32_t: the counts are 64-bit.  Returns 1; 0 with nothing written for a null argument, n <= 0,
 * sampleCount == 0, an unknown kind or launchIndex >= launches. */
typedef struct RaylibAMDGatherCut {
	uint32_t pointsPerLaunch, samplesPerLaunch;        /* of a full launch; their product is at most the slots a launch holds */
	uint64_t pointRanges, sampleRanges, launches;      /* launches = pointRanges x sampleRanges */
	uint32_t pointFirst, numPoints;                    /* launch launchIndex: its points ... */
	uint32_t sampleBase, numSamples;                   /* ... and its samples sampleBase .. sampleBase + numSamples - 1 of the call's sampleCount */
	int32_t  first, last;                              /* it is the first / last sample range of its point range: the sums start from +0 / the result is written */
} RaylibAMDGatherCut;
RAYLIB_API int32_t RaylibAMD_PlanGatherCut(const RaylibAMDGatherParams* params, int32_t n, uint64_t launchIndex, RaylibAMDGatherCut* out);

/* ---- adaptive gather: points stop sampling once their estimate has converged --------------------------
 * RaylibAMD_Gather in passes of samples, with the stopping rule of progressive rendering (RaylibAMD_BeginProgressive) per point.  params.sampleCount is the cap:
 * no point takes more samples.  The estimator is statements 1 to 4 above, unchanged: the live points of a pass are compacted into a contiguous array and traced
 * by the gather's own kernel -- a point's random numbers hang on its `stream` field, not on its place in memory.
 *   A1. Passes.  P = ceil(cap / passSamples).  Pass p = 1 .. P gives every live point the samples sampleFirst + (p - 1) * passSamples .. up to n_p = min(cap,
 *       p * passSamples) samples in all.  All live points therefore hold the same count.  P > 4096 is refused: the host reads one count back per pass.
 *   A2. Key and moments.  The key of a sample is the three floats the sample buffer's first plane holds for it: statement 3's v = L * max(0, dot(N, Wi)) for
 *       IRRADIANCE; L itself -- not a product with Y_j -- for SH9.  lum = dot(key, (0.2126f, 0.7152f, 0.0722f)) with statement 1's left-to-right dot;
 *       y = lum / (1.0f + lum); S1 += y; S2 += y * y.  Both sums are float, run in sample order and start from +0: the progressive renderer's statement.  A key
 *       that is not finite is not replaced.
 *   A3. Decision.  After pass p a live point's error is the progressive rule's standard error of the mean (csrc/rl_progressive.h ProgressivePixelError(S1, S2,
 *       n_p): sqrt(max(0, (S2 - S1 * S1 / n) / (n - 1)) / n), +inf when a sum or the value is not finite).  The point stops when n_p == cap, or when
 *       n_p >= minSamples && error < threshold.  Stopping is final.
 *   A4. Result.  A point that stops with n samples receives, bit for bit, what RaylibAMD_Gather returns for that point with sampleCount = n and everything else
 *       equal: the sum from +0 in sample order, times 1.0f / (float)n, times the solid angle, alpha 1 for IRRADIANCE.  outSamples[i] = n (outSamples may be null).
 *   A5. Independence.  Neither out nor outSamples depends on how a pass is cut into launches (RAYLIB_GATHER_BATCH, the 256 MiB of sample buffer: point ranges and
 *       sample ranges), on the tree walked, or on which other points are in the call. */
typedef struct RaylibAMDGatherAdaptiveParams {
	float    threshold;    /* a point stops when its error (A3) is < threshold; 0: never early; finite, >= 0 */
	uint32_t minSamples;   /* samples a point takes before it may stop early; >= 2 */
	uint32_t passSamples;  /* samples per live point and pass; >= 1 */
} RaylibAMDGatherAdaptiveParams;
/* n points from host memory; n x 4 or n x 27 floats and (outSamples may be null) n counts to host memory; synchronous.  Returns 1 (n == 0 included, with or
 * without a device), or 0 with nothing written for everything RaylibAMD_Gather refuses, a null `adaptive`, a threshold that is negative or not finite,
 * minSamples < 2, passSamples == 0 or more than 4096 passes.  RaylibAMD_GetLastStats reports the gather's counters with cameraSamples = the sum of outSamples,
 * traceLaunches = the trace launches made over all passes, kernelMs the whole call's time -- resolves, compactions and the per-pass read-backs of the live count
 * included -- and traceKernelMs the trace launches' (calls of more than 4096 launches: both the whole call's). */
RAYLIB_API int32_t RaylibAMD_GatherAdaptive(SceneHandle scene, const RaylibAMDGatherParams* params, const RaylibAMDGatherAdaptiveParams* adaptive,
        const RaylibAMDGatherPoint* points, int32_t n, float* out, uint32_t* outSamples);
/* The same on device pointers and a stream, under the pointer and alignment rules of RaylibAMD_GatherDevice; outSamples (may be null) is 4-byte aligned memory of
 * rank 0's device (refused otherwise).  With a non-null hipStream_t the work runs on that stream under the radiance calls' event chain, and the stats are left
 * alone -- but the call is NOT fire-and-forget: the host must know the live count to plan the next pass, so the call waits for that stream once per pass and
 * returns when the last pass is complete, out and outSamples written.  Work the caller enqueued on the stream before the call is waited for with it.
 * Scratch beyond the gather's, kept and grown under the same event chain: 5 or 29 floats and a flag per point of the call (the sums, S1, S2), and, when there is
 * more than one pass, two index lists and two arrays of 32-byte records of the call's size, between which the live set is compacted in order behind each pass. */
RAYLIB_API int32_t RaylibAMD_GatherAdaptiveDevice(SceneHandle scene, const RaylibAMDGatherParams* params, const RaylibAMDGatherAdaptiveParams* adaptive,
        const RaylibAMDGatherPoint* points, int32_t n, float* out, uint32_t* outSamples, void* stream);
/* Host only, no device: statements A1 to A3 on keys of the caller's -- count x cap x 3 floats, point-major, in sample order -- giving the n at which each point
 * stops.  cap stands for params.sampleCount.  Built without FMA from csrc/rl_progressive.h, as RaylibAMD_ProgressiveDecideHost is: the device's oracle.
 * Returns 1, or 0 with nothing written for a null argument (keys and outSamples may be null when count == 0), count < 0, cap == 0 and the refusals of
 * `adaptive` above. */
RAYLIB_API int32_t RaylibAMD_GatherAdaptiveDecideHost(const RaylibAMDGatherAdaptiveParams* adaptive, uint32_t cap, const float* keys, int64_t count, uint32_t* outSamples);
/* Test hook: the compaction behind a pass, launched as a pass launches it.  live: numLive strictly ascending indices < numPoints; stopped: one byte per original
 * point; points: the numPoints original records (the hook hands the kernels the live ones' records, contiguous, as a pass holds them).  outLive / outPoints
 * receive the entries of live whose point has not stopped, in order, and their records -- *outCount of them, nothing behind.  Returns 1, or 0 with nothing
 * written for a null argument, numLive > numPoints, a list that is not strictly ascending below numPoints, or no device. */
RAYLIB_API int32_t RaylibAMD_GatherCompactTest(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const RaylibAMDGatherPoint* points, uint32_t numPoints,
        uint32_t* outLive, RaylibAMDGatherPoint* outPoints, uint32_t* outCount);

/* ---- lightmaps baked on the device: UV-space texels into RaylibAMD_Gather ------------------------------
 * The step in front of RaylibAMD_Gather and the two behind it: the triangles of a range are rasterised in lightmap-UV space into one gather point per covered
 * texel of a width x height atlas, the points are gathered, and the values go back into the atlas, whose gutters are filled by dilation.
 * uv: six floats per triangle of the range, (u0, v0, u1, v1, u2, v2), entry k for triangle triFirst + k; NULL: the triangles' own s0, t0 ... s2, t2.
 * Everything integer is exact, everything float is without FMA, 1.0f / x and sqrtf are the IEEE values.
 *   1. Snap.  Per vertex fx = (u * (float)width) * 256.0f, fy = (v * (float)height) * 256.0f; X = (int32_t)floorf(fx + 0.5f), Y likewise: 8 sub-texel bits, no
 *      flip, no wrap.  A triangle is skipped when any of its six values is not finite or |f| > 16777216.0f.
 *   2. Area.  A2 = (X1-X0)*(Y2-Y0) - (Y1-Y0)*(X2-X0) in int64; a triangle with A2 == 0 is skipped; s = sign(A2).
 *   3. Coverage.  Texel (x, y) has the centre P = (256x + 128, 256y + 128).  orient(Q,R,P) = (Rx-Qx)*(Py-Qy) - (Ry-Qy)*(Px-Qx) in int64;
 *      wA = s*orient(B,C,P), wB = s*orient(C,A,P), wC = s*orient(A,B,P).  The triangle covers the texel when all three are >= 0 (edges are inclusive).  A
 *      texel's owner is the lowest-indexed triangle of the range that covers it.
 *   4. Barycentrics.  b1 = (float)((double)wB / (double)|A2|), b2 = (float)((double)wC / (double)|A2|).
 *   5. Point.  e1 = v1 - v0, e2 = v2 - v0; pos = (v0 + b1*e1) + b2*e2; n = (n0 + b1*(n1-n0)) + b2*(n2-n0), d = dot(n, n) (section 3f's dot).  If d is not
 *      finite or not > 0: n = cross(e1, e2), cross(a,b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), and d its dot.  If d is still not finite or
 *      not > 0, or a component of pos is not finite, the texel is empty (it does not pass to the next triangle).  Otherwise normal = n * (1.0f / sqrtf(d)),
 *      time = params.time and stream = y*width + x.
 *   6. Order.  The points are the non-empty owned texels in ascending y*width + x.
 *   7. Gather.  The covered texels' values are, bit for bit, RaylibAMD_Gather(scene, &params.gather, thosePoints, count, ...).
 *   8. Atlas.  A covered texel receives its value and coverage 1; every other texel +0 in all C channels (C = 4 or 27) and coverage 0.
 *   9. Dilation.  Pass k = 1 .. dilate reads the atlas and the coverage as they were before the pass.  A texel of coverage 0 looks at its neighbours inside the
 *      atlas in the order (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1); m = how many of them have coverage != 0.  If m > 0 each channel becomes (their sum
 *      in that order, from +0) * (1.0f / (float)m), channel 3 of an IRRADIANCE texel becomes 1.0f, and the texel's coverage becomes 1 + k.
 * The stream is the texel's index, not the point's rank: a texel draws the same paths whatever else is in the atlas. */
typedef struct RaylibAMDLightmapParams {
	int32_t width, height;        /* the atlas, 1 .. 16384 each */
	int32_t triFirst, triCount;   /* triangles triFirst .. triFirst + triCount - 1 in RaylibAMD_SceneExportTriangles order; triCount -1: to the end */
	int32_t dilate;               /* gutter passes, 0 .. 64 */
	float   time;                 /* every point's time */
	RaylibAMDGatherParams gather; /* kind IRRADIANCE or SH9 and the rest, as for RaylibAMD_Gather; its timeMin / timeMax are ignored (both are `time`) */
} RaylibAMDLightmapParams;
/* Statements 1 to 6 alone, on the device (rank 0's): the gather points of the atlas' covered texels in ascending texel index and (outTexel may be null) each
 * one's texel index y * width + x, to host memory.  Returns the number of covered texels -- which may exceed capacity: min(count, capacity) records are
 * written; outPoints may be null when capacity is 0 --, or -1 with nothing written for: a null scene or params, a scene not finalized, width or height outside
 * 1 .. 16384, dilate outside 0 .. 64, a triangle range that is empty or not inside the scene, a time that is not finite, a negative capacity, more than 2^36 (triangle, texel-of-its-clipped-
 * bounding-box) pairs to test -- thousands of triangles whose boxes span a large atlas: bake them in ranges --, anything
 * RaylibAMD_Gather refuses of params.gather, no device or no memory.  The stats are left alone. */
RAYLIB_API int64_t RaylibAMD_LightmapPoints(SceneHandle scene, const RaylibAMDLightmapParams* params, const float* uv, RaylibAMDGatherPoint* outPoints, uint32_t* outTexel,
        int64_t capacity);
/* The same on the host, no device needed: the oracle of statements 1 to 6. */
RAYLIB_API int64_t RaylibAMD_LightmapPointsHost(SceneHandle scene, const RaylibAMDLightmapParams* params, const float* uv, RaylibAMDGatherPoint* outPoints, uint32_t* outTexel,
        int64_t capacity);
/* The whole bake, statements 1 to 9, from and to host memory; synchronous.  out: width * height * C floats, texel-major; outCoverage (may be null): one byte per
 * texel.  Returns 1 -- an atlas without a covered texel is a success: zeros, coverage 0 --, or 0 with nothing written for the refusals above (out null
 * included).  RaylibAMD_GetLastStats reports what the gather reports, with pixels = the covered texels and kernelMs the whole call's: the raster stages, the
 * gather, the scatter and the dilation. */
RAYLIB_API int32_t RaylibAMD_BakeLightmap(SceneHandle scene, const RaylibAMDLightmapParams* params, const float* uv, float* out, uint8_t* outCoverage);
/* The same with uv, out and outCoverage in memory of rank 0's device (uv and out 4-byte aligned; refused otherwise), under the rules of RaylibAMD_GatherDevice.
 * A non-null hipStream_t: the raster stages and the read-back of the count run first, on the library's stream -- ordered behind whatever that hipStream_t
 * holds at the call, so a uv still being written there is read complete --, and are waited for, as uploads are; the gather,
 * the scatter, the dilation and the copies into out and outCoverage are then enqueued on that stream and the call returns; the stats are left alone.
 * Scratch, kept and grown by the library under the radiance calls' event chain: the owner map (4 bytes per texel), the ranks (4 per texel), 40 bytes per
 * triangle of the range, the points and their values, and two atlases with their coverage for the dilation's ping-pong. */
RAYLIB_API int32_t RaylibAMD_BakeLightmapDevice(SceneHandle scene, const RaylibAMDLightmapParams* params, const float* uv, float* out, uint8_t* outCoverage, void* stream);
/* The adaptive bake: statements 1 to 9 with statement 7 replaced by RaylibAMD_GatherAdaptive's A1 to A5 on the covered texels (params.gather.sampleCount is the
 * cap).  outSamples (may be null): a width x height atlas of uint32_t holding the texel's sample count n where the coverage is 1 and 0 elsewhere; it is not
 * dilated.  Refusals: RaylibAMD_BakeLightmap's and RaylibAMD_GatherAdaptive's.  The stats are the adaptive gather's, with pixels and kernelMs as for a bake.
 * There is no filtered variant: a raw adaptive bake with dilate 0 followed by RaylibAMD_FilterLightmap is the pipeline. */
RAYLIB_API int32_t RaylibAMD_BakeLightmapAdaptive(SceneHandle scene, const RaylibAMDLightmapParams* params, const RaylibAMDGatherAdaptiveParams* adaptive, const float* uv,
        float* out, uint8_t* outCoverage, uint32_t* outSamples);
/* The same on device pointers, under the rules of RaylibAMD_BakeLightmapDevice (outSamples 4-byte aligned memory of rank 0's device).  With a non-null stream the
 * call waits for that stream once per pass, as RaylibAMD_GatherAdaptiveDevice does; the scatter, the dilation and the copies are enqueued behind the last pass. */
RAYLIB_API int32_t RaylibAMD_BakeLightmapAdaptiveDevice(SceneHandle scene, const RaylibAMDLightmapParams* params, const RaylibAMDGatherAdaptiveParams* adaptive,
        const float* uv, float* out, uint8_t* outCoverage, uint32_t* outSamples, void* stream);

/* ---- an edge-avoiding filter over the atlas' covered texels, between statements 8 and 9 ---------------
 * An a-trous filter (Dammertz et al. 2010) guided by each covered texel's gather point -- its world position and normal -- and by the values themselves: it
 * never reads a gutter, and charts that are neighbours in the atlas and apart in the world do not blend.  Everything is float, without FMA, the divisions are
 * IEEE and expf is csrc/rl_glibc_math.h's expf_ (glibc's, bit for bit).
 *   F1. Channels.  C = 4 (IRRADIANCE) or 27 (SH9).  The key channels are 0, 1, 2 in both kinds: E.rgb, or the rgb of coefficient 0.  The filtered channels are
 *       0 .. 2 for IRRADIANCE and 0 .. 26 for SH9.
 *   F2. Participants.  Only the texels of coverage 1 after statement 8 take part, as centres and as taps; every other texel stays +0 with coverage 0 until
 *       statement 9.
 *   F3. Preparation.  I_0 = the texel's value with every channel that is not finite read as 0.  The guides are the texel's gather point: P = pos, n = normal.
 *   F4. Constants, computed once on the host and handed to both paths as they are, for i = 0 .. K-1 (K = iterations):
 *         invC_i = (float)(1u << (2*i)) / (sigmaColor * sigmaColor)      invN = 1.0f / (sigmaNormal * sigmaNormal)
 *         sp = sigmaPosition * (float)(1u << i); invP_i = 1.0f / (sp * sp)
 *   F5. Iteration i, step s = 2^i.  The taps of texel p = (x, y) are q = p + s*(dx, dy), dy outer, dx inner, both -2 .. 2; a tap outside the atlas or whose
 *       coverage is not 1 is skipped.  With g(v) = c / (1.0f + c), c = v > 0 ? v : 0, and Dist2(a, b) = d0*d0 + d1*d1 + d2*d2 of the three differences a - b,
 *       summed left to right:
 *         dc = (g(I_i(q)[0]) - g(I_i(p)[0]))^2 + (... [1])^2 + (... [2])^2, as a Dist2;  dn = Dist2(n(q), n(p));  dp = Dist2(P(q), P(p))
 *         w  = (k[dx+2] * k[dy+2]) * expf(-(dc*invC_i + dn*invN + dp*invP_i)),  k = {1/16, 1/4, 3/8, 1/4, 1/16}
 *         I_{i+1}(p)[c] = (sum of w * I_i(q)[c]) / (sum of w) for every filtered channel c, both sums in tap order from +0, the same w for every channel.
 *       The centre tap always counts (its w is 9/64), so the divisor is >= 9/64.
 *   F6. Result.  I_K; channel 3 of an IRRADIANCE texel is written 1.0f.
 * The filter sees neither params.dilate nor how the gather was cut into launches. */
typedef struct RaylibAMDLightmapFilterParams {
	int32_t iterations;      /* K, 1 .. 8: steps 1, 2, 4 ... 2^(K-1) texels apart */
	float   sigmaColor;      /* tolerance of the colour distance; halves per step */
	float   sigmaNormal;     /* ... of the normal distance */
	float   sigmaPosition;   /* world-space distance tolerated between texels ONE texel apart; doubles per step */
} RaylibAMDLightmapFilterParams;   /* each sigma finite and in [1e-3, 1e3]; there are no defaults: the position's scale is the caller's */
/* RaylibAMD_BakeLightmap / RaylibAMD_BakeLightmapDevice with statement F between statements 8 and 9.  Refusals, memory rules, stream rules and stats are theirs
 * (kernelMs includes the filter); refused as well, with nothing written: a null filter, iterations outside 1 .. 8, a sigma that is not finite or outside
 * [1e-3, 1e3].  Scratch beside the bakes': a second array of the points' values (the iterations' ping-pong). */
RAYLIB_API int32_t RaylibAMD_BakeLightmapFiltered(SceneHandle scene, const RaylibAMDLightmapParams* params, const RaylibAMDLightmapFilterParams* filter, const float* uv,
        float* out, uint8_t* outCoverage);
RAYLIB_API int32_t RaylibAMD_BakeLightmapFilteredDevice(SceneHandle scene, const RaylibAMDLightmapParams* params, const RaylibAMDLightmapFilterParams* filter, const float* uv,
        float* out, uint8_t* outCoverage, void* stream);
/* An atlas the caller already has -- a raw bake made with dilate 0 and kept -- filtered again without tracing a path: statements 1 to 6 for the ownership and the
 * guides, then `in`'s value at every covered texel (whatever `in` holds elsewhere is ignored), statement F, and statement 9 with params.dilate.  in and out:
 * width * height * C floats; out may be in.  params.gather is checked as a bake checks it; only its kind is used.  Refusals as above, a null `in` included;
 * memory and stream rules as the bakes' (`in` as `out`).  The stats of the host entry: pixels = the covered texels, kernelMs the whole call's, no rays. */
RAYLIB_API int32_t RaylibAMD_FilterLightmap(SceneHandle scene, const RaylibAMDLightmapParams* params, const RaylibAMDLightmapFilterParams* filter, const float* uv,
        const float* in, float* out, uint8_t* outCoverage);
RAYLIB_API int32_t RaylibAMD_FilterLightmapDevice(SceneHandle scene, const RaylibAMDLightmapParams* params, const RaylibAMDLightmapFilterParams* filter, const float* uv,
        const float* in, float* out, uint8_t* outCoverage, void* stream);
/* Statement F alone on the host, without a device or a scene: the oracle.  It works in compacted form, on what RaylibAMD_LightmapPointsHost and RaylibAMD_Gather
 * return: points and texel (strictly ascending texel indices y * width + x) of `count` covered texels, values and outValues count x C floats; outValues may be
 * values.  Returns 1 (count == 0 included), or 0 with nothing written for a null pointer with count > 0, count < 0, an unknown kind, filter params as refused
 * above, width or height outside 1 .. 16384, a texel array that is not strictly ascending or has an entry >= width * height, or no memory. */
RAYLIB_API int32_t RaylibAMD_FilterLightmapHost(int32_t width, int32_t height, int32_t kind, const RaylibAMDLightmapFilterParams* filter, const RaylibAMDGatherPoint* points,
        const uint32_t* texel, int64_t count, const float* values, float* outValues);

/* ---- procedural scene elements ----------------------------------------------------------
 * The reference's two procedural demo scenes (src/main.cc:913-984) `new` its C++ classes (Sphere, Cube, Triangle,
 * Lambertian, Metal, ...) in the application and pass the object pointers to Raylib_AddSceneElement.  A C ABI
 * cannot accept foreign C++ objects, so the same elements are created through the library instead; the handles
 * returned here are what Raylib_AddSceneElement accepts.  Elements and materials are owned by the library and
 * BORROWED by scenes (destroy them after the scene, like OBJ models). */
typedef uintptr_t MaterialHandle;
/* type: 0 Lambertian(albedo) 1 Mirror(albedo) 2 Dielectric(ior, transmission) 3 Microfacet(albedo, roughness, metallic, emissive)
 *       4 Metal(albedo, fuzziness) 5 DiffuseLight(albedo = intensity)      (reference render/material.h:50-270) */
RAYLIB_API MaterialHandle RaylibAMD_CreateMaterial(int32_t type, const float albedo[3], float roughness, float metallic,
	const float emissive[3], float ior, const float transmission[3], float fuzziness);
RAYLIB_API int32_t RaylibAMD_DestroyMaterial(MaterialHandle material);
/* reference geom/sphere.h:11-16 */
RAYLIB_API SceneElementHandle RaylibAMD_CreateSphere(float cx, float cy, float cz, float radius, MaterialHandle material);
/* reference geom/cube.h:24-31 (Cube::FromMinMaxBounds) */
RAYLIB_API SceneElementHandle RaylibAMD_CreateCube(const float minBounds[3], const float maxBounds[3], float timeStartMove,
	const float velocity[3], MaterialHandle material);
/* reference geom/triangle.h:12-15; UVs as SetParameterization (s0 t0 s1 t1 s2 t2), may be NULL */
RAYLIB_API SceneElementHandle RaylibAMD_CreateTriangle(const float v0[3], const float v1[3], const float v2[3],
	const float n0[3], const float n1[3], const float n2[3], const float uv[6], MaterialHandle material);
RAYLIB_API int32_t RaylibAMD_DestroySceneElement(SceneElementHandle element);

/* Test hooks: one function of the hot path on an array of inputs, evaluated by the device code the megakernel uses.
 *   EvalScatter   : Material::Scatter + ScatteringPdf + Emitted for scene material `material`; record i uses the stream
 *                   (seed, i, 0).  in: 16 floats (ray o, d, time; hit t, p, n, paramU, paramV); out: 16 floats (scattered?,
 *                   reflectance, direction, origin, pdf, scatteringPdf, emitted, draws) -- layouts of oracle/ref_glue.cc.
 *   EvalCameraRays: Camera::GetCameraRay(u, v), stream (seed, i, 0); out 7 floats (o, d, time).
 *   EvalTexture   : Texture2D::Sample of scene texture `texture`; out 4 floats. */
RAYLIB_API int32_t RaylibAMD_EvalScatter(SceneHandle scene, int32_t material, const float* records, int32_t n, uint64_t seed, float* out);
RAYLIB_API int32_t RaylibAMD_EvalCameraRays(CameraHandle camera, const float* uv, int32_t n, uint64_t seed, float* out);
RAYLIB_API int32_t RaylibAMD_EvalTexture(SceneHandle scene, int32_t texture, int32_t bSRGB, const float* uv, int32_t n, float* out);
/* Test hook: out[i] = f(x[i] [, y[i]]) evaluated by the DEVICE math the megakernel uses (csrc/rl_math.h).
 * fn: 0 sinf, 1 cosf, 2 tanf, 3 acosf, 4 asinf, 5 atan2f(x,y), 6 expf, 7 logf, 8 powf(x,y), 9/10 sincos (sin / cos
 * part), 11 sqrtf, 12 x / y, 13 fmodf(x, 1) (the texture wrap), 14 1.0f / x and 15 sqrtf(x) in their short exact forms
 * (csrc/rl_math.h rcp1_ / sqrt_, range guards included).  y may be NULL for one-argument functions. */
RAYLIB_API int32_t RaylibAMD_EvalDeviceMath(int32_t fn, const float* x, const float* y, int32_t n, float* out);

/* Test hook (host only, no device needed): which 8 x 8 cells of a width x height frame can no ray of the camera -- pinhole or thin lens, no sky panorama -- meet the box
 * bounds = { min x, y, z, max x, y, z } in?  The renderer leaves those cells out of the megakernel's job list and fills them with the miss shader's
 * constant (csrc/rl_cull.cc).  outEmpty: one byte per cell, row-major, 1 = dropped; outConstant: the constant (the sun's illuminance, or nothing).
 * The sun direction is the normalised one the scene holds.  Returns the number of dropped cells, 0 when none can be dropped, -1 when the frame is not
 * eligible (a corner of the box beside or behind the camera, a sun ray from the camera -- from any point of its lens -- that may meet the box). */
RAYLIB_API int32_t RaylibAMD_CullCells(CameraHandle camera, const float* bounds, const float* sunIlluminance, const float* sunDirection,
                                       int32_t width, int32_t height, uint8_t* outEmpty, float* outConstant);

/* Test hook: the device's short exact sequences for 1.0f / x (which = 0) and sqrtf(x) (which = 1) -- csrc/rl_glibc_math.h rcp1_ / sqrtf_, used by
 * normalize and every reciprocal of the shading code -- against the compiler's IEEE expansions on ALL 2^32 float bit patterns, on the device.
 * which = 2: a / b with the divisor's correctly rounded reciprocal in hand (csrc/rl_math.h div_by_: the pixel -> [0, 1) divisions of a camera ray and the two
 * barycentric divisions of a triangle test) -- every bit pattern as numerator of a set of divisors and as divisor of a set of numerators, wherever the
 * sequence's stated conditions hold; which = 3: the triangle test's short barycentric form (csrc/rl_dev_walk.h Barycentric) against the two divisions and
 * the reference's test, every bit pattern in each of its three operands: same verdict, same quotients; which = 4: acosf and tanf with their divisions in the
 * short form (csrc/rl_glibc_math.h acosf_t / tanf_t, RL_EXACT_DIV bit 4) against the same functions with IEEE divisions, every bit pattern.
 * outMismatches: inputs whose results differ (a NaN may differ in payload); outFirstBits: the smallest such bit pattern.  Returns 1 when the sweep ran. */
RAYLIB_API int32_t RaylibAMD_VerifyExactMath(int32_t which, uint64_t* outMismatches, uint64_t* outFirstBits);
/* The lazy-reflectance instance's per-vertex guard, swept on the device over n scattering events made from edge and random inputs (csrc/rl_render_lazy.hip
 * k_verify_lazy_refl): outUnsafe = events the guard passed although a component of the reflectance or the scattering pdf is not finite (must be 0),
 * outGuardFailed = events it refused.  Returns 1 when the sweep ran. */
RAYLIB_API int32_t RaylibAMD_VerifyLazyRefl(uint32_t n, uint64_t seed, uint64_t* outEvents, uint64_t* outUnsafe, uint64_t* outGuardFailed);
/* The same instance's decision to leave an event's scattering pdf unevaluated, swept over the same n events (csrc/rl_render_lazy.hip k_verify_lazy_pdf):
 * outWrong = events decided "quick" whose pdf is not positive, whose ScatteringPdf value or recomputed half vector is not finite, or whose vertex record (of
 * either form) does not give the fold the eagerly evaluated bits of both (must be 0), outRefused = events that evaluate the pdf after all.  Returns 1 when the
 * sweep ran. */
RAYLIB_API int32_t RaylibAMD_VerifyLazyPdf(uint32_t n, uint64_t seed, uint64_t* outEvents, uint64_t* outWrong, uint64_t* outRefused);
/* The same instance's Beckmann sampler calls logf, expf, sqrtf and 1 / x without their special-case guards where its arguments cannot reach them (csrc/rl_dev_shade.h
 * "the ranged sampler").  Every such piece is a function of one float, compared here with the general form on ALL 2^32 bit patterns of it, on the device
 * (csrc/rl_render_lazy.hip k_verify_sampler_ranged).  mode 0: the Newton loop's body, ErfInv(b) and expf of minus its square; mode 1: the prologue (tanThetaI, Erf of
 * the cotangent, the fit exponent, the normalization) as a function of cosThetaI, for every cosThetaI below the sampler's .9999 branch; mode 2: that branch as a
 * float compare against the (double) compare; mode 3: csrc/rl_glibc_math.h logf_in_range_, expf_in_range_ and sqrtf_in_range_ against the general functions, each over
 * its stated domain.  outMismatches: inputs whose results differ (a NaN may differ in payload; mode 1: inside [C_MIN, .9999] only) -- must be 0; outFirstBits: the
 * smallest such bit pattern.  Mode 1 also fills outInterval[3] with bit patterns: the ends of the interval below the branch on which the two prologues agree
 * everywhere (one pattern above the largest positive cosThetaI at which they differ, and the last float below the branch) and the C_MIN the library was
 * built with, which must lie inside; and outOutside: the differing inputs outside [C_MIN, .9999], which the sampler sends through the general prologue.  Any output
 * may be NULL.  Returns 1 when the sweep ran. */
RAYLIB_API int32_t RaylibAMD_VerifySamplerRanged(int32_t mode, uint64_t* outMismatches, uint64_t* outFirstBits, uint32_t* outInterval, uint64_t* outOutside);
/* The same instance normalises its vectors and takes its single square roots without sqrtf's and 1 / x's range guards, each behind one wave vote on the length or a
 * written bound (csrc/rl_dev_core.h "normalize without the two range guards").  The claims, compared on the device (csrc/rl_render_lazy.hip k_verify_normalize_ranged).
 * mode 0: all 2^32 bit patterns x of a squared length, the guard-free chain 1 / sqrt(x) against the general one; outMismatches counts those inside the vote's domain
 * 2^-101 <= x <= FLT_MAX, outFirstOutside is the smallest pattern outside it at which the chains differ (~0: none) and outCount how many do.  mode 1: acosf without
 * its guards (csrc/rl_glibc_math.h acosf_in_range_) against acosf on every float of the ranged sampler's interval of cosThetaI.  mode 2: the voted normalisation
 * against the general one, component bits compared, on 64 + 2^24 vectors: an edge list (zero vectors, components +-0, subnormal lengths, squared lengths either
 * side of 2^-101, infinities, NaN, overflowing lengths) and generated waves of every binary scale; outCount is the number of vectors whose wave took the guard-free
 * side.  outMismatches: inputs whose results differ (a NaN may differ in payload) -- must be 0; outFirst: the smallest such bit pattern (mode 2: vector index).  Any
 * output may be NULL.  Modes outside 0 .. 2 are refused (0).  Returns 1 when the sweep ran. */
RAYLIB_API int32_t RaylibAMD_VerifyNormalizeRanged(int32_t mode, uint64_t* outMismatches, uint64_t* outFirst, uint64_t* outFirstOutside, uint64_t* outCount);

/* ---- a finalized scene's triangles moved; its trees refitted on the device ---------------------------
 * Triangles [first, first + count) in RaylibAMD_SceneExportTriangles order take new vertices -- positions: count x 9 floats (v0 v1 v2) -- and, when normals is
 * not NULL, new shading normals (count x 9 floats, n0 n1 n2; NULL keeps them).  Materials, UVs, cut-out flags, spheres and cubes are untouched, a query's
 * primitive index stays the triangle's index.  Every later call on the scene -- Raylib_Render, RaylibAMD_RenderDevice, RenderViews, RenderCellsHost, TraceRays,
 * TraceRadiance, Gather*, BakeLightmap*, LightmapPoints* -- returns what that call returns on a scene created from the moved triangles and finalized: the same
 * bits (the closest hit depends neither on how tight a box is nor on the order in which boxes that contain it are tested: DESIGN.md section 4).
 * Topology: the trees keep their shape and the triangles their slots; every box of every format the device holds (binary, 4-wide float and grid, 8-wide, leaf
 * list) is refitted, whole tree.  RaylibAMD_SceneBVHInfo's SAH cost is then that of the refitted binary tree, so a caller sees the trees degrade and may call
 * RaylibAMD_SceneRebuild.  RaylibAMD_SceneTopologyHash is unchanged by a move.  RaylibAMD_SceneBVHHash covers the node records with their boxes: a move changes it, and
 * after RaylibAMD_SceneRebuild both are the hashes of a scene created from the moved triangles.  (RaylibAMD_SceneBVH8Info's expected steps stay those of the last build.)
 * Host copies: the host entry updates the host's triangles at once; after the device entry they are stale, and after either entry so are the host's copies of
 * the trees' boxes but the root's.  One read-back brings them up to date the first time one of these needs them: RaylibAMD_SceneExportTriangles,
 * RaylibAMD_LightmapPointsHost, the lightmap calls' triangle table, RaylibAMD_SceneBVHInfo / BVH4Info / BVH8Info / BVHHash / ExportBVHNodes, RaylibAMD_SceneWalk8Host,
 * RaylibAMD_SceneWalkStackHost, RaylibAMD_PlanViews, RaylibAMD_SceneCheckTrees, RaylibAMD_SceneRebuild, the first upload of a wide tree the device does not hold yet,
 * and whatever drops the scene's device copy for a new upload (Raylib_SetSunIlluminance, Raylib_SetSunDirection, a call that rebuilds a scene of moving cubes for
 * another time interval).
 * Scene bounds: the silhouette cull takes them from the root's boxes (48 bytes), which every move copies to pinned memory with its status; the NEXT call on the
 * scene, whichever it is, waits for that copy before it plans anything -- the device entry itself does not wait.  The same wait applies DSceneView::fastBary as a
 * fresh scene would have it (a count of the triangles whose divisor lies outside [2^-62, 2^125] is kept on the device).
 * Ordering: the host entry is synchronous.  The device entry with stream == NULL runs on the library's stream, synchronously; with a hipStream_t it is enqueued
 * there behind the scene's synchronous first upload and returns.  Either waits for multi-rank frames in flight and goes behind the library's work in flight on
 * other streams (the ray queries' ring, the path calls' event); the library's later work on the scene is ordered behind the move by the move's event, which the next
 * call on the scene waits for ON THE HOST, whatever stream it is given: a RaylibAMD_TraceRaysDevice enqueued right behind a move returns once the move has completed
 * (the caller writes no synchronisation between the two; the library makes one).  Work of the caller's own is ordered by the caller's stream.  With RAYLIB_NUM_GPUS > 1
 * every device's copy of the scene is moved: the same kernels on a stream of each device, a device entry's values peer-copied from rank 0's device behind an event on the
 * call's stream, which in turn waits for those copies (the caller may overwrite the values behind the call).
 * Returns 1 (count == 0 included), or 0 with nothing changed for: a scene unknown or not finalized; first < 0, count < 0 or a range past
 * RaylibAMD_SceneNumTriangles; NULL positions with count > 0; a progressive session open on the scene (its sums would mix two scenes); no device; a value
 * that is not finite (host entry: scanned before anything is touched); device entry: a pointer that is not memory of rank 0's device or not 4-byte aligned.
 * The device entry's values are scanned by a kernel in front of the one that writes the records: a value that is not finite raises a flag, the records kernel then
 * writes nothing and the refit behind it reproduces the boxes that were there.  With stream == NULL the call returns 0; on a caller's stream it has returned 1
 * already, and the next call on the scene logs "that move was NOT applied" and goes on with the unmoved scene. */
RAYLIB_API int32_t RaylibAMD_SceneMoveTriangles(SceneHandle scene, int32_t first, int32_t count, const float* positions, const float* normals);
RAYLIB_API int32_t RaylibAMD_SceneMoveTrianglesDevice(SceneHandle scene, int32_t first, int32_t count, const float* positions, const float* normals, void* stream);
/* The existing host build on the current triangles (read back first where the host's are stale) and a fresh upload at the next call: restores the trees'
 * quality after large moves.  Results keep their bits.  Returns 1, or 0 for a scene unknown or not finalized. */
RAYLIB_API int32_t RaylibAMD_SceneRebuild(SceneHandle scene);
/* Test hook: reads the trees and the triangle records the device holds back and runs the builder's validity checks (RaylibAMD_SceneBVHInfo / BVH4Info / BVH8Info's)
 * on them against the current triangles.  Returns 1 when all pass; else 0 with *outFailedTree (may be NULL) = 2, 4 or 8 for the first tree that failed, or 0
 * when the check could not run (no device, scene unknown or not finalized). */
RAYLIB_API int32_t RaylibAMD_SceneCheckTrees(SceneHandle scene, uint32_t* outFailedTree);
/* Test hook: the VALUES of the wide formats the device holds.  Per device copy of the scene, its binary nodes are read back and the host's statement of the
 * refit rule (csrc/rl_grid.h through rl_bvh.cc RefitWideFromBinary: the double-precision grid of the 4-wide and 8-wide nodes) is applied to them on the host;
 * the result is compared byte for byte with the float-4, grid-4, leaf-list and 8-wide arrays that copy holds (a format it does not hold is not compared), and
 * the copy's triangle records with those of rank 0's copy.  Holds for a scene that was never moved too: the builder quantises with the same rule from the same
 * boxes.  Returns 1 when all are equal; else 0 with *outDiffMask (may be NULL) = a bit per format that differs -- 1 float-4, 2 grid-4, 4 leaf list, 8 8-wide,
 * 16 records --, or 0 when the check could not run (no device, scene unknown or not finalized, a failed read-back).  Like every call on the scene it waits for
 * a move in flight; it changes nothing in the scene, the host's copies and whether they are stale included. */
RAYLIB_API int32_t RaylibAMD_SceneCompareTrees(SceneHandle scene, uint32_t* outDiffMask);

/* ---- host-logic introspection (no GPU needed) ---------------------------------- */
/* Flattened scene as the kernels see it.  Triangle record = 26 words, material record =
 * 19 words, both laid out as oracle/flat_scene.h FlatTriangle / FlatMaterial. */
RAYLIB_API int32_t RaylibAMD_SceneNumTriangles(SceneHandle scene);
RAYLIB_API int32_t RaylibAMD_SceneNumMaterials(SceneHandle scene);
RAYLIB_API int32_t RaylibAMD_SceneNumTextures(SceneHandle scene);
RAYLIB_API void    RaylibAMD_SceneExportTriangles(SceneHandle scene, void* outTriangles);
RAYLIB_API void    RaylibAMD_SceneExportMaterials(SceneHandle scene, void* outMaterials);
/* The finalized scene's leaf order: outOrder[slot] = the RaylibAMD_SceneExportTriangles index of the triangle in slot `slot` (RaylibAMD_SceneNumTriangles words).
 * The slot is what ray queries break exact-t ties with (statement M2).  Returns 1, 0 for a null argument or a scene not finalized. */
RAYLIB_API int32_t RaylibAMD_SceneExportTriOrder(SceneHandle scene, uint32_t* outOrder);
RAYLIB_API void    RaylibAMD_SceneTextureSize(SceneHandle scene, int32_t index, int32_t* outW, int32_t* outH);
RAYLIB_API void    RaylibAMD_SceneExportTexture(SceneHandle scene, int32_t index, float* outRGBA);
RAYLIB_API void    RaylibAMD_SceneGetSun(SceneHandle scene, float outIlluminance[3], float outDirection[3]);
/* BVH shape: nodes (64 B each), depth, and a host-side validity check (every triangle
 * inside its leaf's box, every child box inside its parent's).  Returns 1 if valid. */
RAYLIB_API int32_t RaylibAMD_SceneBVHInfo(SceneHandle scene, uint32_t* outNodes, uint32_t* outDepth, float* outSahCost);
/* The 4-wide collapse of the tree that the pool schedule traverses on large scenes: 0 = the scene has none (fewer than 8 triangles, or
 * analytic primitives), 1 = present and structurally valid (every triangle once, boxes nested, stack bound holds), -1 = invalid. */
RAYLIB_API int32_t RaylibAMD_SceneBVH4Info(SceneHandle scene, uint32_t* outNodes4, uint32_t* outWorstCaseStack);
/* The 8-wide collapse (80-byte grid nodes, children in octant order; scenes of more than 108 triangles): 0 = none, 1 = present and valid (every triangle slot
 * reached once, every node's 8-bit grid boxes contain the triangles below them, no path longer than *outLevels), -1 = invalid.  outSteps4 / outSteps8: the sum
 * over the 4-wide / 8-wide tree's nodes of (node area / root area) -- the node steps a random ray is expected to take; the megakernel walks the 8-wide
 * tree when outSteps4 >= 40 (RAYLIB_BVH8=0|1 overrides; RaylibAMDStats.treeWidth says which tree a frame walked). */
RAYLIB_API int32_t RaylibAMD_SceneBVH8Info(SceneHandle scene, uint32_t* outNodes8, uint32_t* outLevels, float* outSteps4, float* outSteps8);
/* The megakernel's walk of that tree restated on the host, operation by operation in float (csrc/rl_bvh.cc Walk8Host: the ray's per-node factors and error allowance, one fma per
 * 8-bit grid plane, octant visiting order, one stack entry per level), with the exit distance of ray i fixed at tMax[i]: outT[i] = the least distance among the triangles of the leaf
 * children the walk reaches (a tolerant double-precision triangle test; FLT_MAX: none), outSteps[i] (may be NULL) the node steps.  No device needed: what the box
 * arithmetic must never do -- skip the leaf of the closest hit -- is checked against the CPU oracle in `pytest -m "not gpu"`.  rays: count x (origin, direction).
 * Returns 1, 0 without such a tree, -1 on a malformed tree. */
RAYLIB_API int32_t RaylibAMD_SceneWalk8Host(SceneHandle scene, const float* rays, int32_t count, float tMin, const float* tMax, float* outT, uint32_t* outSteps);
/* The stack discipline of the device walks restated on the host (csrc/rl_bvh.cc WalkStackHost), with the stack's capacity as an argument.  tree 2: the binary
 * tree (Traverse / NodeStep), 3: the 4-wide float boxes (Traverse4 of k_trace's FULL instances), 4: the 4-wide grid nodes (Traverse4 / NodeStep4), 8: the 8-wide tree (NodeStep8; capacity counts groups).  Box tests and child order
 * in float as on the device, the exit distance shrinking with the best hit, and the device's guard: a push at sp == capacity is dropped.  outT[i] = the closest hit
 * over [tMin, FLT_MAX] by the reference's triangle test and the ray queries' candidate rule (spheres and cubes, tree 2, at ray time 0; no cut-out test; INFINITY: none);
 * outHighWater[i] (may be NULL) = the most entries ray i held.  At the capacity rl_plan.cc gives an instance every ray must get the brute-force answer; at one less a
 * ray that fills the stack loses a subtree (tests/test_stack_edges_host.py).  rays: count x (origin, direction).  Returns 1, 0 for a bad argument or a scene
 * without that tree, -1 on a malformed tree.  No device needed. */
RAYLIB_API int32_t RaylibAMD_SceneWalkStackHost(SceneHandle scene, int32_t tree, const float* rays, int32_t count, float tMin, int32_t capacity, float* outT, uint32_t* outHighWater);
/* The leaf list of a small scene (at most 24 leaves, 108 triangles): what k_trace walks instead of the tree when the scene is LDS-resident.
 * Returns the number of leaves (0 = the scene has none); the list's validity is part of RaylibAMD_SceneBVH4Info's check. */
RAYLIB_API int32_t RaylibAMD_SceneLeafListInfo(SceneHandle scene, uint32_t* outMaxTrianglesPerLeaf);
/* 1 when no material of the finalized scene has a texture slot and no leaf of its leaf list carries the cut-out bit: with no sky image, k_trace's leaf
 * list is then walked by the kernel's plain instance (no texture, cut-out or sky code; RAYLIB_PLAIN_KERNEL=0 keeps the general one).  0 otherwise.  No device needed. */
RAYLIB_API int32_t RaylibAMD_ScenePlain(SceneHandle scene);
/* 1 when the megakernel of the last path-traced render on this process was the leaf-list kernel's plain instance, else 0. */
RAYLIB_API int32_t RaylibAMD_LastTracePlain(void);
/* 1 when the finalized scene may be rendered by the plain instance's lazy-reflectance form, which evaluates a vertex's reflectance only on paths that end with
 * light in them (the same bits; csrc/rl_dev_shade.h): RaylibAMD_ScenePlain, triangles only, every material a triangle uses microfacet (emission finite,
 * roughness in [2^-10, 1], |albedo| and |metallic| <= 16) or a mirror (|albedo| <= 16).  A render takes it when the plain instance's conditions hold and maxPathLength <= 4096; RAYLIB_LAZY_REFL=0 keeps the eager instance.  No device needed. */
RAYLIB_API int32_t RaylibAMD_SceneLazyRefl(SceneHandle scene);
/* 1 when the megakernel of the last path-traced render on this process was that lazy-reflectance instance (then RaylibAMD_LastTracePlain is 1 too), else 0. */
RAYLIB_API int32_t RaylibAMD_LastTraceLazy(void);
/* 1 when that lazy-reflectance launch was the instance's hit-queue form (k_trace_lazy_hitq: idle lanes take camera rays that have been traced already, so every
 * lane enters the shading part with a hit; the same bits and the same work counters, RaylibAMDStats::waveTrips aside).  A lazy render with maxPathLength >= 1
 * takes it; RAYLIB_HIT_QUEUE=0 keeps the ray-queue instance.  Else 0. */
RAYLIB_API int32_t RaylibAMD_LastHitQueue(void);
/* 1 when that lazy-reflectance launch kept a lit-sample mask (csrc/rl_lit_mask.h): samples that are all zero bits were neither stored nor summed, the same bits.
 * A one-view render that is not progressive takes it for launches of at most 256 samples per pixel, without a sun; RAYLIB_LIT_MASK=0 keeps every sample stored,
 * =1 takes the mask with a sun too.  Else 0. */
RAYLIB_API int32_t RaylibAMD_LastLitMask(void);
/* What a one-rank Raylib_Render of `settings` would launch under the current environment (csrc/rl_plan.cc): the kernel instance, its tree and the job
 * layout of its first launch over every cell of the frame, for a device of numCUs CUs on which the kernel fits workgroupsPerCU workgroups.  No device needed.
 * Returns 1, -1 when the scene's BVH is too deep to render (the plan is then not filled in further), 0 for a bad argument or a scene not finalized. */
typedef struct RaylibAMDRenderPlan {
	int32_t pathTrace;        /* 0: a debug render mode (k_aov on the BVH2) */
	int32_t stack, prims;     /* the instance's STACK; spheres or cubes */
	int32_t poolK;            /* 0: k_trace; K: k_trace_pool, 64 K paths per wave */
	int32_t tree;             /* 0 none (the leaf list), 1 BVH2, 2 4-wide float boxes, 3 4-wide grid nodes, 4 8-wide */
	int32_t lstack;           /* k_trace_pool: traversal-stack entries in LDS */
	int32_t lds;              /* k_trace: 0, 1 the scene in LDS, 2 the leaf list */
	int32_t plain;            /* the leaf-list kernel's plain instance */
	uint32_t pathsPerWave, treeWidth, nodeBytes;   /* as RaylibAMDStats reports them */
	int32_t keepNodes4, keepNodes4f;               /* the launch carries the grid / float-box wide nodes */
	int32_t eagerTree;        /* the wide tree the scene's upload puts on the device (tree code, 0: none) */
	uint32_t batch, sampleCount, blocks, stackStride, jobChunk, heads, jobsPerHead, guideShift;
	uint64_t jobs;
	int32_t lazy;             /* the plain instance's lazy-reflectance form (k_trace_lazy or its hit-queue form); 0 for a batch of views, whose twin stays eager */
	int32_t hitQueue;         /* ... and of that, its hit-queue form (k_trace_lazy_hitq); the field was `reserved`, always 0 */
} RaylibAMDRenderPlan;
RAYLIB_API int32_t RaylibAMD_PlanRender(SceneHandle scene, const RendererSettings* settings, int32_t hasSky, int32_t numCUs, int32_t workgroupsPerCU, RaylibAMDRenderPlan* out);
/* ---- several views of one scene in one megakernel launch (INTEGRATION.md "Several views") ---- */
#define RAYLIB_AMD_MAX_VIEWS 64
/* Renders `count` views of one scene at one RendererSettings.  outImages[i] receives, bit for bit, what
 * Raylib_Render(settings, scene, cameras[i], outImages[i]) would give with the same seed, in every render mode.
 * Each image is resized to the viewport, and its result stays on the device as after Raylib_Render.
 * RaylibAMD_GetLastStats reports the batch: counters summed over the views, one megakernel launch per sample
 * batch for the whole set.  Returns 1, or 0 with no image touched when:
 *   - an argument is null, or count is outside 1..RAYLIB_AMD_MAX_VIEWS;
 *   - a camera or image handle is 0 or unknown, or an image appears twice;
 *   - the scene is not finalized, or the viewport is empty;
 *   - the job count of a one-sample batch would overflow (count * cells of the viewport * 64 > 0xF0000000);
 *   - the scene has moving cubes and the cameras' shutter intervals differ (its boxes are built for one interval);
 *   - there is no device.
 * With RAYLIB_NUM_GPUS > 1 the batch renders on rank 0's device, as a progressive session does. */
RAYLIB_API int32_t RaylibAMD_RenderViews(const RendererSettings* settings, SceneHandle scene,
        const CameraHandle* cameras, int32_t count, const ImageHandle* outImages);
/* The same into caller device memory: count * W * H * 4 floats, view-major, row-major inside a view.
 * outDevice == 0: the library's own buffer (for timing), as RaylibAMD_RenderDevice. */
RAYLIB_API int32_t RaylibAMD_RenderViewsDevice(const RendererSettings* settings, SceneHandle scene,
        const CameraHandle* cameras, int32_t count, void* outDevice);
/* What RaylibAMD_RenderViews would launch under the current environment, as RaylibAMD_PlanRender for one view: the instance and tree (those of the one-view
 * plan) and the job layout of the first launch over every view's listed cells.  outCellEmpty (count * ceil(W/8) * ceil(H/8) bytes, may be null): per cell of
 * each view, view by view, 1 when it is dropped from the job list (RaylibAMD_CullCells of that view's camera).  hasSky as for RaylibAMD_PlanRender.  No device
 * needed.  Returns 1, -1 when the scene's BVH is too deep to render, 0 for a bad argument (as RaylibAMD_RenderViews refuses them), a scene not finalized or a
 * job count that would overflow. */
RAYLIB_API int32_t RaylibAMD_PlanViews(SceneHandle scene, const RendererSettings* settings, const CameraHandle* cameras, int32_t count, int32_t hasSky,
        int32_t numCUs, int32_t workgroupsPerCU, RaylibAMDRenderPlan* outPlan, uint8_t* outCellEmpty);
/* FNV-1a of the flat BVH (node records + leaf order): the multi-threaded build (RAYLIB_BUILD_THREADS, default = host
 * threads, <= 32) must give the tree of the single-threaded one. */
RAYLIB_API uint64_t RaylibAMD_SceneBVHHash(SceneHandle scene);
/* FNV-1a of the trees' topology alone -- child references, leaf order, the 8-wide nodes' masks and bases, no box: unchanged by
 * RaylibAMD_SceneMoveTriangles (the "same topology" signal), changed by RaylibAMD_SceneRebuild whenever the build comes out differently.  No device needed. */
RAYLIB_API uint64_t RaylibAMD_SceneTopologyHash(SceneHandle scene);
/* The binary tree's nodes as the host holds them (read back first after a move), 64 bytes each: lmin[3] lmax[3] rmin[3] rmax[3] (float), left, right (int32: >= 0 an
 * inner node's index, < 0 a leaf reference or 0x80000000 for none), two words of padding; node 0 is the root.  out may be NULL.  Returns the number of nodes. */
RAYLIB_API int32_t RaylibAMD_SceneExportBVHNodes(SceneHandle scene, void* out);
/* Camera derived state: 19 floats origin(3) lensRadius top_left(3) horizontal(3) vertical(3) u(3) v(3)
 * (reference render/camera.h:55-78). */
RAYLIB_API void    RaylibAMD_CameraExport(CameraHandle camera, float out[19]);
/* Create an image from caller memory (RGBA float, row 0 = top): lets tests use textures
 * and sky panoramas without an image codec. */
RAYLIB_API ImageHandle RaylibAMD_CreateImageFromData(uint32_t width, uint32_t height, const float* rgba);
/* Copy RGBA (4 floats per pixel) of an image to caller memory. */
RAYLIB_API void    RaylibAMD_DumpImageRGBA(ImageHandle image, float* outRGBA);
/* Test hook: the OBJ / MTL parser's number reader (value of strtof for one token). */
RAYLIB_API float   RaylibAMD_ParseFloat(const char* token);
/* Size of an image created by Raylib_LoadImage / Raylib_CreateImage (the reference ABI has no accessor). Returns 1 on success. */
RAYLIB_API int32_t RaylibAMD_ImageSize(ImageHandle image, uint32_t* outWidth, uint32_t* outHeight);
/* Replace a material's texture by an image handle (slot: 0 albedo, 1 normal, 2 roughness,
 * 3 metallic, 4 emissive) -- the OBJ loader does the same from map_* statements. */
RAYLIB_API int32_t RaylibAMD_OBJModelSetTexture(OBJModelHandle obj, const char* materialName, int32_t slot, ImageHandle image);

/* ---- denoiser: an edge-avoiding a-trous wavelet filter guided by the Albedo and MicrosurfaceNormal AOVs (csrc/rl_denoise.hip
 *      defines it exactly).  Inputs are RGBA float images of one size; their alpha is ignored; the output's alpha is 1. ---- */
typedef struct RaylibAMDDenoiseParams {
	int32_t iterations;       /* K, 1 .. 8: filter steps 1, 2, 4, ... 2^(K-1) pixels apart */
	float   sigmaColor;       /* tolerance of the colour distance (halved per step); each sigma in [1e-3, 1e3] */
	float   sigmaNormal;      /* ... of the normal distance */
	float   sigmaAlbedo;      /* ... of the albedo distance */
} RaylibAMDDenoiseParams;
/* NULL params = defaults. albedo / normal may be 0. Returns 1 on success; 0 on a null main / out, a guide whose size differs from
 * main's, params out of range, or no device. On 0, out is untouched.  out is reallocated to main's size and may be main; the result
 * stays on the device as after Raylib_Render (Raylib_PostProcess / Raylib_DumpImageData work on it there). */
RAYLIB_API int32_t RaylibAMD_Denoise(ImageHandle main, int32_t bHDR, ImageHandle albedo, ImageHandle normal,
                                     ImageHandle out, const RaylibAMDDenoiseParams* params);
/* The same filter on the host, on caller arrays of W*H*4 floats: the oracle of the device path, no device needed.
 * Same return convention (outRGBA may be colorRGBA). */
RAYLIB_API int32_t RaylibAMD_DenoiseHost(uint32_t width, uint32_t height, const float* colorRGBA, int32_t bHDR,
                                         const float* albedoRGBA, const float* normalRGBA,
                                         const RaylibAMDDenoiseParams* params, float* outRGBA);
/* Process-wide switch, default off (the env var RAYLIB_DENOISER=1 turns it on for unmodified front-ends).
 * On: Raylib_IsDenoiserSupported() returns RaylibAMD_DeviceAvailable(), and Raylib_Denoise(m, hdr, a, n, o)
 * = RaylibAMD_Denoise(m, hdr, a, n, o, NULL). Off: both keep today's behaviour exactly (return 0). */
RAYLIB_API void    RaylibAMD_EnableDenoiser(int32_t enable);

/* ---- progressive rendering: a frame in passes of samples, each pass ending with a preview, and (optionally) cells that stop early.
 *      After any sequence of passes that brings an 8x8 cell to n samples, that cell's pixels are bit for bit those of Raylib_Render with
 *      samplesPerPixel = n and the same settings, scene, camera and seed: a uniform session previews one-shot frames, an adaptive one ends
 *      with a mosaic of them.  A session renders on the first device (RAYLIB_NUM_GPUS > 1: rank 0's). ---- */
typedef uintptr_t RaylibAMDProgressiveHandle;
typedef struct RaylibAMDProgressiveParams {
	float    threshold;   /* adaptive stopping: a cell stops when its error (below) is < threshold; 0 = never (uniform passes); finite, >= 0 */
	uint32_t minSamples;  /* samples every cell takes before it may stop; >= 2 */
} RaylibAMDProgressiveParams;
/* The stopping rule.  Every sample's y = L / (1 + L), L its luminance (0.2126 R + 0.7152 G + 0.0722 B, as Raylib_PostProcess); per pixel
 * S1 = sum of y and S2 = sum of y * y in float, in sample order.  A pixel's error after n samples is
 * se = sqrt(max(0, (S2 - S1 * S1 / n) / (n - 1)) / n), +inf when S1, S2 or se is not finite; a cell's error is the largest of its valid pixels'.  After a
 * pass, a live cell stops when n >= minSamples and its error < threshold; culled cells (outside the scene's silhouette) follow the same rule. */

/* Opens a session on (settings, scene, camera) that renders into `out` in passes; settings->samplesPerPixel (max(1, .)) is the cap.
 * The seed (RaylibAMD_SetSeed / RAYLIB_SEED), the camera and the settings are captured here; `out` is resized to the viewport as by
 * Raylib_Render.  params == NULL: uniform passes.  Returns 0 when an argument is null, the scene is not finalized, the render mode is not
 * RAYLIB_RENDERMODE_Default, params are out of range, the viewport is empty, or there is no device. */
RAYLIB_API RaylibAMDProgressiveHandle RaylibAMD_BeginProgressive(const RendererSettings* settings, SceneHandle scene, CameraHandle camera,
                                                                 ImageHandle out, const RaylibAMDProgressiveParams* params);
/* Renders up to `samples` (>= 1) more samples per live cell (clamped to the cap), then rewrites every pixel of `out` with its cell's mean
 * so far; the result stays on the device, as after Raylib_Render, and RaylibAMD_GetLastStats reports this pass.  Returns the number of
 * cells still live (0 = finished: every cell stopped or reached the cap; a later Step does nothing and returns 0), or -1: a null, unknown
 * or ended handle, samples == 0, a scene that changed since Begin (finalized anew, sun, shutter), a sky panorama that changed, an image
 * that was resized or destroyed, or a device failure.  On -1 the image and the session are unchanged (a device failure excepted). */
RAYLIB_API int32_t RaylibAMD_ProgressiveStep(RaylibAMDProgressiveHandle h, uint32_t samples);
/* Per cell (cellsX * cellsY, row-major): its samples so far and 1 if it has stopped; per pixel (W * H, row-major): S1 and S2 of the rule.
 * Any pointer may be NULL.  Returns 1, or 0 for an unknown handle or without a device. */
RAYLIB_API int32_t RaylibAMD_ProgressiveExport(RaylibAMDProgressiveHandle h, uint32_t* cellSamples, uint8_t* cellStopped, float* sumY, float* sumY2);
/* Frees the session's device buffers (the image stays as the last pass left it).  1, or 0 for an unknown handle.  A session that is never
 * ended holds its buffers until the process exits, as an image that is never destroyed does. */
RAYLIB_API int32_t RaylibAMD_EndProgressive(RaylibAMDProgressiveHandle h);
/* The stopping rule on the host, the oracle of the device's decision (no device needed): for a W x H frame's cells with the given sample
 * counts and moments (as exported), one byte per cell in outStop, 1 = the cell stops.  params == NULL: uniform (nothing stops).
 * Returns 1, or 0 for a null array or params out of range. */
RAYLIB_API int32_t RaylibAMD_ProgressiveDecideHost(uint32_t width, uint32_t height, const uint32_t* cellSamples, const float* sumY,
                                                   const float* sumY2, const RaylibAMDProgressiveParams* params, uint8_t* outStop);
/* Test hook: the kernel that rewrites a session's lists after a pass, on arrays of the caller's, launched as a pass launches it.  live: numLive cells of a
 * width x height frame in ascending order (numCells = its 8x8 cells, row-major); stopped, emptyOrNull: one byte per cell (empty: outside the silhouette;
 * NULL: no cell is).  outLive receives the entries of live whose cell has not stopped, in order; outTrace those of them that are not empty, in order; both
 * have room for numLive entries and are written only up to their counts.  outCounts: [0] entries of outLive, [1] entries of outTrace, [2..3] the valid
 * pixels of the kept empty cells, low and high word.  Returns 1; 0 -- and nothing is written -- without a device, for a null pointer other than emptyOrNull,
 * numLive > numCells, a numCells that is not the frame's cell count (an empty frame included) or an entry of live >= numCells. */
RAYLIB_API int32_t RaylibAMD_ProgressiveCompactTest(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const uint8_t* emptyOrNull, uint32_t numCells,
                                                    uint32_t width, uint32_t height, uint32_t* outLive, uint32_t* outTrace, uint32_t outCounts[4]);

#ifdef __cplusplus
}
#endif
#endif /* RAYLIB_AMD_H */
