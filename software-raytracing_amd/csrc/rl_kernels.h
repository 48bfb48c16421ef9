// Every kernel the host runtime (rl_rt_*.hip) launches: its prototype, its instance list and the explicit instantiation declarations, each written once, and
// the structs a kernel shares with the host.  A kernel's body always defines it; the unit that holds the body owns the kernel and follows it with the
// instantiation definitions (RL_..._INSTANCES(RL_K_...)), every other unit sees what is here.  No kernel lives in a runtime unit.
//   rl_render.hip        k_trace, k_resolve, k_aov, k_closest_hit and the small kernels (progressive resolve and compaction, post-processing, RGB packing,
//                        the multi-rank scatter, the test hooks)
//   rl_render_views.hip  k_trace_views, k_resolve_views, k_aov_views: the views twins (RaylibAMD_RenderViews).  Instantiated beside the one-view kernels they
//                        change how the helpers both call are inlined into those (tools/isa_equivalence.py)
//   rl_render_lazy.hip   k_trace_lazy, k_trace_lazy_hitq, k_resolve_lit, k_verify_lazy_refl, k_verify_lazy_pdf, k_verify_sampler_ranged, k_verify_normalize_ranged: the leaf-list kernel's lazy-reflectance instance.  Beside the other k_trace instances it
//                        changes how two loops of the eager PLAIN instance are scheduled
//   rl_render_pool.hip   k_trace_pool and its twin: a scheduler strategy of its own (Makefile POOLFLAGS)
//   rl_query.hip         k_query (RaylibAMD_TraceRays): beside the render kernels it would change how the walks they share are inlined into those
//   rl_gbuffer.hip       k_gbuffer (RaylibAMD_RenderGBuffer): k_aov's camera rays and debug modes on k_query's driver and walks, with the render's hit rule -- the
//                        query unit widens the candidate rule, so this one is apart from it, and from the render kernels for k_query's reason
//   rl_motion.hip        k_motion (RaylibAMD_RenderMotion): k_gbuffer's pixels, rays and walks with another finish -- the hit plane and the motion plane
//                        (rl_motion.h); apart so that k_gbuffer and every other unit stay the code they are
//   rl_temporal.hip      k_temporal (RaylibAMD_TemporalAccumulate): a streaming kernel on planes (rl_temporal.h); no scene, no walk.  k_temporal_moments
//                        (RaylibAMD_TemporalAccumulateMoments): the same walk with the moments' planes beside it
//   rl_variance.hip      k_vf_pack, k_vf_variance, k_vf_iter (RaylibAMD_FilterVariance): the variance-guided a-trous filter on planes (rl_variance.h); no scene
//   rl_multihit.hip      k_query_all (RaylibAMD_TraceRaysAll): the binary and the 8-wide walk again with a sorted list behind the triangle test, written on the
//                        shared steps; apart so that k_query and every other unit stay the code they are
//   rl_nearest.hip       k_nearest (RaylibAMD_NearestPoints): a walk of its own (point-to-box distances, no ray), which shares with the others the records and the
//                        child sort alone; apart so that every other unit stays the code it is.  k_nearest_all (RaylibAMD_NearestPointsAll): that walk (rl_dev_boxwalk.h
//                        PointWalk, which this unit, rl_overlap.hip and rl_sdf.hip include) with a sorted list behind the triangle test
//   rl_sweep.hip         k_sweep (RaylibAMD_SweepSpheres): the point walk's shape with a time bound in the place of the distance (the entry time of the centre's
//                        path into a box grown by the radius) and the largest narrow phase of the family; its walk is its own text, so every other unit stays the code it is
//   rl_overlap.hip       k_overlap (RaylibAMD_OverlapTriangles): a walk of its own again (box against box, no ray, no distance) with a per-lane index list; apart for
//                        the same reason
//   rl_overlap_box.hip   k_overlap_box (RaylibAMD_OverlapBoxes): k_overlap's walk written again, driven by the box that encloses an oriented query box, with a
//                        box-against-triangle leaf test and a bit mask as a third output kind; apart so that rl_overlap.hip stays the code it is
//   rl_sdf.hip          k_sdf_rows, k_sdf_parity, k_sdf_dist (RaylibAMD_BakeDistanceField): k_query_all's counting walks written again and k_nearest's closest walk (PointWalk) on
//                        generated rays and points, with a bit volume between them; apart for the same reason
//   rl_radiance.hip      k_radiance (RaylibAMD_TraceRadiance): the same reason, towards the render and the query kernels alike
//   rl_gather.hip        k_gather (RaylibAMD_Gather: rl_k_radiance.inl's twin, the generator instances of its loop) and k_gather_resolve: beside k_radiance they would be
//                        more callers of the walks and the shading it inlines.  k_gather_resolve and k_gather_adaptive_resolve are one source, rl_k_gather_resolve.inl,
//                        which each of the two units includes (RL_GATHER_ADAPTIVE 0 / 1)
//   rl_gather_adaptive.hip  k_gather_adaptive_resolve, k_gather_compact_*, k_gather_scatter_counts (RaylibAMD_GatherAdaptive): behind the unchanged k_gather; apart
//                        from rl_gather.hip so that its kernels stay the code they are
//   rl_lightmap.hip      k_lm_*: the lightmap rasteriser, its scans and the atlas stages (RaylibAMD_BakeLightmap); no walk, no shading
//   rl_lightmap_filter.hip  k_lm_filter, k_lm_take: the atlas filter (RaylibAMD_BakeLightmapFiltered) and its host oracle, which share one per-texel function
//   rl_refit.hip         k_move_*, k_refit_*: a finalized scene's triangles moved and its trees refitted (RaylibAMD_SceneMoveTriangles); no walk, no shading
// A twin takes the view table (DViews) as one more trailing argument.  Default template arguments are given here and nowhere else.
#pragma once

#include "rl_dev_jobs.h"
#include "rl_dev_pool.h"
#include "rl_variance.h"

namespace rl {

// ---------------------------------------------------------------------------
// The megakernel.  samples: [sampleCount][numLocalCells*64] SampleRGB.
// pathStack: [maxPathLength][stackStride] records of 2 float4 (refl.xyz, sp | pdf, E.xyz).
#ifndef RL_QUEUE_SPIN_LIMIT
// 0: a wave waits for the workgroup's chunk until the wave that is refilling it is done (microseconds: one global atomic).  N > 0: after N waits of 128
// cycles it takes one batch straight from the global counter instead (1: test build that always does; parity-tested).  The bounded form is not the
// default because its few instructions change the register allocation of the whole loop: 14.98 ms against 14.79 on the Cornell frame (same box, interleaved).
#define RL_QUEUE_SPIN_LIMIT 0
#endif
#ifndef RL_TRACE_MIN_WAVES
#define RL_TRACE_MIN_WAVES 4   /* 4 waves per SIMD = 4 workgroups per CU: caps the kernel at 128 VGPRs */
#endif
// PRIMS: the scene holds spheres / cubes (their leaf and shading code is compiled out of the triangle-only variant)
// FULL: the wide tree, if the launch carries one, has float boxes (S.nodes4f) -- small scenes; else grid nodes (S.nodes4)
// LDS (with FULL, triangle scenes within the RL_LDS_MAX* limits): the scene's records are copied to LDS at the start and read from there;
//     LDS == 2: a scene of <= 16 leaves, walked through its leaf list (TraverseLeafList) instead of its tree
// (STACK, PRIMS, FULL, LDS, PLAIN): every instance rl_rt_frame.hip KernelFor names.
#define RL_TRACE_ARGS const DRenderParams, const DSceneView, const SkyRot, SampleRGB* __restrict__, float* __restrict__, unsigned long long* __restrict__, unsigned int* __restrict__
template <int STACK, bool PRIMS, bool FULL, int LDS = 0, bool PLAIN = false>
__global__ void __launch_bounds__(RL_BLOCK, (STACK <= 32 ? RL_TRACE_MIN_WAVES : 2)) k_trace(RL_TRACE_ARGS);
template <int STACK, bool PRIMS, bool FULL, int LDS = 0, bool PLAIN = false>
__global__ void __launch_bounds__(RL_BLOCK, (STACK <= 32 ? RL_TRACE_MIN_WAVES : 2)) k_trace_views(RL_TRACE_ARGS, const DViews);
#define RL_TRACE_INSTANCES(X) \
	X(16, false, false, 0, false) X(16, false, true, 0, false) X(16, false, true, 1, false) X(16, false, true, 2, false) X(16, false, true, 2, true) \
	X(32, false, false, 0, false) X(32, false, true, 0, false) X(32, true, false, 0, false) X(32, true, true, 0, false) \
	X(64, false, false, 0, false) X(64, false, true, 0, false) X(64, true, false, 0, false) X(64, true, true, 0, false)
#define RL_K_TRACE(a, b, c, d, e) template __global__ void k_trace<a, b, c, d, e>(RL_TRACE_ARGS);
#define RL_K_TRACE_VIEWS(a, b, c, d, e) template __global__ void k_trace_views<a, b, c, d, e>(RL_TRACE_ARGS, const DViews);
RL_TRACE_INSTANCES(extern RL_K_TRACE)
RL_TRACE_INSTANCES(extern RL_K_TRACE_VIEWS)
// The lazy-reflectance instance of the leaf-list kernel's PLAIN instance (rl_k_trace.inl RL_LAZY_REFL, rl_dev_shade.h): a kernel name of its own with the lit list as
// one more trailing argument, so that every other instance keeps its name and its code.  Its waves fold the list's entries themselves, a chunk of 64 in 64 lanes
// (rl_dev_litfold.h): no kernel follows it but the resolve.
template <int STACK, bool PRIMS, bool FULL, int LDS, bool PLAIN>
__global__ void __launch_bounds__(RL_BLOCK, (STACK <= 32 ? RL_TRACE_MIN_WAVES : 2)) k_trace_lazy(RL_TRACE_ARGS, const DLitList);
#define RL_TRACE_LAZY_INSTANCES(X) X(16, false, true, 2, true)
#define RL_K_TRACE_LAZY(a, b, c, d, e) template __global__ void k_trace_lazy<a, b, c, d, e>(RL_TRACE_ARGS, const DLitList);
RL_TRACE_LAZY_INSTANCES(extern RL_K_TRACE_LAZY)
// The lazy instance's hit-queue form (rl_k_trace_hitq.inl): the same arguments, the same paths and the same fold of the lit list; its idle lanes take camera rays
// that have been traced already, so that every lane enters the shading part with a hit.
template <int STACK, bool PRIMS, bool FULL, int LDS, bool PLAIN>
__global__ void __launch_bounds__(RL_BLOCK, (STACK <= 32 ? RL_TRACE_MIN_WAVES : 2)) k_trace_lazy_hitq(RL_TRACE_ARGS, const DLitList);
#define RL_K_TRACE_LAZY_HITQ(a, b, c, d, e) template __global__ void k_trace_lazy_hitq<a, b, c, d, e>(RL_TRACE_ARGS, const DLitList);
RL_TRACE_LAZY_INSTANCES(extern RL_K_TRACE_LAZY_HITQ)
// k_resolve for a batch of the lazy instance with a lit-sample mask (rl_lit_mask.h): the slot's flagged samples alone
__global__ void __launch_bounds__(RL_BLOCK)
k_resolve_lit(const DRenderParams P, const DSceneView S, const SkyRot R, const SampleRGB* __restrict__ samples, float4* __restrict__ accum, float4* __restrict__ out,
              int firstBatch, int lastBatch, const DLitList LL);

// ---------------------------------------------------------------------------
// The pool megakernel (rl_dev_pool.h, rl_k_trace_pool.inl): k_trace's arguments.
// STACK: capacity of the traversal stack; LSTACK <= STACK: how much of it lives in LDS (the rest is private overflow)
// WIDE: 0 the BVH2; 1 the BVH4 (S.nodes4: 64-byte grid nodes); 3 the 8-wide tree (S.nodes8; STACK / LSTACK then count words: two per group)
template <int STACK, bool PRIMS, int K, int LSTACK = STACK, int WIDE = 0>
__global__ void __launch_bounds__(RL_BLOCK, (PoolOcc<LSTACK, PRIMS, K>::kBlocks)) k_trace_pool(RL_TRACE_ARGS);
template <int STACK, bool PRIMS, int K, int LSTACK = STACK, int WIDE = 0>
__global__ void __launch_bounds__(RL_BLOCK, (PoolOcc<LSTACK, PRIMS, K>::kBlocks)) k_trace_pool_views(RL_TRACE_ARGS, const DViews);
// The instances the runtime selects from (rl_rt_frame.hip KernelFor)
#define RL_POOL_INSTANCES(X) \
	X(16, false, 2, 16, 0) X(16, false, 3, 16, 0) X(16, false, 4, 16, 0) X(32, false, 2, 32, 0) X(32, false, 3, 32, 0) X(32, false, 4, 32, 0) \
	X(32, false, 2, 4, 0) X(32, false, 2, RL_POOL_SHORT_LSTACK, 0) \
	X(32, false, 2, 32, 1) X(64, false, 2, 32, 1) X(32, false, 2, RL_POOL_SHORT_LSTACK, 1) X(64, false, 2, RL_POOL_SHORT_LSTACK, 1) \
	X(2 * RL_POOL8_MAXLEVELS, false, 2, RL_POOL8_LSTACK, 3)
#define RL_K_TRACE_POOL(a, b, c, d, e) template __global__ void k_trace_pool<a, b, c, d, e>(RL_TRACE_ARGS);
#define RL_K_TRACE_POOL_VIEWS(a, b, c, d, e) template __global__ void k_trace_pool_views<a, b, c, d, e>(RL_TRACE_ARGS, const DViews);
RL_POOL_INSTANCES(extern RL_K_TRACE_POOL_VIEWS)
RL_POOL_INSTANCES(extern RL_K_TRACE_POOL)

// ---------------------------------------------------------------------------
// k_resolve (rl_k_resolve.inl) and k_aov (rl_k_aov.inl)
__global__ void __launch_bounds__(RL_BLOCK)
k_resolve(const DRenderParams P, const DSceneView S, const SkyRot R, const SampleRGB* __restrict__ samples, float4* __restrict__ accum, float4* __restrict__ out, int firstBatch, int lastBatch);
__global__ void __launch_bounds__(RL_BLOCK)
k_resolve_views(const DRenderParams Pb, const DSceneView S, const SkyRot R, const SampleRGB* __restrict__ samples, float4* __restrict__ accum, float4* __restrict__ out,
                int firstBatch, int lastBatch, const DViews V);
#define RL_AOV_ARGS const DRenderParams, const DSceneView, float4* __restrict__, unsigned long long* __restrict__
template <int STACK, bool PRIMS> __global__ void __launch_bounds__(RL_BLOCK) k_aov(RL_AOV_ARGS);
template <int STACK, bool PRIMS> __global__ void __launch_bounds__(RL_BLOCK) k_aov_views(RL_AOV_ARGS, const DViews);
#define RL_AOV_INSTANCES(X) X(16, false) X(32, false) X(32, true) X(64, false) X(64, true)
#define RL_K_AOV(a, b) template __global__ void k_aov<a, b>(RL_AOV_ARGS);
#define RL_K_AOV_VIEWS(a, b) template __global__ void k_aov_views<a, b>(RL_AOV_ARGS, const DViews);
RL_AOV_INSTANCES(extern RL_K_AOV)
RL_AOV_INSTANCES(extern RL_K_AOV_VIEWS)

// ---------------------------------------------------------------------------
// Progressive rendering (rl_rt.h ProgressiveSession; include/raylib_amd.h RaylibAMD_BeginProgressive)
// What a session keeps on the device, cell-major (slot = cell * 64 + pixel of the cell): the running colour sum in sample order, the moments of y, and
// per cell its samples so far and whether it has stopped.
struct ProgressiveState {
	float4* sum;
	float* s1;
	float* s2;
	uint32_t* cellSamples;
	uint8_t* stopped;
	float threshold;
	uint32_t minSamples;
};
__global__ void __launch_bounds__(RL_BLOCK)
k_progressive_resolve(const DRenderParams P, const DSceneView S, const SkyRot R, const SampleRGB* __restrict__ samples, const ProgressiveState st,
                      float4* __restrict__ out, int lastBatch);
#define RL_COMPACT_BLOCK 1024
#define RL_COMPACT_PER 8
__global__ void __launch_bounds__(RL_COMPACT_BLOCK)
k_progressive_compact(uint32_t* __restrict__ live, uint32_t* __restrict__ trace, const uint8_t* __restrict__ stopped, const uint8_t* __restrict__ empty,
                      uint32_t numLive, uint32_t width, uint32_t height, uint32_t cellsX, uint32_t* __restrict__ counts);

// ---------------------------------------------------------------------------
// Images (post-processing, the RGB dump) and the frame from the ranks' cell buffers (N > 1 behind Raylib_Render): cell c was rendered by rank c % N as its (c / N)-th cell
__global__ void __launch_bounds__(RL_BLOCK) k_pp_max(const float4* __restrict__ px, size_t n, unsigned int* __restrict__ whiteBits);
__global__ void __launch_bounds__(RL_BLOCK) k_pp_map(float4* __restrict__ px, size_t n, const unsigned int* __restrict__ whiteBits);
__global__ void __launch_bounds__(RL_BLOCK) k_pack_rgb(const float4* __restrict__ px, float4* __restrict__ out, float* __restrict__ outTail, size_t n);
struct ScatterPlan { uint32_t ranks; uint32_t offset[16]; };   // offset[r]: first float4 of rank r's cells in the gather buffer
__global__ void __launch_bounds__(RL_BLOCK)
k_scatter_cells(const float4* __restrict__ gather, float4* __restrict__ out, uint32_t width, uint32_t height, uint32_t cellsX, const ScatterPlan plan);

// ---------------------------------------------------------------------------
// The ray queries (RaylibAMD_TraceRays; rl_k_query.inl)
// A hit record as RaylibAMD_ClosestHit and the surface query of RaylibAMD_TraceRays return it (oracle/flat_scene.h FlatHit)
struct DHitOut { int32_t hit; float t; float p[3]; float n[3]; float paramU, paramV; int32_t material; };
enum { RL_QK_ANY = 0, RL_QK_CLOSEST = 1, RL_QK_SURFACE = 2 };   // RAYLIB_AMD_QUERY_*
// rays in (origin, direction: six floats) -> hit records out (RaylibAMD_ClosestHit, tests)
template <int STACK, bool PRIMS>
__global__ void __launch_bounds__(RL_BLOCK) k_closest_hit(const DSceneView S, const float* __restrict__ rays, int n, float tMin, DHitOut* __restrict__ out);
extern template __global__ void k_closest_hit<32, true>(const DSceneView, const float* __restrict__, int, float, DHitOut* __restrict__);
extern template __global__ void k_closest_hit<64, true>(const DSceneView, const float* __restrict__, int, float, DHitOut* __restrict__);
// Rays (k_query) or jobs (k_radiance) a wave takes per atomic on the global counter: one value for both kernels
#ifndef RL_QUERY_CHUNK
#define RL_QUERY_CHUNK 64u
#endif
struct DQueryHit { float t; int32_t prim; float b1, b2; };      // RaylibAMDHitT
// TREE: 2 the binary tree (S.nodes), 4 the grid nodes (S.nodes4), 8 the 8-wide tree (S.nodes8).  STACK: the walk's stack (TREE 8: RL_POOL8_MAXLEVELS groups).
// PRIMS: the scene holds spheres or cubes (binary tree only).  rays: n records of two float4 (org, tMin | dir, tMax).  counters: CNT_* sums, or null.
#define RL_QUERY_ARGS const DSceneView, const float4* __restrict__, uint32_t, float, void* __restrict__, int32_t* __restrict__, const int32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int KIND, int STACK, bool PRIMS> __global__ void __launch_bounds__(RL_BLOCK) k_query(RL_QUERY_ARGS);
// The instances rl_rt_rays.hip QueryKernelOfKind selects from: (TREE, KIND, STACK, PRIMS)
#define RL_QUERY_INSTANCES_K(X, K) \
	X(2, K, 32, false) X(2, K, 32, true) X(2, K, 64, false) X(2, K, 64, true) X(4, K, 32, false) X(4, K, 64, false) X(8, K, 2 * RL_POOL8_MAXLEVELS, false)
#define RL_QUERY_INSTANCES(X) RL_QUERY_INSTANCES_K(X, 0) RL_QUERY_INSTANCES_K(X, 1) RL_QUERY_INSTANCES_K(X, 2)
#define RL_K_QUERY(a, b, c, d) template __global__ void k_query<a, b, c, d>(RL_QUERY_ARGS);
RL_QUERY_INSTANCES(extern RL_K_QUERY)

// ---------------------------------------------------------------------------
// The primary-hit G-buffer (RaylibAMD_RenderGBuffer, statements G1 to G6; rl_k_gbuffer.inl)
// The planes a launch writes (mask; a plane not asked for has a null pointer and is not touched), row-major, width * height records each: hit (DQueryHit as one
// float4), surface (DHitOut), and the five colour planes k_aov's debug modes give (float4, alpha 1).  The frame, its 8 x 8 cells, rayTMin as the render uses it,
// the camera and the seed of the pixels' streams.
enum { RL_GB_HIT = 1u, RL_GB_SURFACE = 2u, RL_GB_ALBEDO = 4u, RL_GB_SURFACE_NORMAL = 8u, RL_GB_MICRO_NORMAL = 16u, RL_GB_TEXCOORD = 32u, RL_GB_EMISSION = 64u,
       RL_GB_COLOUR = RL_GB_ALBEDO | RL_GB_SURFACE_NORMAL | RL_GB_MICRO_NORMAL | RL_GB_TEXCOORD | RL_GB_EMISSION };
struct DGBuffer {
	DCamera camera;
	unsigned long long seed;
	uint32_t width, height, cellsX, numCells, mask;
	float rayTMin;
	float4* hit; DHitOut* surface;
	float4 *albedo, *surfaceNormal, *microNormal, *texcoord, *emission;
};
// TREE, STACK, PRIMS: as k_query's.  slotIndex: as k_query's (read for the hit plane).  cellCounter: the next cell (a wave takes RL_QUERY_CHUNK / 64 of them per
// atomic).  counters: CNT_* sums, or null.
#define RL_GBUFFER_ARGS const DSceneView, const DGBuffer, const int32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int STACK, bool PRIMS> __global__ void __launch_bounds__(RL_BLOCK) k_gbuffer(RL_GBUFFER_ARGS);
// The instances rl_rt_rays.hip GBufferKernelOf selects from, one per CLOSEST instance of k_query: (TREE, STACK, PRIMS)
#define RL_GBUFFER_INSTANCES(X) X(2, 32, false) X(2, 32, true) X(2, 64, false) X(2, 64, true) X(4, 32, false) X(4, 64, false) X(8, 2 * RL_POOL8_MAXLEVELS, false)
#define RL_K_GBUFFER(a, b, c) template __global__ void k_gbuffer<a, b, c>(RL_GBUFFER_ARGS);
RL_GBUFFER_INSTANCES(extern RL_K_GBUFFER)

// ---------------------------------------------------------------------------
// The motion plane (RaylibAMD_RenderMotion, statements T1 to T6; rl_k_motion.inl).  The launch is a G-buffer's (DGBuffer: the frame, the camera, the seed,
// rayTMin, and of the planes `hit` alone, mask RL_GB_HIT or 0) with the previous frame beside it: the previous camera, the range of triangles that had other
// vertices, their previous positions (nine floats each; null with count 0) and the motion plane (float4 {prevX, prevY, prevT, status}; null: not asked for).
struct DMotion {
	DCamera prevCamera;
	int32_t first, count;
	const float* prevPositions;
	float4* motion;
};
#define RL_MOTION_ARGS const DSceneView, const DGBuffer, const DMotion, const int32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int STACK, bool PRIMS> __global__ void __launch_bounds__(RL_BLOCK) k_motion(RL_MOTION_ARGS);
// one instance per instance of k_gbuffer (rl_rt_rays.hip MotionKernelOf)
#define RL_K_MOTION(a, b, c) template __global__ void k_motion<a, b, c>(RL_MOTION_ARGS);
RL_GBUFFER_INSTANCES(extern RL_K_MOTION)

// ---------------------------------------------------------------------------
// The temporal accumulation (RaylibAMD_TemporalAccumulate, statements T7 and T8; rl_temporal.hip).  Planes of width * height records: this frame's colour, hit
// and motion (float4 each), the history's colour, hit (float4) and length (float) -- all three null on the first frame --, and the two outputs.
struct DTemporal {
	uint32_t width, height, cellsX, numCells;
	float depthTolerance, maxLength;
	const float4 *colour, *hit, *motion;
	const float4 *histColour, *histHit; const float* histLength;
	float4* outColour; float* outLength;
};
__global__ void __launch_bounds__(RL_BLOCK) k_temporal(const DTemporal);
// ... with the luminance moments beside it (RaylibAMD_TemporalAccumulateMoments, statements S1 and S2): the history's moments (null with the other three) and
// the output's, two floats per pixel, 8-byte aligned
__global__ void __launch_bounds__(RL_BLOCK) k_temporal_moments(const DTemporal, const float2* __restrict__, float2* __restrict__);

// ---------------------------------------------------------------------------
// The variance-guided filter (RaylibAMD_FilterVariance, statements S3 to S7; rl_variance.hip, arithmetic of rl_variance.h).  pack: colour, hit (float4 each) and
// surface (11 words per pixel) of `pixels` pixels -> guides, values.  variance: guides, moments (2 floats per pixel), length, W, H, the constants; writes
// values[].var.  iter: values in, guides, W, H, the step, the constants, values out (LAST: not written), the caller's colour and variance planes (LAST only;
// the variance plane may be null).  pack takes ceil(pixels / RL_BLOCK) workgroups, the other two one per 16 x 16 tile, row-major.
__global__ void __launch_bounds__(RL_BLOCK) k_vf_pack(const float4* __restrict__, const float4* __restrict__, const float* __restrict__, uint32_t, VfGuide* __restrict__,
                                                      VfValue* __restrict__);
__global__ void __launch_bounds__(RL_BLOCK) k_vf_variance(const VfGuide* __restrict__, const float* __restrict__, const float* __restrict__, uint32_t, uint32_t, const VfConst,
                                                          VfValue*);
#define RL_VF_ITER_ARGS const VfValue* __restrict__, const VfGuide* __restrict__, uint32_t, uint32_t, int32_t, const VfConst, VfValue* __restrict__, float4* __restrict__, float* __restrict__
template <bool LAST> __global__ void __launch_bounds__(RL_BLOCK) k_vf_iter(RL_VF_ITER_ARGS);
extern template __global__ void k_vf_iter<false>(RL_VF_ITER_ARGS);
extern template __global__ void k_vf_iter<true>(RL_VF_ITER_ARGS);

// ---------------------------------------------------------------------------
// The ordered multi-hit ray queries (RaylibAMD_TraceRaysAll; rl_k_multihit.inl)
#define RL_MAX_HITS 16   /* RAYLIB_AMD_MAX_HITS */
// TREE: 2 the binary tree (S.nodes), 8 the 8-wide tree (S.nodes8).  STACK: as k_query's.  COUNT: outCount[i] = every accepted triangle of ray i's interval (the walk
// then never prunes with its K-th key).  rays: as k_query's.  maxHits: 1 .. RL_MAX_HITS, and the launch carries 2 * maxHits * RL_BLOCK words of dynamic LDS
// (the lanes' lists).  outHits: n rows of maxHits DQueryHit.  outCount: n words (COUNT) or null.  slotIndex, rayCounter, counters: as k_query's.
#define RL_QUERY_ALL_ARGS const DSceneView, const float4* __restrict__, uint32_t, uint32_t, float4* __restrict__, uint32_t* __restrict__, const int32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int STACK, bool COUNT> __global__ void __launch_bounds__(RL_BLOCK) k_query_all(RL_QUERY_ALL_ARGS);
// The instances rl_rt_rays.hip QueryAllKernelOf selects from: (TREE, STACK, COUNT)
#define RL_QUERY_ALL_INSTANCES_C(X, C) X(2, 32, C) X(2, 64, C) X(8, 2 * RL_POOL8_MAXLEVELS, C)
#define RL_QUERY_ALL_INSTANCES(X) RL_QUERY_ALL_INSTANCES_C(X, false) RL_QUERY_ALL_INSTANCES_C(X, true)
#define RL_K_QUERY_ALL(a, b, c) template __global__ void k_query_all<a, b, c>(RL_QUERY_ALL_ARGS);
RL_QUERY_ALL_INSTANCES(extern RL_K_QUERY_ALL)

// ---------------------------------------------------------------------------
// The nearest-point queries (RaylibAMD_NearestPoints; rl_k_nearest.inl, arithmetic of rl_nearest.h)
enum { RL_NK_WITHIN = 0, RL_NK_CLOSEST = 1 };   // RAYLIB_AMD_NEAREST_*
struct DNearestHit { float dist2; int32_t prim; float b1, b2; };   // RaylibAMDNearestHit
// TREE: 2 the binary tree (S.nodes), 4 the grid nodes (S.nodes4).  STACK: the walk's stack.  points: n float4 (pos, maxDist).  out: uint32_t (WITHIN) or
// DNearestHit (CLOSEST) per point.  slotIndex: triangle slot -> export index (null: the identity).  counters: CNT_RAYS (points), CNT_NODES, CNT_TRIS sums, or null.
#define RL_NEAREST_ARGS const DSceneView, const float4* __restrict__, uint32_t, void* __restrict__, const int32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int KIND, int STACK> __global__ void __launch_bounds__(RL_BLOCK) k_nearest(RL_NEAREST_ARGS);
// The instances rl_rt_rays.hip NearestKernelOfKind selects from: (TREE, KIND, STACK)
#define RL_NEAREST_INSTANCES_K(X, K) X(2, K, 32) X(2, K, 64) X(4, K, 32) X(4, K, 64)
#define RL_NEAREST_INSTANCES(X) RL_NEAREST_INSTANCES_K(X, 0) RL_NEAREST_INSTANCES_K(X, 1)
#define RL_K_NEAREST(a, b, c) template __global__ void k_nearest<a, b, c>(RL_NEAREST_ARGS);
RL_NEAREST_INSTANCES(extern RL_K_NEAREST)
// The K nearest triangles and the count in range (RaylibAMD_NearestPointsAll; rl_k_nearest_all.inl, the same arithmetic)
#define RL_MAX_NEAREST 16   /* RAYLIB_AMD_MAX_NEAREST */
// TREE, STACK, points, slotIndex, counters: as k_nearest's.  COUNT: outCount[i] = every triangle within maxDist of point i (the walk then never prunes with its
// K-th key).  maxHits: 1 .. RL_MAX_NEAREST, and the launch carries 2 * maxHits * RL_BLOCK words of dynamic LDS (the lanes' lists).  outHits: n rows of maxHits
// DNearestHit.  outCount: n words (COUNT) or null.
#define RL_NEAREST_ALL_ARGS const DSceneView, const float4* __restrict__, uint32_t, uint32_t, float4* __restrict__, uint32_t* __restrict__, const int32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int STACK, bool COUNT> __global__ void __launch_bounds__(RL_BLOCK) k_nearest_all(RL_NEAREST_ALL_ARGS);
// The instances rl_rt_rays.hip NearestAllKernelOf selects from: (TREE, STACK, COUNT)
#define RL_NEAREST_ALL_INSTANCES_C(X, C) X(2, 32, C) X(2, 64, C) X(4, 32, C) X(4, 64, C)
#define RL_NEAREST_ALL_INSTANCES(X) RL_NEAREST_ALL_INSTANCES_C(X, false) RL_NEAREST_ALL_INSTANCES_C(X, true)
#define RL_K_NEAREST_ALL(a, b, c) template __global__ void k_nearest_all<a, b, c>(RL_NEAREST_ALL_ARGS);
RL_NEAREST_ALL_INSTANCES(extern RL_K_NEAREST_ALL)

// ---------------------------------------------------------------------------
// The swept-sphere queries (RaylibAMD_SweepSpheres; rl_k_sweep.inl, arithmetic of rl_sweep.h)
enum { RL_SK_ANY = 0, RL_SK_CLOSEST = 1 };   // RAYLIB_AMD_SWEEP_*
struct DSweepHit { float t; int32_t prim; int32_t feature; uint32_t reserved0; float point[3]; uint32_t reserved1; };   // RaylibAMDSweepHit
// TREE: 2 the binary tree (S.nodes), 4 the grid nodes (S.nodes4).  STACK: the walk's stack.  queries: n records of two float4 (origin, radius | delta, a word
// that is not read).  out: uint32_t (ANY) or DSweepHit (CLOSEST, two float4 stores) per query.  slotIndex, counters: as k_nearest's.
#define RL_SWEEP_ARGS const DSceneView, const float4* __restrict__, uint32_t, void* __restrict__, const int32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int KIND, int STACK> __global__ void __launch_bounds__(RL_BLOCK) k_sweep(RL_SWEEP_ARGS);
// The instances rl_rt_rays.hip SweepKernelOfKind selects from: (TREE, KIND, STACK)
#define RL_SWEEP_INSTANCES_K(X, K) X(2, K, 32) X(2, K, 64) X(4, K, 32) X(4, K, 64)
#define RL_SWEEP_INSTANCES(X) RL_SWEEP_INSTANCES_K(X, 0) RL_SWEEP_INSTANCES_K(X, 1)
#define RL_K_SWEEP(a, b, c) template __global__ void k_sweep<a, b, c>(RL_SWEEP_ARGS);
RL_SWEEP_INSTANCES(extern RL_K_SWEEP)

// ---------------------------------------------------------------------------
// The triangle-overlap queries (RaylibAMD_OverlapTriangles; rl_k_overlap.inl, arithmetic of rl_overlap.h)
enum { RL_OK_ANY = 0, RL_OK_LIST = 1 };   // RAYLIB_AMD_OVERLAP_*
#define RL_OVERLAP_SKIP_SHARED 1u         /* RAYLIB_AMD_OVERLAP_SKIP_SHARED */
#define RL_MAX_OVERLAPS 16                /* RAYLIB_AMD_MAX_OVERLAPS */
// TREE: 2 the binary tree (S.nodes), 4 the grid nodes (S.nodes4).  STACK: the walk's stack.  queries: n records of three float4 (a vertex and a word that is not
// read, each).  flags: RL_OVERLAP_SKIP_SHARED or 0.  maxHits: 1 .. RL_MAX_OVERLAPS for LIST, and the launch then carries maxHits * RL_BLOCK words of dynamic LDS
// (the lanes' lists); not read for ANY.  out: uint32_t per query (ANY) or a row of maxHits int32_t (LIST).  outCount: n words or null (LIST).  slotIndex:
// triangle slot -> export index (null: the identity).  counters: CNT_RAYS (queries), CNT_NODES, CNT_TRIS sums, or null.
#define RL_OVERLAP_ARGS const DSceneView, const float4* __restrict__, uint32_t, uint32_t, uint32_t, void* __restrict__, uint32_t* __restrict__, const int32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int KIND, int STACK> __global__ void __launch_bounds__(RL_BLOCK) k_overlap(RL_OVERLAP_ARGS);
// The instances rl_rt_rays.hip OverlapKernelOfKind selects from: (TREE, KIND, STACK)
#define RL_OVERLAP_INSTANCES_K(X, K) X(2, K, 32) X(2, K, 64) X(4, K, 32) X(4, K, 64)
#define RL_OVERLAP_INSTANCES(X) RL_OVERLAP_INSTANCES_K(X, 0) RL_OVERLAP_INSTANCES_K(X, 1)
#define RL_K_OVERLAP(a, b, c) template __global__ void k_overlap<a, b, c>(RL_OVERLAP_ARGS);
RL_OVERLAP_INSTANCES(extern RL_K_OVERLAP)
// The contacts kind (RaylibAMD_OverlapContacts; statements C1 to C6, rl_contact.h): k_overlap's text as LIST (rl_k_overlap.inl, its second pass), and at write-out a 32-byte record per held entry.
// Two more arguments -- outContact: n * maxHits records of two float4, 16-byte aligned; exportSlot: export index -> triangle slot, the inverse of slotIndex
// (null: the identity) -- so it is a kernel of its own name and the eight instances above keep their arguments.  The same dynamic LDS as LIST.
#define RL_OVERLAP_CONTACTS_ARGS RL_OVERLAP_ARGS, float4* __restrict__, const int32_t* __restrict__
template <int TREE, int STACK> __global__ void __launch_bounds__(RL_BLOCK) k_overlap_contacts(RL_OVERLAP_CONTACTS_ARGS);
#define RL_OVERLAP_CONTACTS_INSTANCES(X) X(2, 32) X(2, 64) X(4, 32) X(4, 64)
#define RL_K_OVERLAP_CONTACTS(a, b) template __global__ void k_overlap_contacts<a, b>(RL_OVERLAP_CONTACTS_ARGS);
RL_OVERLAP_CONTACTS_INSTANCES(extern RL_K_OVERLAP_CONTACTS)

// ---------------------------------------------------------------------------
// The oriented-box range queries (RaylibAMD_OverlapBoxes; rl_k_overlap_box.inl, arithmetic of rl_box.h)
enum { RL_BK_ANY = 0, RL_BK_LIST = 1, RL_BK_MARK = 2 };   // RAYLIB_AMD_BOX_*
// TREE, STACK: as k_overlap's.  queries: n records of four float4 (the centre and a word that is not read; each axis with its half extent).  maxHits:
// 1 .. RL_MAX_OVERLAPS for LIST, and the launch then carries maxHits * RL_BLOCK words of dynamic LDS (the lanes' lists); not read for ANY and MARK.  out: uint32_t
// per query (ANY), a row of maxHits int32_t (LIST), or the call's mask of (numTriangles + 31) / 32 words, cleared before the launch (MARK).  outCount: n words or
// null (LIST).  slotIndex: triangle slot -> export index (null: the identity); LIST and MARK read it.  counters: CNT_RAYS (queries), CNT_NODES, CNT_TRIS sums, or null.
#define RL_OVERLAP_BOX_ARGS const DSceneView, const float4* __restrict__, uint32_t, uint32_t, void* __restrict__, uint32_t* __restrict__, const int32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int KIND, int STACK> __global__ void __launch_bounds__(RL_BLOCK) k_overlap_box(RL_OVERLAP_BOX_ARGS);
// The instances rl_rt_rays.hip OverlapBoxKernelOfKind selects from: (TREE, KIND, STACK)
#define RL_OVERLAP_BOX_INSTANCES(X) RL_OVERLAP_INSTANCES_K(X, 0) RL_OVERLAP_INSTANCES_K(X, 1) RL_OVERLAP_INSTANCES_K(X, 2)
#define RL_K_OVERLAP_BOX(a, b, c) template __global__ void k_overlap_box<a, b, c>(RL_OVERLAP_BOX_ARGS);
RL_OVERLAP_BOX_INSTANCES(extern RL_K_OVERLAP_BOX)

// ---------------------------------------------------------------------------
// Distance-field bakes (RaylibAMD_BakeDistanceField; rl_k_sdf.inl, statements V1 to V7 of include/raylib_amd.h)
// The grid and the bit volumes of the sign axes.  axes: bit a set when axis a's rows are traced and its inside bits read.  The rows of a launch are numbered
// axis by axis: axis a's end at rowEnd[a] (an axis not traced ends where its predecessor does); row r of axis x is (j, k) -> k * ny + j, of y (i, k) -> k * nx + i,
// of z (i, j) -> j * nx + i.  Row r of axis a owns words[a] = ceil((dims[a] + 1) / 32) words from word wordBase[a] + r * words[a]: toggle bits 1 .. dims[a]
// behind k_sdf_rows, inside bits 0 .. dims[a] - 1 behind k_sdf_parity.
struct DSdfGrid { float origin[3], spacing[3]; uint32_t dims[3]; float maxDist; uint32_t axes, rowEnd[3], words[3]; unsigned long long wordBase[3]; };
// TREE: 2 the binary tree (S.nodes), 8 the 8-wide tree (S.nodes8).  STACK: as k_query's.  n: the launch's rows.  bits: the zeroed volumes.  rowCounter,
// counters: as k_query's.
#define RL_SDF_ROWS_ARGS const DSceneView, const DSdfGrid, uint32_t, uint32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int STACK> __global__ void __launch_bounds__(RL_BLOCK) k_sdf_rows(RL_SDF_ROWS_ARGS);
#define RL_SDF_ROWS_INSTANCES(X) X(2, 32) X(2, 64) X(8, 2 * RL_POOL8_MAXLEVELS)
#define RL_K_SDF_ROWS(a, b) template __global__ void k_sdf_rows<a, b>(RL_SDF_ROWS_ARGS);
RL_SDF_ROWS_INSTANCES(extern RL_K_SDF_ROWS)
// one thread per row of the launch (n rows)
__global__ void __launch_bounds__(RL_BLOCK) k_sdf_parity(const DSdfGrid, uint32_t, uint32_t* __restrict__);
// TREE: 2 the binary tree, 4 the grid nodes.  STACK: the walk's stack.  SIGNED: the value's sign comes from the volumes of G.axes (bits).  outDist, outPrim
// (may be null): a word per voxel, voxel (i, j, k) at (k * ny + j) * nx + i.  slotIndex, counters: as k_nearest's.  brickCounter: the next 4 x 4 x 4 brick.
#define RL_SDF_DIST_ARGS const DSceneView, const DSdfGrid, float* __restrict__, int32_t* __restrict__, const uint32_t* __restrict__, const int32_t* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int STACK, bool SIGNED> __global__ void __launch_bounds__(RL_BLOCK) k_sdf_dist(RL_SDF_DIST_ARGS);
#define RL_SDF_DIST_INSTANCES_S(X, S) X(2, 32, S) X(2, 64, S) X(4, 32, S) X(4, 64, S)
#define RL_SDF_DIST_INSTANCES(X) RL_SDF_DIST_INSTANCES_S(X, false) RL_SDF_DIST_INSTANCES_S(X, true)
#define RL_K_SDF_DIST(a, b, c) template __global__ void k_sdf_dist<a, b, c>(RL_SDF_DIST_ARGS);
RL_SDF_DIST_INSTANCES(extern RL_K_SDF_DIST)

// ---------------------------------------------------------------------------
// Path-traced radiance along caller rays (RaylibAMD_TraceRadiance; rl_k_radiance.inl)
// What RaylibAMDRadianceParams and the launch say: the seed mixed once (raylib_rng_mix64), the path stack's stride in lanes (the grid's size)
struct DRadianceParams { unsigned long long seedMixed; int32_t maxPathLength; float rayTMin; uint32_t sampleFirst, sampleCount, skipDraws, stackStride; float timeMin, timeMax; };
// k_gather's generator: how the twin of rl_k_radiance.inl makes a job's ray from the caller's point
enum { RL_GEN_HEMISPHERE = 1, RL_GEN_SPHERE = 2 };   // the gather kinds + 1 (RAYLIB_AMD_GATHER_IRRADIANCE, RAYLIB_AMD_GATHER_SH9); k_radiance, whose rays are the caller's, has no generator
// One launch of a gather: job j is sample sampleBase + j / numPoints of point pointFirst + j % numPoints
struct DGatherJobs { uint32_t pointFirst, numPoints, sampleBase; };
// TREE: 2 the binary tree (S.nodes), 4 the grid nodes (S.nodes4).  STACK: the walk's stack.  PRIMS: the scene holds spheres or cubes (binary tree only).
// rays: n records of two float4 (org, time | dir, stream).  out: n float4.  pathStack: [maxPathLength][stackStride] records of 2 float4, as k_trace's.
// counters: CNT_* sums, or null.
#define RL_RADIANCE_ARGS const DSceneView, const SkyRot, const DRadianceParams, const float4* __restrict__, uint32_t, float4* __restrict__, float* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int STACK, bool PRIMS>
__global__ void __launch_bounds__(RL_BLOCK, (STACK <= 32 ? RL_TRACE_MIN_WAVES : 2)) k_radiance(RL_RADIANCE_ARGS);
// The instances rl_rt_rays.hip RadianceKernelFor selects from: (TREE, STACK, PRIMS)
#define RL_RADIANCE_INSTANCES(X) X(2, 32, false) X(2, 32, true) X(2, 64, false) X(2, 64, true) X(4, 32, false) X(4, 64, false)
#define RL_K_RADIANCE(a, b, c) template __global__ void k_radiance<a, b, c>(RL_RADIANCE_ARGS);
RL_RADIANCE_INSTANCES(extern RL_K_RADIANCE)

// ---------------------------------------------------------------------------
// Irradiance and SH probes gathered at caller points (RaylibAMD_Gather; rl_k_radiance.inl, rl_gather.hip)
// points: the call's records of two float4 (pos, time | normal, stream).  n: the launch's jobs.  samples: the launch's sample buffer, slot j = job j: one float4
// (the sample's value) for the hemisphere; two planes of n float4 for the sphere (L, then Wi).
#define RL_GATHER_ARGS const DSceneView, const SkyRot, const DRadianceParams, const float4* __restrict__, uint32_t, const DGatherJobs, float4* __restrict__, float* __restrict__, unsigned int* __restrict__, unsigned long long* __restrict__
template <int TREE, int STACK, bool PRIMS, int GEN>
__global__ void __launch_bounds__(RL_BLOCK, (STACK <= 32 ? RL_TRACE_MIN_WAVES : 2)) k_gather(RL_GATHER_ARGS);
// The instances rl_rt_rays.hip GatherKernelOfKind selects from: k_radiance's (TREE, STACK, PRIMS), once per generator
#define RL_GATHER_INSTANCES_G(X, G) X(2, 32, false, G) X(2, 32, true, G) X(2, 64, false, G) X(2, 64, true, G) X(4, 32, false, G) X(4, 64, false, G)
#define RL_GATHER_INSTANCES(X) RL_GATHER_INSTANCES_G(X, RL_GEN_HEMISPHERE) RL_GATHER_INSTANCES_G(X, RL_GEN_SPHERE)
#define RL_K_GATHER(a, b, c, d) template __global__ void k_gather<a, b, c, d>(RL_GATHER_ARGS);
RL_GATHER_INSTANCES(extern RL_K_GATHER)
// Folds a launch's sample values into per-point sums in sample order, one thread per point (GEN as above).  samples: as k_gather wrote them, numPoints x
// numSamples slots.  acc: 3 (hemisphere) or 27 (sphere) planes of numPoints floats, read unless `first`, written unless `last`.  out: the call's output at the
// launch's first point; written when `last`: sum * rcp1_(sampleCount) * the solid angle.
#define RL_GATHER_RESOLVE_ARGS const float4* __restrict__, uint32_t, uint32_t, float* __restrict__, float* __restrict__, int, int, uint32_t
template <int GEN> __global__ void __launch_bounds__(RL_BLOCK) k_gather_resolve(RL_GATHER_RESOLVE_ARGS);
extern template __global__ void k_gather_resolve<RL_GEN_HEMISPHERE>(RL_GATHER_RESOLVE_ARGS);
extern template __global__ void k_gather_resolve<RL_GEN_SPHERE>(RL_GATHER_RESOLVE_ARGS);

// ---------------------------------------------------------------------------
// Adaptive gather (RaylibAMD_GatherAdaptive, statements A1 to A5; rl_gather_adaptive.hip)
// What a call keeps on the device, indexed by the point's index in the call (its "original" index): the running sums in sample order (3 or 27 planes of
// numPoints floats), the moments of y, and whether the point has stopped -- all cleared when the call begins -- with the rule's parameters.
struct GatherAdaptiveState {
	float* sum;
	float* s1;
	float* s2;
	uint8_t* stopped;
	uint32_t numPoints, cap;
	float threshold;
	uint32_t minSamples;
};
// k_gather_resolve for a launch of a pass: slot p of the launch is the point live[pointFirst + p] (live null: pointFirst + p).  decide: the pass's last sample
// range -- the points then hold samplesNow samples; one that stops by A3 writes out / outSamples (may be null) at its original index and sets its flag.
#define RL_GATHER_ADAPTIVE_RESOLVE_ARGS const float4* __restrict__, uint32_t, uint32_t, const uint32_t* __restrict__, uint32_t, const GatherAdaptiveState, int, uint32_t, float* __restrict__, uint32_t* __restrict__
template <int GEN> __global__ void __launch_bounds__(RL_BLOCK) k_gather_adaptive_resolve(RL_GATHER_ADAPTIVE_RESOLVE_ARGS);
extern template __global__ void k_gather_adaptive_resolve<RL_GEN_HEMISPHERE>(RL_GATHER_ADAPTIVE_RESOLVE_ARGS);
extern template __global__ void k_gather_adaptive_resolve<RL_GEN_SPHERE>(RL_GATHER_ADAPTIVE_RESOLVE_ARGS);
// The ordered compaction of the live set behind a pass, three launches: count (a workgroup per tile of the list: blockCounts[tile] = the entries it keeps), scan
// (one workgroup: the counts scanned in place, the total into blockCounts[numTiles] and *count), move (a workgroup per tile: the kept entries of live -- null: the
// identity -- into outLive, ascending as they were, and each one's record from slot i of points into outPoints).  blockCounts: numTiles + 1 words.
#define RL_GATHER_COMPACT_PER 8
#define RL_GATHER_COMPACT_TILE (RL_BLOCK * RL_GATHER_COMPACT_PER)
#define RL_GATHER_COMPACT_SCAN_BLOCK 1024
__global__ void __launch_bounds__(RL_BLOCK)
k_gather_compact_count(const uint32_t* __restrict__ live, const uint8_t* __restrict__ stopped, uint32_t numLive, uint32_t* __restrict__ blockCounts);
__global__ void __launch_bounds__(RL_GATHER_COMPACT_SCAN_BLOCK) k_gather_compact_scan(uint32_t* __restrict__ blockCounts, uint32_t numTiles, uint32_t* __restrict__ count);
__global__ void __launch_bounds__(RL_BLOCK)
k_gather_compact_move(const uint32_t* __restrict__ live, const uint8_t* __restrict__ stopped, uint32_t numLive, const uint32_t* __restrict__ blockCounts,
                      const float4* __restrict__ points, uint32_t* __restrict__ outLive, float4* __restrict__ outPoints);
// a bake's per-point sample counts into the atlas through the scanned ranks (k_lm_scatter's rule): 0 where no point is
__global__ void __launch_bounds__(RL_BLOCK)
k_gather_scatter_counts(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ counts, uint32_t numTexels, uint32_t* __restrict__ atlas);

// ---------------------------------------------------------------------------
// Lightmaps (RaylibAMD_BakeLightmap; rl_lightmap.hip, arithmetic of rl_lightmap.h).  tris: the range's records of 26 floats (rl_host.h HostTriangle); uv: six
// floats per triangle, or null for the records' own.  A triangle's raster record: its snapped corners and the rectangle of texel centres in its box (rw 0: skipped).
struct DLmTri { int32_t X[3], Y[3]; uint32_t lo; uint32_t rw; };   // lo: the rectangle's first column | its first row << 16
static_assert(sizeof(DLmTri) == 32, "raster record");
// one thread per triangle: the record, and the rectangle's texel count into counts[k]
__global__ void __launch_bounds__(RL_BLOCK)
k_lm_setup(const float* __restrict__ tris, const float* __restrict__ uv, uint32_t numTris, int32_t width, int32_t height, DLmTri* __restrict__ rec, unsigned long long* __restrict__ counts);
// one thread per (triangle, rectangle texel) pair base + i, i < pairs: the triangle by binary search in the scanned counts offs[0 .. numTris], statement 3, atomicMin into owner
__global__ void __launch_bounds__(RL_BLOCK)
k_lm_cover(const DLmTri* __restrict__ rec, const unsigned long long* __restrict__ offs, uint32_t numTris, unsigned long long base, uint32_t pairs, int32_t width, uint32_t numTexels, uint32_t* __restrict__ owner);
// one thread per texel, statements 3 to 5 from the owner.  WRITE false: rank[i] = the texel has a point.  WRITE true, rank scanned (rank[numTexels] the count): the
// point of a texel whose rank is below capacity into points[rank] (two float4) and its index into texel[rank] (may be null)
template <bool WRITE> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_points(const DLmTri* __restrict__ rec, const float* __restrict__ tris, const uint32_t* __restrict__ owner, uint32_t* __restrict__ rank, int32_t width, uint32_t numTexels,
            float time, float4* __restrict__ points, uint32_t* __restrict__ texel, unsigned long long capacity);
extern template __global__ void k_lm_points<false>(const DLmTri* __restrict__, const float* __restrict__, const uint32_t* __restrict__, uint32_t* __restrict__, int32_t, uint32_t, float, float4* __restrict__, uint32_t* __restrict__, unsigned long long);
extern template __global__ void k_lm_points<true>(const DLmTri* __restrict__, const float* __restrict__, const uint32_t* __restrict__, uint32_t* __restrict__, int32_t, uint32_t, float, float4* __restrict__, uint32_t* __restrict__, unsigned long long);
// The exclusive scan of n values in place, data[n] receiving the total, as reduce, scan, add over tiles of RL_SCAN_TILE values: k_lm_scan_reduce (a block per tile)
// leaves the tiles' sums, k_lm_scan_sums (one block) scans them in place with sums[numTiles] the total, k_lm_scan_add (a block per tile) scans each tile from its sum.
#define RL_SCAN_PER 8
#define RL_SCAN_TILE (RL_BLOCK * RL_SCAN_PER)
#define RL_SCAN_SUMS_BLOCK 1024
template <typename T> __global__ void __launch_bounds__(RL_BLOCK) k_lm_scan_reduce(const T* __restrict__ data, unsigned long long n, T* __restrict__ sums);
template <typename T> __global__ void __launch_bounds__(RL_SCAN_SUMS_BLOCK) k_lm_scan_sums(T* __restrict__ sums, uint32_t numTiles);
template <typename T> __global__ void __launch_bounds__(RL_BLOCK) k_lm_scan_add(T* __restrict__ data, unsigned long long n, const T* __restrict__ sums, uint32_t numTiles);
#define RL_LM_SCAN_INSTANCES(X, T) \
	X template __global__ void k_lm_scan_reduce<T>(const T* __restrict__, unsigned long long, T* __restrict__); \
	X template __global__ void k_lm_scan_sums<T>(T* __restrict__, uint32_t); \
	X template __global__ void k_lm_scan_add<T>(T* __restrict__, unsigned long long, const T* __restrict__, uint32_t);
RL_LM_SCAN_INSTANCES(extern, uint32_t)
RL_LM_SCAN_INSTANCES(extern, unsigned long long)
// statement 8, one thread per texel: a texel with a point (rank[i + 1] != rank[i]) takes values[rank[i]] (C floats) and coverage 1, every other +0 and 0
template <int C> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_scatter(const uint32_t* __restrict__ rank, const float* __restrict__ values, uint32_t numTexels, float* __restrict__ atlas, uint8_t* __restrict__ coverage);
// statement 9, one pass, one thread per texel: src -> dst
template <int C> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_dilate(const float* __restrict__ src, const uint8_t* __restrict__ srcCov, float* __restrict__ dst, uint8_t* __restrict__ dstCov, int32_t width, int32_t height, int32_t pass);
#define RL_LM_ATLAS_INSTANCES(X, C) \
	X template __global__ void k_lm_scatter<C>(const uint32_t* __restrict__, const float* __restrict__, uint32_t, float* __restrict__, uint8_t* __restrict__); \
	X template __global__ void k_lm_dilate<C>(const float* __restrict__, const uint8_t* __restrict__, float* __restrict__, uint8_t* __restrict__, int32_t, int32_t, int32_t);
RL_LM_ATLAS_INSTANCES(extern, 4)
RL_LM_ATLAS_INSTANCES(extern, 27)
// The atlas filter (RaylibAMD_BakeLightmapFiltered, statement F; rl_lightmap_filter.hip), on the points in compacted form, in front of the scatter.
// One iteration, one thread per point i < count: its texel is texel[i], a tap's point is found through rank (scanned: a texel has a point when rank[q + 1] !=
// rank[q]), src -> dst (count x C floats each).  prep: the first iteration, which reads a value that is not finite as 0.
template <int C> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_filter(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ texel, const float4* __restrict__ points, const float* __restrict__ src, float* __restrict__ dst,
            uint32_t count, int32_t width, int32_t height, int32_t step, float invC, float invN, float invP, int32_t prep);
// RaylibAMD_FilterLightmap: one thread per texel, a texel with a point hands its C floats of `atlas` to values[rank[i]]
template <int C> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_take(const uint32_t* __restrict__ rank, const float* __restrict__ atlas, uint32_t numTexels, float* __restrict__ values);
#define RL_LM_FILTER_INSTANCES(X, C) \
	X template __global__ void k_lm_filter<C>(const uint32_t* __restrict__, const uint32_t* __restrict__, const float4* __restrict__, const float* __restrict__, float* __restrict__, \
	                                          uint32_t, int32_t, int32_t, int32_t, float, float, float, int32_t); \
	X template __global__ void k_lm_take<C>(const uint32_t* __restrict__, const float* __restrict__, uint32_t, float* __restrict__);
RL_LM_FILTER_INSTANCES(extern, 4)
RL_LM_FILTER_INSTANCES(extern, 27)

// ---------------------------------------------------------------------------
// A move of a finalized scene's triangles and the refit of its trees (rl_refit.hip, bodies in rl_k_refit.inl; launched by rl_rt_move.hip): no walk, no shading.
// The status block of a scene's moves: word RL_MOVE_NONFINITE is raised by k_move_scan when a value is not finite (k_move_records then writes nothing), word
// RL_MOVE_BAD_DENOM counts the triangles whose divisor lies outside [2^-62, 2^125] (none: DSceneView::fastBary may stand).
enum { RL_MOVE_NONFINITE = 0, RL_MOVE_BAD_DENOM = 1, RL_MOVE_WORDS = 4 };
__global__ void __launch_bounds__(RL_BLOCK) k_move_count(const DTriIsect* __restrict__ isect, uint32_t numTris, uint32_t* __restrict__ status);
__global__ void __launch_bounds__(RL_BLOCK) k_move_scan(const float* __restrict__ positions, const float* __restrict__ normals, uint32_t floats, uint32_t* __restrict__ status);
__global__ void __launch_bounds__(RL_BLOCK)
k_move_records(DTriIsect* __restrict__ isect, DTriShade* __restrict__ shade, const int32_t* __restrict__ slotOf, uint32_t first, uint32_t count, uint32_t numTris,
               const float* __restrict__ positions, const float* __restrict__ normals, uint32_t* __restrict__ status);
__global__ void __launch_bounds__(RL_BLOCK)
k_refit_level(DNode* nodes, const DTriIsect* __restrict__ isect, const uint32_t* __restrict__ levelNodes, uint32_t count, uint32_t numNodes, uint32_t numTris);
__global__ void __launch_bounds__(RL_BLOCK)
k_refit_wide4(const DNode* __restrict__ nodes, uint32_t numNodes, const int32_t* __restrict__ boxOf, DNode4* __restrict__ nodes4f, DNode4Q* __restrict__ nodes4q, uint32_t count);
__global__ void __launch_bounds__(RL_BLOCK)
k_refit_wide8(const DNode* __restrict__ nodes, uint32_t numNodes, const int32_t* __restrict__ boxOf, DNode8* __restrict__ nodes8, uint32_t count);

// ---------------------------------------------------------------------------
// Test hooks (rl_rt_hooks.hip): single functions of the hot path evaluated on arrays
__global__ void __launch_bounds__(RL_BLOCK) k_eval_scatter(const DSceneView S, int material, const float* __restrict__ in, int n, unsigned long long seed, float* __restrict__ out);
__global__ void __launch_bounds__(RL_BLOCK) k_eval_camera(const DCamera cam, const float* __restrict__ uv, int n, unsigned long long seed, float* __restrict__ out);
__global__ void __launch_bounds__(RL_BLOCK) k_eval_texture(const DSceneView S, int tex, int srgb, const float* __restrict__ uv, int n, float* __restrict__ out);
__global__ void __launch_bounds__(RL_BLOCK) k_eval_math(int fn, const float* __restrict__ x, const float* __restrict__ y, int n, float* __restrict__ out);
__global__ void __launch_bounds__(RL_BLOCK) k_verify_exact_math(int which, unsigned long long* __restrict__ out);
__global__ void __launch_bounds__(RL_BLOCK) k_verify_lazy_refl(uint32_t n, unsigned long long seed, unsigned long long* __restrict__ out);
__global__ void __launch_bounds__(RL_BLOCK) k_verify_lazy_pdf(uint32_t n, unsigned long long seed, unsigned long long* __restrict__ out);
__global__ void __launch_bounds__(RL_BLOCK) k_verify_sampler_ranged(int mode, unsigned long long* __restrict__ out);
__global__ void __launch_bounds__(RL_BLOCK) k_verify_normalize_ranged(int mode, unsigned long long* __restrict__ out);

} // namespace rl
