// Which megakernel instance a render launches, on which tree, and how its job list is laid out: host facts in, plain structs out,
// no HIP calls (rl_plan.cc).  The runtime (rl_rt_*.hip) launches what these say; RaylibAMD_PlanRender exposes them to the tests.
#pragma once

#include "rl_host.h"

namespace rl {

#define RL_POOL_DEFAULT_MIN_TRIS 256u   /* triangles from which the pool schedule is the default (RAYLIB_POOL_MIN_TRIS) */
#define RL_HIT_QUEUE_DEFAULT 1          /* a lazy plan takes the hit-queue form (k_trace_lazy_hitq) unless RAYLIB_HIT_QUEUE=0 */
#define RL_FLOAT_BOX_MAX_TRIS 4096u    /* scenes below this many triangles carry the float-box wide nodes (and the leaf list) on the device */

// The per-render switches of INTEGRATION.md, read from the environment by ReadRenderKnobs() on every render (tests change them between renders).
// A default-constructed RenderKnobs is "nothing set".  -1: not set; the 0 / 1 switches hold atoi(value) != 0.
struct RenderKnobs {
	int pool = -1;                                // RAYLIB_POOL: 0 (k_trace), 2, 3 or 4 (any other value: 0)
	uint32_t poolMinTris = RL_POOL_DEFAULT_MIN_TRIS;   // RAYLIB_POOL_MIN_TRIS
	int poolShortStack = -1;                      // RAYLIB_POOL_SHORT_STACK: 0, 4 (tests: nearly every push overflows) or 1 (any other value)
	int bvh4 = -1, bvh8 = -1;                     // RAYLIB_BVH4, RAYLIB_BVH8
	int ldsScene = -1, leafList = -1, plainKernel = -1;   // RAYLIB_LDS_SCENE, RAYLIB_LEAF_LIST, RAYLIB_PLAIN_KERNEL
	int sampleBatch = 0, sampleBufferGiB = 0;     // RAYLIB_SAMPLE_BATCH, RAYLIB_SAMPLE_BUFFER_GIB (0: not set or not positive)
	int jobChunk = -1;                            // RAYLIB_JOB_CHUNK: max(0, value)
	int jobHeads = 0;                             // RAYLIB_JOB_HEADS: max(1, value); 0: not set
	int guided = 0;                               // RAYLIB_GUIDED
	int blocksPerCU = 0;                          // RAYLIB_BLOCKS_PER_CU (0: not set or not positive)
	int cullCells = 1;                            // RAYLIB_CULL_CELLS (rl_cull.cc reads it for itself; the runtime keys its cached cell lists on it)
	int queryTree = 0;                            // RAYLIB_QUERY_TREE: 2, 4 or 8 (RaylibAMD_TraceRays, RaylibAMD_TraceRadiance, RaylibAMD_Gather; any other value: 0, not set)
	int gatherBatch = 0;                          // RAYLIB_GATHER_BATCH: (point, sample) slots per launch of RaylibAMD_Gather (0: not set or not positive)
	int lazyRefl = -1;                            // RAYLIB_LAZY_REFL
	int hitQueue = -1;                            // RAYLIB_HIT_QUEUE
	long long litList = -1;                       // RAYLIB_LIT_LIST: entries of the lazy instance's lit list (0: every lit path folds in place); -1: not set
	int litMask = -1;                             // RAYLIB_LIT_MASK: 0 keeps every sample stored and k_resolve; 1 takes the lit-sample mask with a sun too
};
RenderKnobs ReadRenderKnobs();

enum PlanTree : int32_t { TREE_NONE = 0, TREE_BVH2 = 1, TREE_BOX4 = 2, TREE_GRID4 = 3, TREE_WIDE8 = 4 };

struct TracePlan {
	bool ok = true;             // false: the BVH is deeper than any traversal stack (logged)
	bool pathTrace = true;      // false: a debug render mode, k_aov<stack, prims> on the BVH2
	int stack = 16;             // the instance's STACK
	bool prims = false;         // spheres or cubes
	int poolK = 0;              // 0: k_trace (one path per lane); K: k_trace_pool with 64 K paths per wave
	int32_t tree = TREE_BVH2;   // what the walk reads (TREE_NONE: the leaf list)
	int lstack = 0;             // pool: entries of the traversal stack in LDS
	int lds = 0;                // k_trace: 0, 1 = the scene in LDS, 2 = the leaf list
	bool plain = false;         // the leaf-list kernel's instance without texture, cut-out and sky code
	bool lazy = false;          // ... and of that, the lazy-reflectance instance (k_trace_lazy or its hit-queue form); the views twin of a lazy plan is the plain instance's
	bool hitQueue = false;      // ... and of that, its hit-queue form (k_trace_lazy_hitq): idle lanes take camera rays that have been traced already
	uint32_t pathsPerWave = 64, treeWidth = 2, nodeBytes = 64;   // RaylibAMDStats
	bool keepNodes4 = true, keepNodes4f = true;   // the launch's view keeps the grid / float-box wide nodes (k_trace tells the tree by which is set)
	int32_t eagerTree = TREE_NONE;   // the wide tree UploadScene puts on the device (TREE_GRID4, TREE_WIDE8 or none): the default plan's
};
// sc is finalized; hasSky: the render has a sky image (sc.sky of non-zero size)
TracePlan PlanTrace(const Scene& sc, const RendererSettings& st, bool hasSky, const RenderKnobs& knobs);
int32_t EagerTree(const Scene& sc);   // = PlanTrace(sc, <a path-traced render>, false, RenderKnobs()).eagerTree

struct LaunchPlan {
	uint32_t batch = 1;         // samples per launch
	uint32_t sampleCount = 0;   // of this launch (from sampleBegin)
	uint64_t jobs = 0;          // numActive * sampleCount * 64
	uint32_t blocks = 1, stackStride = 0, jobChunk = 64, heads = 1, jobsPerHead = 0, guideShift = 0;
};
// One launch of a path-traced render: numActive of the rank's numLocalCells cells are in the job list, samples from sampleBegin; workgroupsPerCU as the occupancy query gave it.
LaunchPlan PlanLaunch(uint32_t numLocalCells, uint32_t numActive, uint32_t spp, uint32_t sampleBegin, int numCUs, int workgroupsPerCU,
                      const TracePlan& trace, const RenderKnobs& knobs);

// Which tree and k_query instance a batch of ray queries walks (RaylibAMD_TraceRays, rl_k_query.inl): the 8-wide tree when the scene carries one of at most
// RL_POOL8_MAXLEVELS levels and has no spheres or cubes; else the grid-4 tree when its worst-case stack fits 64 entries (no spheres or cubes either); else the
// binary tree.  RAYLIB_QUERY_TREE=2|4|8 starts the list lower; a tree the scene lacks falls through to the next one.
struct QueryPlan {
	bool ok = true;             // false: the BVH is deeper than the binary walk's stack (64)
	int32_t tree = TREE_BVH2;   // TREE_BVH2, TREE_GRID4 or TREE_WIDE8
	uint32_t treeWidth = 2, nodeBytes = 64;
	int stack = 32;             // the instance's STACK (the 8-wide tree: words, two per group)
	bool prims = false;         // spheres or cubes
	bool early = false;         // the occlusion query stops at its first accepted candidate
};
QueryPlan PlanQuery(const Scene& sc, int32_t kind, const RenderKnobs& knobs);
// Which tree and k_gbuffer instance a G-buffer walks (RaylibAMD_RenderGBuffer, rl_k_gbuffer.inl): k_gbuffer has an instance per CLOSEST instance of k_query
// and its pixels are the SURFACE query's rays, so this is PlanQuery's answer for that kind.  `early` is false.
QueryPlan PlanGBuffer(const Scene& sc, const RenderKnobs& knobs);
// Which tree and k_query_all instance a batch of ordered multi-hit queries walks (RaylibAMD_TraceRaysAll, rl_k_multihit.inl): the 8-wide tree under PlanQuery's
// conditions, else the binary tree.  There is no grid-4 instance: RAYLIB_QUERY_TREE=4 falls through to the binary tree, =2 selects it, =8 is the default.
// `early` is unused (false).  The scene holds triangles only (the entries refuse spheres and cubes before they plan).
QueryPlan PlanQueryAll(const Scene& sc, const RenderKnobs& knobs);
// Which tree and k_radiance instance a batch of caller rays is path-traced on (RaylibAMD_TraceRadiance, rl_k_radiance.inl): the grid-4 tree when the scene
// carries one, has no spheres or cubes and its worst-case stack fits 64 entries; else the binary tree.  The 8-wide walk is a step walk and not fused with
// shading here: RAYLIB_QUERY_TREE=8 falls through to 4, =2 walks the binary tree.  `early` is unused (false).
QueryPlan PlanRadiance(const Scene& sc, const RenderKnobs& knobs);
// Which tree and k_nearest instance a batch of nearest-point queries walks (RaylibAMD_NearestPoints, rl_k_nearest.inl): the grid-4 tree when the scene carries
// one and its worst-case stack fits 64 entries; else the binary tree.  The walk pushes at most (children - 1) references per level, as the ray walks do, so
// their stack bounds are its bounds.  There is no 8-wide nearest walk: RAYLIB_QUERY_TREE=8 falls through to 4, =2 walks the binary tree.  `early`: the kind is
// WITHIN.  The scene holds triangles only (the entries refuse spheres and cubes before they plan).
QueryPlan PlanNearest(const Scene& sc, int32_t kind, const RenderKnobs& knobs);
// Which tree and k_nearest_all instance a batch of K-nearest queries walks (RaylibAMD_NearestPointsAll, rl_k_nearest_all.inl): what PlanNearest gives CLOSEST --
// the walk and its pushes are the same, so is the stack.  `early` is false.  maxHits and the count choose the launch's list bytes and the COUNT instance, not the plan.
QueryPlan PlanNearestAll(const Scene& sc, const RenderKnobs& knobs);
// Which tree and k_sweep instance a batch of swept-sphere queries walks (RaylibAMD_SweepSpheres, rl_k_sweep.inl): PlanNearest's trees and stack bounds under the
// same switch -- the walk pushes at most (children - 1) references per level, as the point walk does -- with PlanOverlap's default: the grid-4 tree when the
// scene carries one and its worst-case stack fits the 32-deep instance, else the binary tree, which the 298 k-triangle room's sweeps walk in half the time of
// the 64-deep grid instance (measured: profiles/sweep_time.log).  RAYLIB_QUERY_TREE=4 takes the grid-4 tree up to a worst-case stack of 64 entries, =8 falls
// through to 4, =2 walks the binary tree.  `early`: the kind is ANY.  The scene holds triangles only.
QueryPlan PlanSweep(const Scene& sc, int32_t kind, const RenderKnobs& knobs);
// Which trees a distance-field bake walks (RaylibAMD_BakeDistanceField, rl_k_sdf.inl): the distance kernel is k_nearest's CLOSEST walk, so its plan is
// PlanNearest's; the row kernel is k_query_all's counting walk, so its plan is PlanQueryAll's.  One RAYLIB_QUERY_TREE steers both.
struct DistanceFieldPlan { QueryPlan nearest, rows; };
DistanceFieldPlan PlanDistanceField(const Scene& sc, const RenderKnobs& knobs);
// Which tree and k_overlap instance a batch of triangle-overlap queries walks (RaylibAMD_OverlapTriangles, rl_k_overlap.inl): PlanNearest's trees under the same
// switch, with a default of its own: the grid-4 tree when the scene carries one and its worst-case stack fits the 32-deep instance, else the binary tree,
// which the self-intersection pass on the 298 k-triangle room walks faster than the 64-deep grid instance (measured: DESIGN.md section 2).
// RAYLIB_QUERY_TREE=4 takes the grid-4 tree up to a worst-case stack of 64 entries, =8 falls through to 4 (no 8-wide walk), =2 walks the binary tree.  At most
// (children - 1) pushes per level, so the ray walks' stack bounds hold.  `early`: the kind is ANY.  The scene holds triangles
// only (the entries refuse spheres and cubes before they plan).
QueryPlan PlanOverlap(const Scene& sc, int32_t kind, const RenderKnobs& knobs);
// Which tree and k_overlap_box instance a batch of oriented-box queries walks (RaylibAMD_OverlapBoxes, rl_k_overlap_box.inl): PlanOverlap's answer -- the same
// walk, the same pushes, the same switch.  `early`: the kind is ANY (LIST and MARK walk to the end).
QueryPlan PlanOverlapBoxes(const Scene& sc, int32_t kind, const RenderKnobs& knobs);

// How RaylibAMD_Gather cuts n points x sampleCount samples into launches (rl_rt_rays.hip DeviceGather; RaylibAMD_PlanGatherCut): a launch holds at most `slots`
// (point, sample) pairs -- RL_GATHER_SAMPLE_BUDGET over the slot's bytes (16 for IRRADIANCE, 32 for SH9), or RAYLIB_GATHER_BATCH, at most RL_GATHER_MAX_SLOTS.
// While one sample of every point fits, a launch takes all the points and samplesPer samples; otherwise the points are cut into ranges of pointsPer as well, one
// sample per launch.  Launch k of `launches` is sample range k % sampleRanges of point range k / sampleRanges: a point range runs through all its sample ranges
// before the next begins, so one set of running sums serves.  sampleCount may be any uint32_t and n any positive int32_t: the counts and every product are 64-bit.
struct GatherCut { uint32_t pointsPer = 0, samplesPer = 0; uint64_t pointRanges = 0, sampleRanges = 0, launches = 0; };
struct GatherLaunch { uint32_t pointFirst, numPoints, sampleBase, numSamples; bool first, last; };   // first / last: of the point range's sample ranges
GatherCut PlanGatherCut(uint32_t n, uint32_t sampleCount, bool sphere, const RenderKnobs& knobs);   // n, sampleCount >= 1
GatherLaunch GatherLaunchAt(const GatherCut& c, uint32_t n, uint32_t sampleCount, uint64_t k);      // k < c.launches

// Several views of one scene in one launch per sample batch (RaylibAMD_RenderViews): the job list of the batch.  Cell c of view v is batch cell
// v * cellsPerView + c; the list is every view's listed cells, view by view, each view culled on its own (CullCells), a view that is not eligible listing all
// of its cells.  What the kernels add up for a dropped cell is one constant for the whole batch (emptyL: the sun's illuminance or nothing -- CullCells
// drops cells only where the sun ray misses the scene, so the constant depends on the scene alone); a view whose constant would differ lists all its cells.
struct ViewsPlan {
	bool ok = false;                      // false: the job count of a one-sample batch would overflow
	uint32_t cellsPerView = 0, numCells = 0, numActive = 0;
	std::vector<uint32_t> active;         // listed batch cells, ascending
	std::vector<unsigned char> empty;     // per batch cell: dropped
	std::vector<uint32_t> culledPerView;  // cells dropped per view
	uint64_t emptyPixels = 0;             // valid pixels of the dropped cells (per sample)
	float emptyL[3] = { 0, 0, 0 };
	uint32_t raysPerSample = 1;           // of a dropped cell's sample (counters)
	RenderKnobs knobs;                    // the knobs every launch of the batch is planned with: RAYLIB_SAMPLE_BATCH lowered where the job count needs it
	LaunchPlan launch;                    // the first launch
};
ViewsPlan PlanViews(const CullScene& cs, const RendererSettings& st, const DCamera* cameras, uint32_t count, const TracePlan& trace,
                    int numCUs, int workgroupsPerCU, const RenderKnobs& knobs);
// What CullCells needs to know of a finalized scene, for the runtime's renders and the planner hooks alike: its box (the root node's two child boxes; valid for
// triangle scenes with finite coordinates) and its sun
CullScene SceneCullScene(const Scene& sc, bool hasSky);

} // namespace rl
