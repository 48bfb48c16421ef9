// The one place that decides which megakernel instance a render launches, on which tree, and the launch's job layout (rl_plan.h).
// Every measurement behind a default is cited where the default is made; DESIGN.md section 5 has the tables.
#include "rl_plan.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <stdlib.h>

namespace rl {

RenderKnobs ReadRenderKnobs()
{
	RenderKnobs k;
	auto flag = [](const char* name) { const char* e = getenv(name); return e ? (atoi(e) != 0 ? 1 : 0) : -1; };
	if (const char* e = getenv("RAYLIB_POOL")) { const int v = atoi(e); k.pool = (v == 2 || v == 3 || v == 4) ? v : 0; }
	if (const char* e = getenv("RAYLIB_POOL_MIN_TRIS")) k.poolMinTris = (uint32_t)atoi(e);
	if (const char* e = getenv("RAYLIB_POOL_SHORT_STACK")) { const int v = atoi(e); k.poolShortStack = (v == 0 || v == 4) ? v : 1; }
	k.bvh4 = flag("RAYLIB_BVH4"); k.bvh8 = flag("RAYLIB_BVH8");
	k.ldsScene = flag("RAYLIB_LDS_SCENE"); k.leafList = flag("RAYLIB_LEAF_LIST"); k.plainKernel = flag("RAYLIB_PLAIN_KERNEL");
	if (const char* e = getenv("RAYLIB_SAMPLE_BATCH")) k.sampleBatch = std::max(0, atoi(e));
	if (const char* e = getenv("RAYLIB_SAMPLE_BUFFER_GIB")) k.sampleBufferGiB = std::max(0, atoi(e));
	if (const char* e = getenv("RAYLIB_JOB_CHUNK")) k.jobChunk = std::max(0, atoi(e));
	if (const char* e = getenv("RAYLIB_JOB_HEADS")) k.jobHeads = std::max(1, atoi(e));
	if (const char* e = getenv("RAYLIB_GUIDED")) k.guided = atoi(e);
	if (const char* e = getenv("RAYLIB_BLOCKS_PER_CU")) k.blocksPerCU = std::max(0, atoi(e));
	if (const char* e = getenv("RAYLIB_CULL_CELLS")) k.cullCells = atoi(e);
	k.lazyRefl = flag("RAYLIB_LAZY_REFL"); k.hitQueue = flag("RAYLIB_HIT_QUEUE");
	if (const char* e = getenv("RAYLIB_LIT_LIST")) k.litList = std::max(0ll, atoll(e));
	k.litMask = flag("RAYLIB_LIT_MASK");
	if (const char* e = getenv("RAYLIB_QUERY_TREE")) { const int v = atoi(e); k.queryTree = (v == 2 || v == 4 || v == 8) ? v : 0; }
	if (const char* e = getenv("RAYLIB_GATHER_BATCH")) k.gatherBatch = std::max(0, atoi(e));
	return k;
}

namespace {

// the launch's choice; `say`: log what the render should know (only for the plan that is launched)
TracePlan Pick(const Scene& sc, const RendererSettings& st, bool hasSky, const RenderKnobs& k, bool say)
{
	TracePlan p;
	const BVH& b = sc.bvh;
	const size_t ntri = sc.triangles.size();
	p.prims = !sc.spheres.empty() || !sc.cubes.empty();
	if (b.depth > 64) {
		if (say) Log("Raylib_Render: BVH depth %u exceeds the traversal stack (64)", b.depth);
		p.ok = false;
		return p;
	}
	p.stack = (b.depth <= 16 && !p.prims) ? 16 : b.depth <= 32 ? 32 : 64;
	p.pathTrace = st.renderMode == RAYLIB_RENDERMODE_Default;
	if (!p.pathTrace) return p;   // k_aov walks the BVH2
	const bool hasNodes4 = !b.nodes4.empty(), hasNodes8 = !b.nodes8.empty();

	// The pool schedule for triangle scenes from RAYLIB_POOL_MIN_TRIS triangles on, else k_trace (the Cornell class: tens of triangles, shading-bound).
	// Measured crossover (tools/gpu_crossover.py, tessellated rooms at 1080p x 16 spp, pool time / k_trace time): 36 triangles 1.07, 144: 0.97, 324: 0.95,
	// 1296: 0.89, 5184: 0.80, 20736: 0.67.  RAYLIB_POOL=0|2|3|4 overrides.
	const bool poolable = p.stack <= 32 && !p.prims;
	const int poolK = k.pool >= 0 ? k.pool : (poolable && ntri >= k.poolMinTris ? 2 : 0);
	if (poolable && poolK > 0) {
		p.poolK = poolK; p.pathsPerWave = 64u * (uint32_t)poolK;
		// the wide tree: whenever the scene carries one whose worst-case stack fits; RAYLIB_BVH4=0|1 overrides
		if (poolK == 2 && hasNodes4 && b.stackNeed4 <= 64 && k.bvh4 != 0) {
			p.tree = TREE_GRID4; p.treeWidth = 4;
			p.stack = b.stackNeed4 <= 32 ? 32 : 64;
			if (k.poolShortStack == 0) { p.lstack = 32; return p; }
			// the 8-wide tree (0.67 x the steps of the 4-wide one, each 1.4 x as long) when the scene carries one of at most RL_POOL8_MAXLEVELS levels -- a group
			// of hit children per level is all its stack ever holds -- and its rays are expected to take many steps: measured over rooms and colonnades of 1 k ...
			// 10 M triangles (tools/gpu_bvh8_sweep.py, profiles/r04_bvh8_sweep.log) the 8-wide walk loses 2 - 8 % below ~30 expected steps of the 4-wide tree
			// (the builder's sum of node areas over the root's), breaks even between 30 and 42 and wins 3 - 9 % from 59 up.  RAYLIB_BVH8=0|1 overrides.
			const bool want8 = hasNodes8 && (k.bvh8 >= 0 ? k.bvh8 != 0 : b.sahNodes4 >= RL_BVH8_MIN_STEPS);
			if (want8 && b.depth8 <= RL_POOL8_MAXLEVELS) {
				p.tree = TREE_WIDE8; p.treeWidth = 8; p.nodeBytes = (uint32_t)sizeof(DNode8);
				p.stack = 2 * RL_POOL8_MAXLEVELS; p.lstack = RL_POOL8_LSTACK;
				return p;
			}
			if (want8 && say) {   // (a deeper 8-wide tree is not walked, and that is said once per scene)
				static std::atomic<const Scene*> told{ nullptr };
				if (told.exchange(&sc) != &sc) Log("Raylib_Render: the scene's 8-wide tree has %u levels, the pool kernel's stack holds %d: walking the 4-wide tree", b.depth8, (int)RL_POOL8_MAXLEVELS);
			}
			p.lstack = RL_POOL_SHORT_LSTACK;
			return p;
		}
		p.lstack = p.stack;
		if (p.stack == 32 && poolK == 2) {
			if (k.poolShortStack == 4) p.lstack = 4;
			else if (k.poolShortStack >= 0 ? k.poolShortStack != 0 : b.depth <= RL_POOL_SHORT_MAXDEPTH) p.lstack = RL_POOL_SHORT_LSTACK;
		}
		return p;
	}

	// k_trace walks the 4-wide tree too when the scene has one whose worst-case stack fits the instance's LDS stack: on float boxes if the scene carries them
	// (small scenes, where the grid's extra arithmetic buys nothing: Cornell frame 22.8 ms on float boxes, 23.8 ms on the grid), else on the grid nodes
	const bool floatBoxes = hasNodes4 && ntri < RL_FLOAT_BOX_MAX_TRIS;
	const bool wide = !p.prims && hasNodes4 && b.stackNeed4 <= (uint32_t)p.stack && k.bvh4 != 0;
	p.tree = !wide ? TREE_BVH2 : floatBoxes ? TREE_BOX4 : TREE_GRID4;
	p.treeWidth = wide ? 4 : 2;
	p.keepNodes4 = p.tree == TREE_GRID4;
	p.keepNodes4f = p.tree == TREE_BOX4;
	// the whole scene in LDS when it fits the fixed layout (rl_device.h RL_LDS_*); RAYLIB_LDS_SCENE=0 keeps it in global memory
	if (p.stack == 16 && p.tree == TREE_BOX4 && k.ldsScene != 0 && b.nodes4.size() <= RL_LDS_MAXNODES && ntri <= RL_LDS_MAXTRIS && sc.materials.size() <= RL_LDS_MAXMATS) {
		p.lds = 1;
		// ... and a scene of few leaves without a tree (rl_bvh.cc "the leaf list"); RAYLIB_LEAF_LIST=0 walks its BVH4 instead.  Its sortable keys are entry
		// distances, never negative (rl_dev_walk.h TraverseLeafList): not with rayTMin < 0.
		if (!b.leafList.empty() && b.leafList.size() <= RL_LEAFLIST_RECORDS && ntri <= RL_LEAFLIST_MAXTRIS && k.leafList != 0 && st.rayTMin >= 0.0f) {
			p.lds = 2; p.tree = TREE_NONE; p.treeWidth = 0;
			// the instance without the texture, cut-out and sky code computes the same values in the same order for the scenes it takes: those without a texture
			// slot or a cut-out leaf (ScenePlain) rendered without a sky image.  RAYLIB_PLAIN_KERNEL=0 keeps the general instance.
			p.plain = !hasSky && k.plainKernel != 0 && ScenePlain(sc);
			// ... and the instance that evaluates a vertex's reflectance on lit paths only, for the scenes whose reflectances are provably finite wherever its
			// per-vertex guard passes (SceneLazyRefl; rl_dev_shade.h LazyVertexSafe), on paths short enough for the guard's bound on a direction's length.
			// The same bits as the eager instance (measured: DESIGN.md section 5).  RAYLIB_LAZY_REFL=0 keeps the eager instance.
			p.lazy = p.plain && k.lazyRefl != 0 && st.maxPathLength <= RL_LAZY_MAX_PATH && SceneLazyRefl(sc);
			// ... and of that, the form whose idle lanes take camera rays that have been traced already, so that every lane enters the shading part with a hit
			// (rl_k_trace_hitq.inl).  The same bits and the same work counters, waveTrips aside.  It traces a camera ray before its path has a depth to test: not
			// with maxPathLength < 1.  RAYLIB_HIT_QUEUE=0|1 overrides the default (measured: DESIGN.md section 5).
			p.hitQueue = p.lazy && st.maxPathLength >= 1 && (k.hitQueue >= 0 ? k.hitQueue != 0 : RL_HIT_QUEUE_DEFAULT != 0);
		}
	}
	return p;
}

} // namespace

int32_t EagerTree(const Scene& sc)
{
	RendererSettings st = {};
	st.renderMode = RAYLIB_RENDERMODE_Default;
	const TracePlan d = Pick(sc, st, false, RenderKnobs(), false);
	return (d.tree == TREE_GRID4 || d.tree == TREE_WIDE8) ? d.tree : TREE_NONE;
}

TracePlan PlanTrace(const Scene& sc, const RendererSettings& st, bool hasSky, const RenderKnobs& knobs)
{
	TracePlan p = Pick(sc, st, hasSky, knobs, true);
	p.eagerTree = EagerTree(sc);
	return p;
}

QueryPlan PlanQuery(const Scene& sc, int32_t kind, const RenderKnobs& k)
{
	QueryPlan p;
	const BVH& b = sc.bvh;
	p.prims = !sc.spheres.empty() || !sc.cubes.empty();
	if (b.depth > 64) { p.ok = false; return p; }
	const int want = k.queryTree ? k.queryTree : 8;
	if (want >= 8 && !p.prims && !b.nodes8.empty() && b.depth8 <= RL_POOL8_MAXLEVELS) {
		p.tree = TREE_WIDE8; p.treeWidth = 8; p.nodeBytes = (uint32_t)sizeof(DNode8); p.stack = 2 * RL_POOL8_MAXLEVELS;
	} else if (want >= 4 && !p.prims && !b.nodes4q.empty() && b.stackNeed4 <= 64) {
		p.tree = TREE_GRID4; p.treeWidth = 4; p.stack = b.stackNeed4 <= 32 ? 32 : 64;
	} else {
		p.stack = b.depth <= 32 ? 32 : 64;
	}
	// the instances with spheres and cubes have no early exit: with them the occlusion query walks to the closest hit (rl_k_query.inl, EARLY)
	p.early = kind == RAYLIB_AMD_QUERY_ANY && !p.prims;
	return p;
}

QueryPlan PlanGBuffer(const Scene& sc, const RenderKnobs& k)
{
	return PlanQuery(sc, RAYLIB_AMD_QUERY_SURFACE, k);   // a pixel is a closest-hit query with its surface: that kind's tree, stack and instance
}

QueryPlan PlanQueryAll(const Scene& sc, const RenderKnobs& k)
{
	QueryPlan p;
	const BVH& b = sc.bvh;
	p.prims = !sc.spheres.empty() || !sc.cubes.empty();
	if (b.depth > 64) { p.ok = false; return p; }
	const int want = k.queryTree ? k.queryTree : 8;
	if (want >= 8 && !p.prims && !b.nodes8.empty() && b.depth8 <= RL_POOL8_MAXLEVELS) {
		p.tree = TREE_WIDE8; p.treeWidth = 8; p.nodeBytes = (uint32_t)sizeof(DNode8); p.stack = 2 * RL_POOL8_MAXLEVELS;
	} else {
		p.stack = b.depth <= 32 ? 32 : 64;   // (no grid-4 instance of k_query_all: 4 asked for, or no 8-wide tree, is the binary tree)
	}
	return p;
}

QueryPlan PlanRadiance(const Scene& sc, const RenderKnobs& k)
{
	QueryPlan p;
	const BVH& b = sc.bvh;
	p.prims = !sc.spheres.empty() || !sc.cubes.empty();
	if (b.depth > 64) { p.ok = false; return p; }
	const int want = k.queryTree ? k.queryTree : 4;
	if (want >= 4 && !p.prims && !b.nodes4q.empty() && b.stackNeed4 <= 64) {
		p.tree = TREE_GRID4; p.treeWidth = 4; p.stack = b.stackNeed4 <= 32 ? 32 : 64;
	} else {
		p.stack = b.depth <= 32 ? 32 : 64;
	}
	return p;
}

QueryPlan PlanNearest(const Scene& sc, int32_t kind, const RenderKnobs& k)
{
	QueryPlan p = PlanRadiance(sc, k);   // the same trees under the same switch
	p.early = kind == RAYLIB_AMD_NEAREST_WITHIN;
	return p;
}

QueryPlan PlanNearestAll(const Scene& sc, const RenderKnobs& k)
{
	return PlanNearest(sc, RAYLIB_AMD_NEAREST_CLOSEST, k);   // k_nearest_all is CLOSEST's walk: its tree, its stack, no early exit
}

QueryPlan PlanSweep(const Scene& sc, int32_t kind, const RenderKnobs& k)
{
	// PlanNearest's trees and stack bounds (k_sweep is the point walk's shape: at most children - 1 pushes per level) with PlanOverlap's default: the grid-4 tree
	// while its walk is the 32-deep instance, else the binary tree.  Measured on the 298 k-triangle room (profiles/sweep_time.log), where the grid walk is the
	// 64-deep instance -- 96 KB of LDS, one workgroup per CU for the binary walk's three: 1 M CLOSEST sweeps of 0.1 extents take 2.2 ms on the binary tree and
	// 4.8 ms on the grid nodes, ANY 1.1 and 2.4 ms, for half the node visits.
	RenderKnobs asked = k;
	if (!asked.queryTree) asked.queryTree = (!sc.bvh.nodes4q.empty() && sc.bvh.stackNeed4 <= 32) ? 4 : 2;
	QueryPlan p = PlanNearest(sc, RAYLIB_AMD_NEAREST_CLOSEST, asked);
	p.early = kind == RAYLIB_AMD_SWEEP_ANY;
	return p;
}

DistanceFieldPlan PlanDistanceField(const Scene& sc, const RenderKnobs& k)
{
	DistanceFieldPlan p;
	p.nearest = PlanNearest(sc, RAYLIB_AMD_NEAREST_CLOSEST, k);   // k_sdf_dist is CLOSEST's walk
	p.rows = PlanQueryAll(sc, k);                                 // k_sdf_rows is k_query_all's counting walk
	return p;
}

QueryPlan PlanOverlap(const Scene& sc, int32_t kind, const RenderKnobs& k)
{
	// Unless RAYLIB_QUERY_TREE says otherwise: the grid-4 tree while its walk is the 32-deep instance, else the binary tree.  Measured (DESIGN.md section 2,
	// profiles/overlap.json): on Cornell, both instances 32 deep, the grid walk is 0 - 8 % faster; on the 298 k-triangle room the grid walk is the 64-deep
	// instance, 2 waves per SIMD for the binary walk's 5, and the self-intersection pass -- queries on the surface, which walk down to many leaves -- takes
	// 0.84 of its time on the binary tree.  (Queries in empty space, which end high in the tree and cost half of that, are faster on the grid nodes even there.)
	RenderKnobs asked = k;
	if (!asked.queryTree) asked.queryTree = (!sc.bvh.nodes4q.empty() && sc.bvh.stackNeed4 <= 32) ? 4 : 2;
	QueryPlan p = PlanRadiance(sc, asked);   // the same trees under the same switch
	p.early = kind == RAYLIB_AMD_OVERLAP_ANY;
	return p;
}

QueryPlan PlanOverlapBoxes(const Scene& sc, int32_t kind, const RenderKnobs& k)
{
	// PlanOverlap's rule: k_overlap_box is that walk with another leaf test (the rule's default was measured on triangles; for boxes: profiles/box_query_time.log)
	return PlanOverlap(sc, kind == RAYLIB_AMD_BOX_ANY ? RAYLIB_AMD_OVERLAP_ANY : RAYLIB_AMD_OVERLAP_LIST, k);
}

GatherCut PlanGatherCut(uint32_t n, uint32_t sampleCount, bool sphere, const RenderKnobs& k)
{
	GatherCut c;
	const uint64_t slotBytes = (sphere ? 2u : 1u) * 16u;   // one float4 (the hemisphere's weighted sample) or two (the sphere's L and Wi)
	const uint64_t slots = k.gatherBatch > 0 ? std::min<uint64_t>((uint64_t)k.gatherBatch, RL_GATHER_MAX_SLOTS) : RL_GATHER_SAMPLE_BUDGET / slotBytes;
	c.pointsPer = (uint32_t)std::min<uint64_t>(n, slots);
	c.samplesPer = (uint32_t)std::min<uint64_t>(sampleCount, std::max<uint64_t>(1, slots / c.pointsPer));
	c.pointRanges = ((uint64_t)n + c.pointsPer - 1) / c.pointsPer;
	c.sampleRanges = ((uint64_t)sampleCount + c.samplesPer - 1) / c.samplesPer;
	c.launches = c.pointRanges * c.sampleRanges;   // (< 2^31 * 2^32)
	return c;
}
GatherLaunch GatherLaunchAt(const GatherCut& c, uint32_t n, uint32_t sampleCount, uint64_t k)
{
	GatherLaunch L;
	const uint64_t pr = k / c.sampleRanges, sr = k % c.sampleRanges;
	const uint64_t pf = pr * c.pointsPer, sb = sr * c.samplesPer;   // (pf < n, sb < sampleCount: both fit 32 bits; their successors may not)
	L.pointFirst = (uint32_t)pf; L.numPoints = (uint32_t)std::min<uint64_t>(c.pointsPer, (uint64_t)n - pf);
	L.sampleBase = (uint32_t)sb; L.numSamples = (uint32_t)std::min<uint64_t>(c.samplesPer, (uint64_t)sampleCount - sb);
	L.first = sr == 0; L.last = sr + 1 == c.sampleRanges;
	return L;
}

LaunchPlan PlanLaunch(uint32_t numLocalCells, uint32_t numActive, uint32_t spp, uint32_t sampleBegin, int numCUs, int workgroupsPerCU,
                      const TracePlan& trace, const RenderKnobs& k)
{
	LaunchPlan L;
	// sample batches: one launch per <= 16 GiB of sample buffer (288 GB of HBM: few, large launches -- every launch pays its ramp-up and its tail once;
	// measured on the 298 k-triangle scene at 128 spp: 1 launch 61.3 ms, 2 launches 68.9, 4 launches 90.1)
	const size_t perSample = (size_t)numLocalCells * 64u * sizeof(SampleRGB);
	const size_t capBytes = (size_t)(k.sampleBufferGiB > 0 ? k.sampleBufferGiB : 16) << 30;
	L.batch = (uint32_t)std::max<size_t>(1, std::min<size_t>(spp, perSample ? capBytes / perSample : spp));
	if (k.sampleBatch > 0) L.batch = std::min<uint32_t>((uint32_t)k.sampleBatch, spp);
	L.sampleCount = sampleBegin < spp ? std::min(L.batch, spp - sampleBegin) : 0;
	const uint32_t pathsPerThread = trace.poolK > 0 ? (uint32_t)trace.poolK : 1u;
	const int perCU = k.blocksPerCU > 0 ? k.blocksPerCU : std::max(1, workgroupsPerCU);
	const uint64_t jobs64 = (uint64_t)numActive * L.sampleCount * 64u;
	L.jobs = jobs64;
	L.blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)numCUs * perCU, (jobs64 + RL_BLOCK * pathsPerThread - 1) / (RL_BLOCK * pathsPerThread)));
	L.stackStride = L.blocks * RL_BLOCK * pathsPerThread;
	const bool leafList = trace.poolK == 0 && trace.lds == 2;
	{   // jobs per global atomic: ~1/16 of a wave's share, rounded to a multiple of 64 (one cell at one sample), 64..1024.
		// Measured on the slice one of 8 ranks renders of the 1080p x 64 spp Cornell frame (16.6 M jobs): 64 -> 4.10 ms,
		// 128 -> 3.62, 256 -> 3.45, 512 -> 3.53, 1024 -> 4.07; on the whole frame 1024 is best (64 -> 33.6 ms: the atomic saturates).
		const uint64_t waves = (uint64_t)L.blocks * (RL_BLOCK / 64);
		uint64_t chunk = ((jobs64 / (waves * 16)) + 32) & ~63ull;
		if (k.jobChunk >= 0) chunk = (uint64_t)k.jobChunk;
		L.jobChunk = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(64, chunk));
		// The pool schedule's jobs differ by two orders of magnitude (a cell that misses the scene's root box against one full of geometry): the launch's
		// tail is what a wave needs for its LAST chunk, and on the 298 k-triangle frame a chunk of 1024 heavy jobs is 6 ms of a 45 ms launch (wave timeline,
		// tools/gpu_timeline_pool.py: first wave out of jobs at 39.7 ms, last at 46.0).  One head took chunks no smaller than 1024 (256: 48.1 ms, the atomic's
		// queue); with a head per XCD 256 is the best: 1024 -> 46.5 ms, 512 -> 45.0, 256 -> 44.0, 128 -> 44.0, 64 -> 48.4 (one head, 1024: 44.9).
		if (trace.poolK > 0 && k.jobChunk < 0) {
			const uint32_t h = k.jobHeads > 0 ? (uint32_t)k.jobHeads : RL_MAX_HEADS;
			if (h >= 4) L.jobChunk = std::min<uint32_t>(L.jobChunk, 256u);
			// ... and with the cells that cannot see the scene out of the list (CullCells) every job is a heavy one and there are far fewer of them: 128
			// as long as that stays under ~400 k draws per launch (298 k frame, 29 M jobs: 256 -> 37.75 ms, 128 -> 37.25, 64 -> 37.2, 512 -> 38.7)
			if (h >= 4 && numActive < numLocalCells && jobs64 / 128u <= 400000u) L.jobChunk = std::min<uint32_t>(L.jobChunk, 128u);
		}
		// the leaf-list kernel's chunk belongs to a workgroup, whose four waves draw batches of 64 from it (RL_QUEUE_SHARED_CHUNK): four waves' worth, 1024 at most
		if (RL_QUEUE_SHARED_CHUNK && leafList && k.jobChunk < 0) L.jobChunk = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(256, 4 * chunk));
		// a chunk is whole batches of 64 jobs (one cell at one sample: DecodeJobBatch decodes base >> 6, TakeJobs packs the head's number into the low
		// bits of a band's job count) whatever the environment asked for
		L.jobChunk = std::max(64u, L.jobChunk & ~63u);
	}
	{   // the job list in bands of whole cells, one head per XCD (rl_dev_jobs.h TakeJobs)
		uint32_t heads = k.jobHeads > 0 ? std::min<uint32_t>(RL_MAX_HEADS, (uint32_t)k.jobHeads) : RL_MAX_HEADS;
		const uint32_t cellsPerHead = (std::max(1u, numActive) + heads - 1) / heads;
		heads = (std::max(1u, numActive) + cellsPerHead - 1) / cellsPerHead;   // no empty band: every head's first job exists (and h * jobsPerHead < numJobs < 2^32)
		L.heads = heads; L.jobsPerHead = cellsPerHead * L.sampleCount * 64u;
		// guided draws at the end of a band: 2^shift ~ twice the drawers per head (waves; workgroups in the leaf-list kernel, whose chunk is shared)
		const bool perBlockChunk = RL_QUEUE_SHARED_CHUNK && leafList;
		const uint32_t drawers = std::max(1u, L.blocks * (perBlockChunk ? 1u : (uint32_t)(RL_BLOCK / 64)) / heads);
		uint32_t shift = 1; while ((1u << shift) < 2u * drawers && shift < 24u) ++shift;
		// measured: no gain on either bench workload -- a heavy chunk drawn three rounds before the end outlasts the guided ones
		L.guideShift = k.guided > 0 ? shift + (uint32_t)(k.guided - 1) : 0u;
	}
	return L;
}

ViewsPlan PlanViews(const CullScene& cs, const RendererSettings& st, const DCamera* cameras, uint32_t count, const TracePlan& trace,
                    int numCUs, int workgroupsPerCU, const RenderKnobs& knobs)
{
	ViewsPlan V;
	const uint32_t W = st.viewportWidth, H = st.viewportHeight, cellsX = (W + 7) / 8;
	V.cellsPerView = cellsX * ((H + 7) / 8);
	V.numCells = V.cellsPerView * count;
	V.empty.assign(V.numCells, 0);
	V.culledPerView.assign(count, 0);
	V.active.reserve(V.numCells);
	bool haveL = false;
	for (uint32_t v = 0; v < count; ++v) {
		CullResult cr;
		const uint32_t base = v * V.cellsPerView;
		bool culled = trace.pathTrace && CullCells(cs, cameras[v], st.maxPathLength, st.rayTMin, W, H, cellsX, 0, 1, V.cellsPerView, cr);
		if (culled && haveL && (memcmp(cr.L, V.emptyL, sizeof(V.emptyL)) != 0 || cr.raysPerSample != V.raysPerSample)) culled = false;   // (does not happen: see rl_plan.h)
		if (!culled) { for (uint32_t c = 0; c < V.cellsPerView; ++c) V.active.push_back(base + c); continue; }
		if (!haveL) { memcpy(V.emptyL, cr.L, sizeof(V.emptyL)); V.raysPerSample = cr.raysPerSample; haveL = true; }
		for (uint32_t k : cr.active) V.active.push_back(base + k);
		for (uint32_t c = 0; c < V.cellsPerView; ++c) V.empty[base + c] = cr.empty[c];
		V.culledPerView[v] = V.cellsPerView - (uint32_t)cr.active.size();
		V.emptyPixels += cr.emptyPixels;
	}
	V.numActive = (uint32_t)V.active.size();
	const uint32_t spp = (uint32_t)(st.samplesPerPixel > 1 ? st.samplesPerPixel : 1);
	// the job-count guard of a launch (rl_rt_frame.hip EnqueueFrame) splits samples into batches, never views
	const uint64_t perSample = (uint64_t)V.numActive * 64u;
	const uint64_t maxBatch = perSample ? 0xF0000000ull / perSample : spp;
	V.knobs = knobs;
	if (maxBatch == 0) return V;
	V.launch = PlanLaunch(V.numCells, V.numActive, spp, 0, numCUs, workgroupsPerCU, trace, V.knobs);
	if (V.launch.batch > maxBatch) {
		V.knobs.sampleBatch = (int)maxBatch;
		V.launch = PlanLaunch(V.numCells, V.numActive, spp, 0, numCUs, workgroupsPerCU, trace, V.knobs);
	}
	V.ok = true;
	return V;
}

CullScene SceneCullScene(const Scene& sc, bool hasSky)
{
	CullScene cs;
	cs.prims = !sc.spheres.empty() || !sc.cubes.empty();
	cs.hasSky = hasSky;
	cs.hasSun = !(sc.sunIlluminance.x == 0.0f && sc.sunIlluminance.y == 0.0f && sc.sunIlluminance.z == 0.0f);
	cs.sunIlluminance[0] = sc.sunIlluminance.x; cs.sunIlluminance[1] = sc.sunIlluminance.y; cs.sunIlluminance[2] = sc.sunIlluminance.z;
	cs.sunDirection[0] = sc.sunDirection.x; cs.sunDirection[1] = sc.sunDirection.y; cs.sunDirection[2] = sc.sunDirection.z;
	if (!cs.prims && !sc.bvh.nodes.empty() && !sc.triangles.empty()) {
		const DNode& root = sc.bvh.nodes[0];
		bool ok = true;
		for (int k = 0; k < 3; ++k) {
			double lo = 1e300, hi = -1e300;
			if (root.left != DNODE_EMPTY) { lo = std::min(lo, (double)root.lmin[k]); hi = std::max(hi, (double)root.lmax[k]); }
			if (root.right != DNODE_EMPTY) { lo = std::min(lo, (double)root.rmin[k]); hi = std::max(hi, (double)root.rmax[k]); }
			if (!(lo <= hi) || !std::isfinite(lo) || !std::isfinite(hi)) ok = false;
			cs.boundsMin[k] = lo; cs.boundsMax[k] = hi;
		}
		cs.boundsValid = ok;
	}
	return cs;
}

} // namespace rl
