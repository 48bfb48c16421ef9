// Host runtime: which kernel a plan names, the one path on which every render is queued (BeginFrame, EnqueueFrame), a rank's share of a one-view render or a
// pass of a progressive session (EnqueueRender), the one wait and the numbers behind it (FinishRender), and a batch of views (rl_rt.h).
#include "rl_rt.h"

#include <atomic>

namespace rl {

// The kernels a render launches go by address (hipLaunchKernel): a one-view kernel and its views twin (RaylibAMD_RenderViews) differ by the twin's trailing DViews.
typedef void (*TraceKernel)(const DRenderParams, const DSceneView, const SkyRot, SampleRGB*, float*, unsigned long long*, unsigned int*);
typedef void (*TraceViewsKernel)(const DRenderParams, const DSceneView, const SkyRot, SampleRGB*, float*, unsigned long long*, unsigned int*, const DViews);
typedef void (*TraceLazyKernel)(const DRenderParams, const DSceneView, const SkyRot, SampleRGB*, float*, unsigned long long*, unsigned int*, const DLitList);
typedef void (*AovKernel)(const DRenderParams, const DSceneView, float4*, unsigned long long*);
typedef void (*AovViewsKernel)(const DRenderParams, const DSceneView, float4*, unsigned long long*, const DViews);

// The kernel instance of a plan (rl_plan.cc), or its views twin: the only code that names the instances of k_trace, k_trace_pool and k_aov a render launches.
// Every instance has its twin, so that a batch of views is never a loop of one-view launches.
template <int STACK, bool PRIMS, bool FULL, int LDS = 0, bool PLAIN = false>
static const void* Trace(bool views)
{
	return views ? (const void*)(TraceViewsKernel)k_trace_views<STACK, PRIMS, FULL, LDS, PLAIN> : (const void*)(TraceKernel)k_trace<STACK, PRIMS, FULL, LDS, PLAIN>;
}
template <int STACK, bool PRIMS>
static const void* TraceFor(bool floatBoxes, bool views) { return floatBoxes ? Trace<STACK, PRIMS, true>(views) : Trace<STACK, PRIMS, false>(views); }
template <int STACK, bool PRIMS>
static const void* Aov(bool views) { return views ? (const void*)(AovViewsKernel)k_aov_views<STACK, PRIMS> : (const void*)(AovKernel)k_aov<STACK, PRIMS>; }
static const void* KernelFor(const TracePlan& p, bool views)
{
	if (p.poolK > 0) {   // the instances rl_render_pool.hip defines: (STACK, PRIMS, K, LSTACK, WIDE), WIDE 0 the BVH2, 1 the grid nodes, 3 the 8-wide tree
		const int wide = p.tree == TREE_WIDE8 ? 3 : p.tree == TREE_GRID4 ? 1 : 0;
#define RL_POOL_PICK(a, b, c, d, e) if (p.stack == a && p.prims == b && p.poolK == c && p.lstack == d && wide == e) \
			return views ? (const void*)(TraceViewsKernel)k_trace_pool_views<a, b, c, d, e> : (const void*)(TraceKernel)k_trace_pool<a, b, c, d, e>;
		RL_POOL_INSTANCES(RL_POOL_PICK)
#undef RL_POOL_PICK
		return nullptr;
	}
	if (p.lds == 2 && p.lazy && p.hitQueue && !views) return (const void*)(TraceLazyKernel)k_trace_lazy_hitq<16, false, true, 2, true>;
	if (p.lds == 2 && p.lazy && !views) return (const void*)(TraceLazyKernel)k_trace_lazy<16, false, true, 2, true>;   // (a batch of views stays eager: the plain twin)
	if (p.lds == 2) return p.plain ? Trace<16, false, true, 2, true>(views) : Trace<16, false, true, 2>(views);
	if (p.lds == 1) return Trace<16, false, true, 1>(views);
	const bool full = p.tree == TREE_BOX4;
	if (p.stack == 16) return TraceFor<16, false>(full, views);
	if (p.stack == 32) return p.prims ? TraceFor<32, true>(full, views) : TraceFor<32, false>(full, views);
	return p.prims ? TraceFor<64, true>(full, views) : TraceFor<64, false>(full, views);
}
static const void* AovKernelFor(const TracePlan& p, bool views)
{
	if (p.stack == 16) return Aov<16, false>(views);
	if (p.stack == 32) return p.prims ? Aov<32, true>(views) : Aov<32, false>(views);
	return p.prims ? Aov<64, true>(views) : Aov<64, false>(views);
}
static std::atomic<int32_t> g_lastTracePlain{0};   // RaylibAMD_LastTracePlain: set by EnqueueFrame
int32_t DeviceLastTracePlain() { return g_lastTracePlain.load(std::memory_order_relaxed); }
static std::atomic<int32_t> g_lastTraceLazy{0};    // RaylibAMD_LastTraceLazy
int32_t DeviceLastTraceLazy() { return g_lastTraceLazy.load(std::memory_order_relaxed); }
static std::atomic<int32_t> g_lastHitQueue{0};     // RaylibAMD_LastHitQueue
int32_t DeviceLastHitQueue() { return g_lastHitQueue.load(std::memory_order_relaxed); }
static std::atomic<int32_t> g_lastLitMask{0};      // RaylibAMD_LastLitMask
int32_t DeviceLastLitMask() { return g_lastLitMask.load(std::memory_order_relaxed); }

// What differs between the frames the runtime queues -- a rank's share of a one-view render, a pass of a progressive session, a batch of views (EnqueueRender,
// DeviceRenderViews): they fill this in, EnqueueFrame queues what it says.
struct Frame {
	RenderKnobs knobs;                   // what the launches are planned with (a batch of views: ViewsPlan::knobs, whose sampleBatch may be lowered)
	TracePlan plan;
	DSceneView view;                     // TraceView
	DRenderParams P;                     // BaseParams and the job list (ListCells); EnqueueFrame sets the per-launch fields
	uint32_t numLive = 0, numActive = 0; // of P.numLocalCells cells: those still sampled, and those of them in the job list (ListCells; else all)
	uint32_t sBegin = 0, sEnd = 1;       // the samples to render
	float4* out = nullptr;
	const DViews* views = nullptr;       // a batch of views: the twins are launched, with this as their trailing argument
	// behind every batch: k_resolve, k_resolve_views or k_progressive_resolve as resolve(P, view, skyRot, the rank's samples, resolveArgs...)
	const void* resolve = nullptr;
	void* resolveArgs[5] = {};
	int firstBatch = 0, lastBatch = 0;   // (of the batch being queued: what resolveArgs may point at)
	bool accum = true;                   // the resolve sums the batches in the rank's accum buffer: grown when there is more than one
	ProgressiveSession* compact = nullptr;   // behind the last batch: k_progressive_compact on the session's lists, and its counts to pinned memory
};

// DRenderParams as far as settings, seed and cell geometry decide them: the frame's cells cellFirst, cellFirst + stride, ..., numLocalCells of them
static DRenderParams BaseParams(const RendererSettings& st, uint64_t seed, const DCamera& camera, uint32_t cellFirst, uint32_t stride, uint32_t numLocalCells, bool rowMajor)
{
	DRenderParams P; memset(&P, 0, sizeof(P));
	const uint32_t W = st.viewportWidth, H = st.viewportHeight, cellsX = (W + 7) / 8;
	P.width = W; P.height = H; P.spp = (uint32_t)(st.samplesPerPixel > 1 ? st.samplesPerPixel : 1); P.maxPathLength = st.maxPathLength; P.rayTMin = st.rayTMin;
	P.invWidth = 1.0f / (float)W; P.invHeight = 1.0f / (float)H;   // correctly rounded (IEEE division on the host): rl_dev_jobs.h PixelUV
	P.renderMode = st.renderMode; P.seed = seed; P.cellsX = cellsX; P.cellsY = (H + 7) / 8;
	P.cellFirst = cellFirst; P.cellStride = stride; P.numLocalCells = numLocalCells;
	P.rowMajorOutput = rowMajor ? 1u : 0u; P.camera = camera;
	P.seedMixed = raylib_rng_mix64(seed);
	P.magicCellsX = cellsX > 1 ? (uint32_t)(0x100000000ull / cellsX) : 0xFFFFFFFFu;
	return P;
}

// the valid pixels of the cells cellFirst, cellFirst + stride, ... (count of them) of a W x H frame
static uint64_t CoveredPixels(uint32_t W, uint32_t H, uint32_t cellFirst, uint32_t stride, uint32_t count)
{
	const uint32_t cellsX = (W + 7) / 8;
	uint64_t px = 0;
	for (uint32_t k = 0; k < count; ++k) {
		const uint32_t cell = cellFirst + k * stride, cx = cell % cellsX, cy = cell / cellsX;
		px += (uint64_t)std::min(8u, W - cx * 8) * std::min(8u, H - cy * 8);
	}
	return px;
}

// the scene as a plan's kernels read it: the plan's wide tree is on the device (EnsureWideTree), the wide nodes it does not walk are out of the view (k_trace tells the tree
// by which is set; a debug mode's plan keeps both)
static bool TraceView(DeviceSceneCopy* D, Scene& sc, const TracePlan& plan, DSceneView& view)
{
	if (!EnsureWideTree(D, sc, plan.tree)) return false;
	view = D->view;
	if (!plan.keepNodes4) view.nodes4 = nullptr;
	if (!plan.keepNodes4f) view.nodes4f = nullptr;
	return true;
}

// The frame's job list (device memory): numListed of its numLive live cells, ascending, and a flag per cell for those outside the scene's silhouette, whose samples are
// the constant L (plus their sky texel) and stand for emptyPixels pixels and raysPerSample rays each in the counters (CullCells).
static void ListCells(Frame& F, PendingRender& pend, const uint32_t* list, const uint8_t* empty, uint32_t numListed, uint32_t numLive, const float* L, uint64_t emptyPixels, uint32_t raysPerSample)
{
	DRenderParams& P = F.P;
	F.numLive = numLive; F.numActive = numListed;
	P.activeCells = list; P.cellEmpty = empty; P.numActiveCells = numListed;
	P.emptyL[0] = L[0]; P.emptyL[1] = L[1]; P.emptyL[2] = L[2];
	P.emptySky = F.view.sky ? 1u : 0u;
	pend.culledSamples = emptyPixels * (uint64_t)(F.sEnd - F.sBegin); pend.culledRaysPerSample = raysPerSample; pend.culledSkyTexels = F.view.sky ? 1u : 0u;
}

// The head of every frame on the rank's stream: the counters reset and the start event of frame slot q.
static bool BeginFrame(RankCtx& R, int q, const Frame& F, size_t outBytes, PendingRender& pend)
{
	pend.pathTrace = F.plan.pathTrace; pend.slot = q; pend.cnt = R.cntHost[q].ptr;
	pend.out = F.out; pend.outBytes = outBytes;
	HIP_OK(hipMemsetAsync(R.counters.ptr, 0, RL_CNT_BLOCK * sizeof(unsigned long long), R.stream));
	HIP_OK(hipEventRecord(R.ev[q][0], R.stream));
	return true;
}

// The rest of the frame behind BeginFrame, queued and not waited for: the megakernel and the resolve per sample batch (or k_aov), what follows the last batch, the end
// event and the counter read-back.  False (a HIP call failed, logged) leaves pend.enqueuedToEnd unset: FinishRender then drains the stream.
static bool EnqueueFrame(RankCtx& R, int q, const DeviceScene& DS, Frame& F, PendingRender& pend)
{
	const TracePlan& plan = F.plan;
	DRenderParams& P = F.P;
	const uint32_t numCells = P.numLocalCells, numSlots = numCells * 64u;
	const uint32_t rblocks = (numSlots + RL_BLOCK - 1) / RL_BLOCK;   // one thread per pixel slot: k_aov and the resolves
	SkyRot skyRot = DS.skyRot;
	if (numSlots == 0) {
		// nothing to do for this rank
	} else if (!plan.pathTrace) {
		void* args[] = { &P, &F.view, &F.out, &R.counters.ptr, (void*)F.views };
		HIP_OK(hipLaunchKernel(AovKernelFor(plan, F.views != nullptr), dim3(rblocks), dim3(RL_BLOCK), args, 0, R.stream));
	} else {
		const void* traceKernel = KernelFor(plan, F.views != nullptr);
		if (!traceKernel) { Log("Raylib_Render: no megakernel instance for STACK %d, K %d, stack in LDS %d", plan.stack, plan.poolK, plan.lstack); return false; }
		const int blocksPerCU = OccupancyOf(R, traceKernel, &plan);
		if (blocksPerCU < 0) return false;
		g_lastTracePlain.store(plan.plain ? 1 : 0, std::memory_order_relaxed);
		const bool lazy = plan.lazy && !F.views;   // k_trace_lazy: the lit list is its trailing argument; its waves fold the list themselves, only the resolve follows
		g_lastTraceLazy.store(lazy ? 1 : 0, std::memory_order_relaxed);
		g_lastHitQueue.store(lazy && plan.hitQueue ? 1 : 0, std::memory_order_relaxed);
		pend.lazy = lazy;
		DLitList LL = {};
		pend.pathsPerWave = plan.pathsPerWave; pend.treeWidth = plan.treeWidth; pend.nodeBytes = plan.nodeBytes;
		pend.culledCells = F.numLive - F.numActive; pend.listedCells = F.numActive;
		const uint32_t batch = PlanLaunch(numCells, F.numActive, F.sEnd, F.sBegin, R.numCUs, blocksPerCU, plan, F.knobs).batch;
		if (!R.samples.Grow((size_t)numSlots * sizeof(SampleRGB) * std::min(batch, F.sEnd - F.sBegin))) return false;
		if (F.accum && batch < P.spp && !R.accum.Grow((size_t)numSlots * sizeof(float4))) return false;
		// the lit-sample mask (rl_lit_mask.h): a lazy launch behind which k_resolve runs (not a progressive pass, not a batch of views) whose samples fit the mask's
		// words.  With a sun most samples are lit and would pay an atomic each: not there, unless RAYLIB_LIT_MASK=1 asks for it.  RAYLIB_LIT_MASK=0: never.
		const bool masked = lazy && F.resolve == (const void*)k_resolve && F.knobs.litMask != 0 && (F.knobs.litMask > 0 || !F.view.hasSun) &&
		                    (std::min(batch, F.sEnd - F.sBegin) + 31u) / 32u <= RL_LIT_MASK_MAX_WORDS;
		g_lastLitMask.store(masked ? 1 : 0, std::memory_order_relaxed);
		const void* resolveKernel = masked ? (const void*)k_resolve_lit : F.resolve;
		const int depthSlots = P.maxPathLength > 1 ? P.maxPathLength : 1;
		void* traceArgs[] = { &P, &F.view, &skyRot, &R.samples.ptr, &R.pathStack.ptr, &R.counters.ptr, &R.jobCounter.ptr, lazy ? (void*)&LL : (void*)F.views };
		void* resolveArgs[] = { &P, &F.view, &skyRot, &R.samples.ptr, F.resolveArgs[0], F.resolveArgs[1], F.resolveArgs[2], F.resolveArgs[3], masked ? (void*)&LL : F.resolveArgs[4] };
		for (uint32_t s0 = F.sBegin; s0 < F.sEnd; s0 += batch) {
			const LaunchPlan L = PlanLaunch(numCells, F.numActive, F.sEnd, s0, R.numCUs, blocksPerCU, plan, F.knobs);
			const uint32_t cnt = L.sampleCount;
			P.sampleBegin = s0; P.sampleCount = cnt;
			P.magicSamples = cnt > 1 ? (uint32_t)(0x100000000ull / cnt) : 0xFFFFFFFFu;
			if (L.jobs > 0xF0000000ull) { Log("Raylib_Render: job count overflow"); return false; }   // (a head overshoots its band by one chunk per wave and attempt)
			P.numJobs = (uint32_t)L.jobs;
			P.stackStride = L.stackStride; P.jobChunk = L.jobChunk;
			P.numHeads = L.heads; P.jobsPerHead = L.jobsPerHead; P.guideShift = L.guideShift;
			if (!R.pathStack.Grow((size_t)depthSlots * 8 * P.stackStride * sizeof(float))) return false;
			if (lazy) {
				// the lit list: an entry per 32 jobs of the launch (the Cornell frame lights 2 % of its traced paths, 0.7 % of its jobs; a scene that lights more folds the rest in
				// place) and a chunk per wave on top, because every wave with a lit path holds a chunk of its own, unless RAYLIB_LIT_LIST says otherwise; in whole
				// chunks; its chunk counter is reset per launch
				const uint64_t want = F.knobs.litList >= 0 ? (uint64_t)F.knobs.litList
				                                           : std::max<uint64_t>(4096, L.jobs / 32) + (uint64_t)L.blocks * (RL_BLOCK / 64) * RL_LIT_CHUNK;
				const uint32_t chunks = (uint32_t)std::min<uint64_t>(want / RL_LIT_CHUNK, 0x7FFFFFFFu / RL_LIT_CHUNK);
				if (!R.litList.Grow(std::max<size_t>(1, chunks) * RL_LIT_CHUNK * RL_LIT_STRIDE * sizeof(float4))) return false;
				if (!R.litCtl.Grow(sizeof(uint32_t))) return false;
				LL.entries = (float*)R.litList.ptr; LL.ctl = R.litCtl.ptr; LL.numChunks = chunks;
				HIP_OK(hipMemsetAsync(R.litCtl.ptr, 0, sizeof(uint32_t), R.stream));
				if (masked) {   // a bit per sample of this batch, zeroed behind the resolve that read the last batch's
					const uint32_t words = (cnt + 31u) / 32u;
					const size_t bytes = (size_t)words * numSlots * sizeof(uint32_t);
					if (!R.litMask.Grow(bytes)) return false;
					LL.mask = R.litMask.ptr; LL.maskWords = words;
					HIP_OK(hipMemsetAsync(R.litMask.ptr, 0, bytes, R.stream));
				}
			}
			pend.jobHeads = L.heads;
			F.firstBatch = s0 == F.sBegin; F.lastBatch = s0 + cnt >= F.sEnd;
			HIP_OK(hipMemsetAsync(R.jobCounter.ptr, 0, RL_MAX_HEADS * RL_HEAD_STRIDE * sizeof(unsigned int), R.stream));   // heads count from their band's first job: one memset
			HIP_OK(hipEventRecord(R.ev[q][2], R.stream));
			if (L.jobs > 0)   // (else no cell of this frame sees the scene: the resolve has all it needs)
				HIP_OK(hipLaunchKernel(traceKernel, dim3(L.blocks), dim3(RL_BLOCK), traceArgs, 0, R.stream));
			HIP_OK(hipEventRecord(R.ev[q][3], R.stream));
			HIP_OK(hipLaunchKernel(resolveKernel, dim3(rblocks), dim3(RL_BLOCK), resolveArgs, 0, R.stream));
			++pend.launches;
			if (!F.lastBatch) {   // the event pair is reused by the next batch; the last batch's pair is read after the one final sync
				HIP_OK(hipEventSynchronize(R.ev[q][3]));
				float ms = 0.0f;
				HIP_OK(hipEventElapsedTime(&ms, R.ev[q][2], R.ev[q][3]));
				pend.traceMs += ms;
			} else pend.lastBatchPending = true;
		}
		if (ProgressiveSession* S = F.compact) {   // the cells that stopped leave the lists; the counts go to pinned memory, where the session reads them once the pass is waited for
			hipLaunchKernelGGL(k_progressive_compact, dim3(1), dim3(RL_COMPACT_BLOCK), 0, R.stream,
			                   S->live.ptr, S->trace.ptr, (const uint8_t*)S->st.stopped, (const uint8_t*)S->empty.ptr, S->numLive, P.width, P.height, P.cellsX, S->counts.ptr);
			HIP_OK(hipGetLastError());
			HIP_OK(hipMemcpyAsync(S->countsHost.ptr, S->counts.ptr, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, R.stream));
		}
	}
	if (!plan.pathTrace) pend.listedCells = numCells;
	HIP_OK(hipEventRecord(R.ev[q][1], R.stream));
	HIP_OK(hipMemcpyAsync(R.cntHost[q].ptr, R.counters.ptr, (CNT_COUNT + 24) * sizeof(unsigned long long), hipMemcpyDeviceToHost, R.stream));
	if (pend.lazy) HIP_OK(hipMemcpyAsync(R.cntHost[q].ptr + CNT_COUNT + 24, R.counters.ptr + RL_CNT_LIT, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, R.stream));
	HIP_OK(hipEventRecord(R.ev[q][7], R.stream));
	pend.enqueuedToEnd = true;
	return true;
}

// One rank's share of a one-view render, queued on its stream (BeginFrame, EnqueueFrame).  `req.outDevice` receives the row-major frame (cellStride 1) or the rank's cells
// back to back.  The job list is the cull's, cached per frame slot.
// With `prog` (rank 0, the whole frame): one pass of a progressive session -- the samples [prog->samples, prog->passEnd) of its live cells, its lists in place
// of the cull's (seeded from the cull at its first pass), k_progressive_resolve in place of k_resolve, and k_progressive_compact behind the last batch.
bool EnqueueRender(RankCtx& R, Scene& sc, const RenderRequest& req, PendingRender& pend, ProgressiveSession* prog)
{
	DeviceSceneCopy* D = sc.device->copy[(size_t)R.devSlot];
	const RendererSettings& st = req.settings;
	Frame F;
	F.knobs = ReadRenderKnobs();
	F.plan = PlanTrace(sc, st, D->view.sky != nullptr, F.knobs);
	if (!F.plan.ok || !TraceView(D, sc, F.plan, F.view)) return false;
	const uint32_t W = st.viewportWidth, H = st.viewportHeight;
	const uint32_t cellsX = (W + 7) / 8, numCells = cellsX * ((H + 7) / 8);
	const uint32_t stride = req.cellStride ? req.cellStride : 1;
	const uint32_t numLocalCells = req.cellFirst < numCells ? (numCells - req.cellFirst + stride - 1) / stride : 0;
	const bool rowMajor = (stride == 1 && req.cellFirst == 0 && !req.cellMajor);
	const int q = req.slot & 1;
	F.P = BaseParams(st, req.seed, req.camera, req.cellFirst, stride, numLocalCells, rowMajor);
	F.numLive = F.numActive = numLocalCells;
	F.sBegin = prog ? prog->samples : 0u; F.sEnd = prog ? prog->passEnd : F.P.spp;
	const size_t outBytes = rowMajor ? (size_t)W * H * sizeof(float4) : (size_t)numLocalCells * 64u * sizeof(float4);
	F.out = (float4*)req.outDevice;
	if (!F.out) { if (!R.image.Grow(outBytes ? outBytes : 16)) return false; F.out = R.image.ptr; }
	if (!BeginFrame(R, q, F, outBytes, pend)) return false;
	if (F.plan.pathTrace && numLocalCells && (!prog || !prog->seeded)) {
		// ---- cells that cannot see the scene leave the job list (CullCells) ----
		// what the decision depends on: an unchanged view keeps the lists the slot already holds on the device
		const CullScene cs = SceneCullScene(sc, F.view.sky != nullptr);
		std::vector<unsigned char> key;
		auto put = [&](const void* ptr, size_t n) { const unsigned char* b = (const unsigned char*)ptr; key.insert(key.end(), b, b + n); };
		const uint32_t geo[7] = { W, H, req.cellFirst, stride, numLocalCells, (uint32_t)st.maxPathLength, __builtin_bit_cast(uint32_t, st.rayTMin) };
		const int flags[3] = { cs.hasSky ? 1 : 0, cs.hasSun ? 1 : 0, F.knobs.cullCells };
		put(&req.camera, sizeof(req.camera)); put(geo, sizeof(geo)); put(flags, sizeof(flags)); put(cs.sunDirection, sizeof(cs.sunDirection));
		put(cs.sunIlluminance, sizeof(cs.sunIlluminance)); put(cs.boundsMin, sizeof(cs.boundsMin)); put(cs.boundsMax, sizeof(cs.boundsMax));
		const void* sceneId = sc.device; put(&sceneId, sizeof(sceneId));
		if (key != R.cullKey[q]) {
			CullResult cr;
			const bool culled = CullCells(cs, req.camera, st.maxPathLength, st.rayTMin, W, H, cellsX, req.cellFirst, stride, numLocalCells, cr);
			R.cullKey[q].clear();   // (valid again once the slot's buffers hold this view)
			R.cullActive[q] = numLocalCells; R.cullEmptyPixels[q] = 0;
			if (culled) {
				if (R.cellListCells[q] < numLocalCells) {
					R.cellListCells[q] = 0;
					// the list (uint32 per cell) and the flags (one byte per cell, behind it) in one buffer
					if (!R.cellListHost[q].Grow((size_t)numLocalCells * 5 + 16) || !R.cellList[q].Grow((size_t)numLocalCells * 5 + 16)) return false;
					R.cellListCells[q] = numLocalCells;
				}
				// (the slot's staging buffer is free: the frame that used it last has been waited for -- FinishRender, or FinishInflight before a slot is re-used)
				memcpy(R.cellListHost[q].ptr, cr.active.data(), cr.active.size() * sizeof(uint32_t));
				memcpy((unsigned char*)(R.cellListHost[q].ptr + R.cellListCells[q]), cr.empty.data(), numLocalCells);
				HIP_OK(hipMemcpyAsync(R.cellList[q].ptr, R.cellListHost[q].ptr, (size_t)R.cellListCells[q] * 5, hipMemcpyHostToDevice, R.stream));
				R.cullActive[q] = (uint32_t)cr.active.size(); R.cullEmptyPixels[q] = cr.emptyPixels;
				R.cullL[q][0] = cr.L[0]; R.cullL[q][1] = cr.L[1]; R.cullL[q][2] = cr.L[2]; R.cullRays[q] = cr.raysPerSample;
			}
			R.cullKey[q] = key;
		}
		const uint32_t* list = R.cellList[q].ptr; const uint8_t* empty = (const uint8_t*)(R.cellList[q].ptr + R.cellListCells[q]);
		if (!prog) {
			if (R.cullActive[q] < numLocalCells) ListCells(F, pend, list, empty, R.cullActive[q], numLocalCells, R.cullL[q], R.cullEmptyPixels[q], R.cullRays[q]);
		} else {   // the session's first pass: its lists start from the cull's (every cell is live)
			if (R.cullActive[q] < numLocalCells) {
				HIP_OK(hipMemcpyAsync(prog->trace.ptr, list, (size_t)R.cullActive[q] * sizeof(uint32_t), hipMemcpyDeviceToDevice, R.stream));
				HIP_OK(hipMemcpyAsync(prog->empty.ptr, empty, numLocalCells, hipMemcpyDeviceToDevice, R.stream));
				prog->emptyLivePixels = R.cullEmptyPixels[q]; prog->culledRays = R.cullRays[q];
				for (int k = 0; k < 3; ++k) prog->emptyL[k] = R.cullL[q][k];
			}
			prog->numLive = numLocalCells; prog->numTrace = R.cullActive[q];
			prog->seeded = true;
		}
	}
	if (prog) {
		if (F.plan.pathTrace && numLocalCells) ListCells(F, pend, prog->trace.ptr, prog->empty.ptr, prog->numTrace, prog->numLive, prog->emptyL, prog->emptyLivePixels, prog->culledRays);
		F.resolve = (const void*)k_progressive_resolve; F.resolveArgs[0] = &prog->st; F.resolveArgs[1] = &F.out; F.resolveArgs[2] = &F.lastBatch;
		F.accum = false; F.compact = prog;
	} else {
		F.resolve = (const void*)k_resolve; F.resolveArgs[0] = &R.accum.ptr; F.resolveArgs[1] = &F.out; F.resolveArgs[2] = &F.firstBatch; F.resolveArgs[3] = &F.lastBatch;
	}
	if (!EnqueueFrame(R, q, *sc.device, F, pend)) return false;
	pend.pixels = CoveredPixels(W, H, req.cellFirst, stride, numLocalCells);   // (counted while the device works)
	return true;
}

// The diagnostic builds' numbers behind a render (RL_DIAG_TIMELINE, RL_DIAG_TOPN) and RAYLIB_PRINT_STAMPS: cnt = the render's counter block on the host.
static bool PrintStamps(RankCtx& R, const unsigned long long* cnt)
{
	(void)R;
#ifdef RL_DIAG_TIMELINE
	if (getenv("RAYLIB_PRINT_STAMPS")) {
		std::vector<unsigned long long> tl(RL_TIMELINE_SLOTS);
		HIP_OK(hipMemcpy(tl.data(), R.counters.ptr + CNT_COUNT + 24, tl.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
		std::vector<double> st, ex, en;
		unsigned long long t0 = ~0ull;
		for (int w = 0; w < 8192; ++w) if (tl[w] && tl[w] < t0) t0 = tl[w];
		for (int w = 0; w < 8192; ++w) if (tl[w]) { st.push_back((tl[w] - t0) * 0.01); if (tl[8192 + w]) ex.push_back((tl[8192 + w] - t0) * 0.01); en.push_back((tl[16384 + w] - t0) * 0.01); }
		auto pct = [](std::vector<double>& v, double q) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return v[(size_t)(q * (v.size() - 1))]; };
		Log("timeline (us from the first wave's start; last launch, %d waves): start p50 %.1f max %.1f | queue seen empty min %.1f p50 %.1f max %.1f | end min %.1f p10 %.1f p50 %.1f p90 %.1f max %.1f",
			(int)st.size(), pct(st, 0.5), pct(st, 1.0), pct(ex, 0.0), pct(ex, 0.5), pct(ex, 1.0), pct(en, 0.0), pct(en, 0.1), pct(en, 0.5), pct(en, 0.9), pct(en, 1.0));
		for (unsigned x = 0; x < 8; ++x) {   // per XCD: which waves ran there, when they found the job list empty, when they ended
			std::vector<double> xe, xn;
			for (int w = 0; w < 8192; ++w) if (tl[w] && tl[24576 + w] == x) { if (tl[8192 + w]) xe.push_back((tl[8192 + w] - t0) * 0.01); xn.push_back((tl[16384 + w] - t0) * 0.01); }
			if (!xn.empty()) Log("   XCC %u: %d waves | job list seen empty min %.1f p50 %.1f max %.1f | end min %.1f p50 %.1f max %.1f", x, (int)xn.size(), pct(xe, 0.0), pct(xe, 0.5), pct(xe, 1.0), pct(xn, 0.0), pct(xn, 0.5), pct(xn, 1.0));
		}
	}
#endif
#ifdef RL_DIAG_TOPN
	if (getenv("RAYLIB_PRINT_STAMPS")) {
		const double n = (double)cnt[CNT_NODES] + 1e-9;
		Log("node steps by node number (breadth first): < 9: %.3f  < 22: %.3f  < 53: %.3f  < 73: %.3f  < 128: %.3f  < 256: %.3f  < 1024: %.3f  beyond: %.3f (cumulative shares of %.0f steps)",
		    cnt[CNT_COUNT + 4] / n, (cnt[CNT_COUNT + 4] + cnt[CNT_COUNT + 5]) / n, (cnt[CNT_COUNT + 4] + cnt[CNT_COUNT + 5] + cnt[CNT_COUNT + 6]) / n,
		    (cnt[CNT_COUNT + 4] + cnt[CNT_COUNT + 5] + cnt[CNT_COUNT + 6] + cnt[CNT_COUNT + 7]) / n, (cnt[CNT_COUNT + 4] + cnt[CNT_COUNT + 5] + cnt[CNT_COUNT + 6] + cnt[CNT_COUNT + 7] + cnt[CNT_COUNT + 8]) / n,
		    (cnt[CNT_COUNT + 4] + cnt[CNT_COUNT + 5] + cnt[CNT_COUNT + 6] + cnt[CNT_COUNT + 7] + cnt[CNT_COUNT + 8] + cnt[CNT_COUNT + 9]) / n,
		    (cnt[CNT_COUNT + 4] + cnt[CNT_COUNT + 5] + cnt[CNT_COUNT + 6] + cnt[CNT_COUNT + 7] + cnt[CNT_COUNT + 8] + cnt[CNT_COUNT + 9] + cnt[CNT_COUNT + 10]) / n, cnt[CNT_COUNT + 11] / n, n);
		Log("groups on the stack at a node step: 0: %.3f  1: %.3f  2: %.3f  3: %.3f  4: %.3f  5: %.3f  6-7: %.3f  8+: %.3f", cnt[CNT_COUNT + 16] / n, cnt[CNT_COUNT + 17] / n, cnt[CNT_COUNT + 18] / n,
		    cnt[CNT_COUNT + 19] / n, cnt[CNT_COUNT + 20] / n, cnt[CNT_COUNT + 21] / n, cnt[CNT_COUNT + 22] / n, cnt[CNT_COUNT + 23] / n);
	}
#else
	if (getenv("RAYLIB_PRINT_STAMPS")) {
		const double tot = (double)(cnt[CNT_COUNT] + cnt[CNT_COUNT + 1] + cnt[CNT_COUNT + 2] + cnt[CNT_COUNT + 3]);
		Log("wave steps: node %llu (lane steps %llu, eff %.3f)  tri %llu (lane %llu, eff %.3f)  leaf rounds %llu  trips %llu", cnt[CNT_COUNT + 4], cnt[CNT_NODES], cnt[CNT_NODES] / (64.0 * cnt[CNT_COUNT + 4] + 1), cnt[CNT_COUNT + 5], cnt[CNT_TRIS], cnt[CNT_TRIS] / (64.0 * cnt[CNT_COUNT + 5] + 1), cnt[CNT_COUNT + 6], cnt[CNT_TRIPS]);
#if defined(RL_DIAG_STAMPS) && RL_DIAG_STAMPS >= 2
		if (cnt[CNT_COUNT + 7]) Log("leaf list: %llu triangle wave steps taken; %llu if every round's (ray, triangle) pairs were dealt evenly to the wave's 64 lanes (the bound of any regrouping: a round cannot take less than one step)", cnt[CNT_COUNT + 5], cnt[CNT_COUNT + 7]);
#endif
		Log("diagnostic slots (wave level): [4] %llu [5] %llu [6] %llu [7] %llu [16] %llu [17] %llu [18] %llu [19] %llu trips %llu", cnt[CNT_COUNT + 4], cnt[CNT_COUNT + 5], cnt[CNT_COUNT + 6], cnt[CNT_COUNT + 7],
		    cnt[CNT_COUNT + 16], cnt[CNT_COUNT + 17], cnt[CNT_COUNT + 18], cnt[CNT_COUNT + 19], cnt[CNT_TRIPS]);
		if (tot > 0) Log("shade split (of all): surface+material %.3f scatter %.3f emit+store %.3f", cnt[CNT_COUNT + 8] / tot, cnt[CNT_COUNT + 9] / tot, cnt[CNT_COUNT + 10] / tot);
		if (tot > 0) Log("microfacet split (of all): setup %.3f beckmann sample %.3f brdf+pdf %.3f | newton wave iters %llu lane iters %llu (eff %.3f) | microfacet wave calls %llu lanes %llu (eff %.3f)", cnt[CNT_COUNT + 12] / tot, cnt[CNT_COUNT + 13] / tot, cnt[CNT_COUNT + 14] / tot, cnt[CNT_COUNT + 16], cnt[CNT_COUNT + 17], cnt[CNT_COUNT + 17] / (64.0 * cnt[CNT_COUNT + 16] + 1), cnt[CNT_COUNT + 18], cnt[CNT_COUNT + 19], cnt[CNT_COUNT + 19] / (64.0 * cnt[CNT_COUNT + 18] + 1));
		{
			static const char* nm[4] = { "traverse", "shade a hit", "miss shader", "fold + store" };
			for (int k = 0; k < 4; ++k) if (cnt[CNT_COUNT + 4 + k] && cnt[CNT_COUNT + 20 + k])
				Log("  %-12s clock share %.3f, lanes taking part %.3f (level-1 diagnostic build)", nm[k], cnt[CNT_COUNT + 4 + k] / tot, cnt[CNT_COUNT + 20 + k] / (64.0 * cnt[CNT_COUNT + 4 + k]));
		}
		if (tot > 0) Log("phase shares (shader clock): refill %.3f traverse %.3f shade %.3f fold %.3f", cnt[CNT_COUNT] / tot, cnt[CNT_COUNT + 1] / tot, cnt[CNT_COUNT + 2] / tot, cnt[CNT_COUNT + 3] / tot);
	}
#endif
	return true;
}

// The one host synchronisation of a rank's render, then its numbers.  Adds to `stats` (counters are summed over ranks, times
// are the slowest rank's).
bool FinishRender(RankCtx& R, PendingRender& pend, RaylibAMDStats& stats)
{
	const int q = pend.slot;
	HIP_OK(hipSetDevice(R.device));
	if (!pend.enqueuedToEnd) {
		// the enqueue failed half-way: whatever it did queue is waited for (the stream is drained whatever happened), there are no numbers to report
		(void)hipStreamSynchronize(R.stream);
		return false;
	}
	HIP_OK(hipEventSynchronize(R.ev[q][7]));   // this render's last operation on the rank's stream (a later frame may already be queued behind it)
	if (pend.lastBatchPending) {
		float ms = 0.0f;
		HIP_OK(hipEventElapsedTime(&ms, R.ev[q][2], R.ev[q][3]));
		pend.traceMs += ms;
	}
	float totalMs = 0.0f;
	HIP_OK(hipEventElapsedTime(&totalMs, R.ev[q][0], R.ev[q][1]));
	const unsigned long long* cnt = pend.cnt;
	stats.rays += cnt[CNT_RAYS]; stats.nodesVisited += cnt[CNT_NODES]; stats.trisTested += cnt[CNT_TRIS];
	stats.shadedHits += cnt[CNT_SHADED]; stats.texFetches += cnt[CNT_TEXELS]; stats.cameraSamples += cnt[CNT_SAMPLES];
	// camera samples of the cells outside the scene's silhouette (CullCells) were never generated or traced: they are reported next to the executed work, not in it
	// (each would have been one root-box query, two with a sun -- what the megakernel counts for a sample it decides at the root)
	stats.culledCells += pend.culledCells; stats.listedCells += pend.listedCells;
	stats.culledSamples += pend.culledSamples; stats.culledRays += pend.culledSamples * pend.culledRaysPerSample;
	stats.texFetches += pend.culledSamples * pend.culledSkyTexels;   // (k_resolve DOES look up the sky texel of every sample of a dropped cell: executed, counted)
	stats.waveTrips += cnt[CNT_TRIPS];
	if (pend.lazy) { stats.litPaths += cnt[CNT_COUNT + 24]; stats.litFoldedInPlace += cnt[CNT_COUNT + 24 + 1]; }
	stats.pathsPerWave = pend.pathsPerWave; stats.treeWidth = pend.treeWidth; stats.nodeBytes = pend.nodeBytes;
	stats.pixels += pend.pixels;
	stats.kernelMs = std::max(stats.kernelMs, (double)totalMs);
	stats.traceKernelMs = std::max(stats.traceKernelMs, (double)(pend.pathTrace ? pend.traceMs : totalMs));
	stats.traceLaunches = std::max(stats.traceLaunches, pend.pathTrace ? pend.launches : 1u);
	if (R.rank >= 0 && R.rank < 16) { stats.rankKernelMs[R.rank] = (double)totalMs; stats.rankTraceMs[R.rank] = (double)(pend.pathTrace ? pend.traceMs : totalMs); }
	if (pend.jobHeads) stats.jobHeads = pend.jobHeads;
	return PrintStamps(R, cnt);
}

// ---- several views of one scene (RaylibAMD_RenderViews): rank 0's device and stream, whatever RAYLIB_NUM_GPUS says, as a progressive session ----
// The batch's output is ONE buffer, view-major (view v's row-major frame at v * W * H); the images get theirs by device-to-device copies behind the
// resolve.  The cull's list and flags and the camera table go through buffers of their own: the one-view renders' cached lists (RankCtx::cullKey) are
// never those of a batch, nor the reverse.
struct ViewsBuffers {
	PinBuf<unsigned char> host;   // pinned staging: the camera table, the list of listed cells, the flags
	DevBuf<unsigned char> dev;
	DevBuf<float4> out;           // the library's own output (RaylibAMD_RenderViewsDevice with no buffer of the caller's, and the images')
};

bool DeviceRenderViews(Scene& sc, const RenderRequest& req, const DCamera* cameras, uint32_t count, void* outDevice, void* const* imagePixels, RaylibAMDStats& stats)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	static ViewsBuffers& B = *new ViewsBuffers;   // (kept for the process, as the runtime: rl_rt.h Runtime)
	const auto t0 = std::chrono::steady_clock::now();
	if (!EnsureRuntime() || count == 0 || count > RL_MAX_VIEWS) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (!UploadScene(sc) || !SyncSky(sc)) return false;
	(void)DrainLocked();            // rank 0's slot-0 events, counter block and work buffers
	Rt().deferredUnreported = false;   // (the numbers the caller reads next are this batch's)
	DeviceSceneCopy* D = sc.device->copy[(size_t)R.devSlot];
	const RendererSettings& st = req.settings;
	Frame F;
	F.knobs = ReadRenderKnobs();
	F.plan = PlanTrace(sc, st, D->view.sky != nullptr, F.knobs);
	if (!F.plan.ok || !TraceView(D, sc, F.plan, F.view)) return false;
	const uint32_t W = st.viewportWidth, H = st.viewportHeight;
	const uint32_t cellsPerView = ((W + 7) / 8) * ((H + 7) / 8), numCells = cellsPerView * count;
	const size_t viewBytes = (size_t)W * H * sizeof(float4);
	F.P = BaseParams(st, req.seed, cameras[0], 0, 1, numCells, false);   // (the twins read every view's camera from the table)
	F.numLive = F.numActive = numCells;
	F.sEnd = F.P.spp;

	// the batch's job list: all of it decided before anything is enqueued
	ViewsPlan VP;
	if (F.plan.pathTrace) {
		const void* traceKernel = KernelFor(F.plan, true);
		if (!traceKernel) { Log("RaylibAMD_RenderViews: no megakernel instance for STACK %d, K %d, stack in LDS %d", F.plan.stack, F.plan.poolK, F.plan.lstack); return false; }
		const int blocksPerCU = OccupancyOf(R, traceKernel, &F.plan);
		if (blocksPerCU < 0) return false;
		VP = PlanViews(SceneCullScene(sc, F.view.sky != nullptr), st, cameras, count, F.plan, R.numCUs, blocksPerCU, F.knobs);
		if (!VP.ok) { Log("RaylibAMD_RenderViews: job count overflow"); return false; }
		F.knobs = VP.knobs;   // (RAYLIB_SAMPLE_BATCH lowered where the job count needs it)
	}
	// the camera table, then (culled views) the list of listed cells and the flags, staged in pinned memory and copied in one go
	const size_t camBytes = (size_t)count * sizeof(DCamera), listAt = (camBytes + 255) & ~(size_t)255;
	const bool culled = F.plan.pathTrace && VP.numActive < numCells;
	const size_t flagsAt = listAt + (culled ? (size_t)numCells * sizeof(uint32_t) : 0), stageBytes = flagsAt + (culled ? numCells : 0);
	if (!B.host.Grow(stageBytes) || !B.dev.Grow(stageBytes)) return false;
	memcpy(B.host.ptr, cameras, camBytes);
	PendingRender pend;
	if (culled) {
		memcpy(B.host.ptr + listAt, VP.active.data(), VP.active.size() * sizeof(uint32_t));
		memcpy(B.host.ptr + flagsAt, VP.empty.data(), numCells);
		ListCells(F, pend, (const uint32_t*)(B.dev.ptr + listAt), (const uint8_t*)(B.dev.ptr + flagsAt), VP.numActive, numCells, VP.emptyL, VP.emptyPixels, VP.raysPerSample);
	}
	F.out = (float4*)outDevice;
	if (!F.out) { if (!B.out.Grow(viewBytes * count)) return false; F.out = B.out.ptr; }
	DViews V;
	V.cameras = (const DCamera*)B.dev.ptr; V.cellsPerView = cellsPerView;
	V.magicCellsPerView = cellsPerView > 1 ? (uint32_t)(0x100000000ull / cellsPerView) : 0xFFFFFFFFu;
	F.views = &V;
	F.resolve = (const void*)k_resolve_views;
	F.resolveArgs[0] = &R.accum.ptr; F.resolveArgs[1] = &F.out; F.resolveArgs[2] = &F.firstBatch; F.resolveArgs[3] = &F.lastBatch; F.resolveArgs[4] = &V;

	auto enqueue = [&]() -> bool {   // the staged tables, the frame, and behind it every image's copy of its view
		HIP_OK(hipMemcpyAsync(B.dev.ptr, B.host.ptr, stageBytes, hipMemcpyHostToDevice, R.stream));
		if (!BeginFrame(R, 0, F, viewBytes * count, pend) || !EnqueueFrame(R, 0, *sc.device, F, pend)) return false;
		if (imagePixels)
			for (uint32_t v = 0; v < count; ++v) HIP_OK(hipMemcpyAsync(imagePixels[v], (const char*)F.out + viewBytes * v, viewBytes, hipMemcpyDeviceToDevice, R.stream));
		pend.pixels = CoveredPixels(W, H, 0, 1, cellsPerView) * count;
		return true;
	};
	bool ok = enqueue();
	ok = FinishRender(R, pend, stats) && ok;
	HIP_OK(hipStreamSynchronize(R.stream));   // (the images' copies)
	OneRankStats(stats, sc);
	stats.wallMs = MsSince(t0);
	return ok;
}

} // namespace rl
