// Host runtime: rays of the caller's -- the ray queries (RaylibAMD_TraceRays, k_query) and path-traced radiance (RaylibAMD_TraceRadiance, k_radiance) on
// rank 0's device, from host memory or from device pointers, on the library's stream (synchronous, with stats) or enqueued on a stream of the caller's (rl_rt.h).
// The two entries share the refusals of a device call's pointers, the synchronous call's counter block and event pair, the stats' header, the staging of a
// host call through qRays / qOut, the grid that fills the device once, and the synchronous tail; each keeps its plan and kernel, its parameter block and the
// discipline of its scratch: a ring of ray counters with an event per slot for the queries, one counter and one path stack ordered by radEv for radiance.
#include "rl_rt.h"

namespace rl {

typedef void (*QueryKernel)(const DSceneView, const float4*, uint32_t, float, void*, int32_t*, const int32_t*, unsigned int*, unsigned long long*);
template <int KIND>
static QueryKernel QueryKernelOfKind(const QueryPlan& p)
{
	if (p.tree == TREE_WIDE8) return (QueryKernel)k_query<8, KIND, 2 * RL_POOL8_MAXLEVELS, false>;
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (QueryKernel)k_query<4, KIND, 32, false> : (QueryKernel)k_query<4, KIND, 64, false>;
	if (p.stack <= 32) return p.prims ? (QueryKernel)k_query<2, KIND, 32, true> : (QueryKernel)k_query<2, KIND, 32, false>;
	return p.prims ? (QueryKernel)k_query<2, KIND, 64, true> : (QueryKernel)k_query<2, KIND, 64, false>;
}
static_assert(RAYLIB_AMD_QUERY_ANY == RL_QK_ANY && RAYLIB_AMD_QUERY_CLOSEST == RL_QK_CLOSEST && RAYLIB_AMD_QUERY_SURFACE == RL_QK_SURFACE, "query kinds");
static_assert(sizeof(RaylibAMDRay) == 32 && sizeof(RaylibAMDHitT) == sizeof(DQueryHit) && sizeof(DHitOut) == 44, "query records");

typedef void (*RadianceKernel)(const DSceneView, const SkyRot, const DRadianceParams, const float4*, uint32_t, float4*, float*, unsigned int*, unsigned long long*);
static RadianceKernel RadianceKernelFor(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (RadianceKernel)k_radiance<4, 32, false> : (RadianceKernel)k_radiance<4, 64, false>;
	if (p.stack <= 32) return p.prims ? (RadianceKernel)k_radiance<2, 32, true> : (RadianceKernel)k_radiance<2, 32, false>;
	return p.prims ? (RadianceKernel)k_radiance<2, 64, true> : (RadianceKernel)k_radiance<2, 64, false>;
}
static_assert(sizeof(RaylibAMDPathRay) == sizeof(RaylibAMDRay), "radiance records");
static_assert(RL_RADIANCE_STACK_BUDGET / ((uint64_t)RL_RADIANCE_MAX_PATH * 8 * sizeof(float) * RL_BLOCK) >= 1, "one workgroup's path stack fits the budget");

// a device pointer a call may use: memory of rank 0's device
static bool OnDevice(const void* p, int device)
{
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
	return (a.type == hipMemoryTypeDevice || a.isManaged) && a.device == device;
}
// The refusals of a device call (`api`): every pointer is memory of the device; the kernels read a ray as two 16-byte loads and write a 16-byte result as one
// store (outAlign 15), the other records as 4-byte words (3).  outPrim, when given, is checked as device memory only where the call writes it (primUsed).
static bool DevicePointersOk(const char* api, int device, const void* rays, const void* out, uintptr_t outAlign, const void* outPrim, bool primUsed)
{
	if (!OnDevice(rays, device) || !OnDevice(out, device) || (outPrim && primUsed && !OnDevice(outPrim, device))) {
		Log("%s: a pointer is not device memory of device %d", api, device);
		return false;
	}
	if (((uintptr_t)rays & 15u) != 0) { Log("%s: the rays are not 16-byte aligned", api); return false; }
	if (((uintptr_t)out & outAlign) != 0 || ((uintptr_t)outPrim & 3u) != 0) { Log("%s: the output is not %u-byte aligned", api, (unsigned)outAlign + 1u); return false; }
	return true;
}

// a synchronous call's counter block, its pinned copy and the event pair around its kernel: made when the first such call needs them
static bool EnsureSyncStats(RankCtx& R)
{
	if (R.qStats.ptr) return true;
	if (!R.qStats.Grow(8 * sizeof(unsigned long long)) || !R.qStatsHost.Grow(8 * sizeof(unsigned long long))) return false;
	HIP_OK(hipEventCreate(&R.qEv[0])); HIP_OK(hipEventCreate(&R.qEv[1]));
	return true;
}
// what a call reports whether it has rays or not
static void StatsHeader(RaylibAMDStats& stats, const QueryPlan& plan, const Scene& sc)
{
	memset(&stats, 0, sizeof(stats));
	stats.treeWidth = plan.treeWidth; stats.nodeBytes = plan.nodeBytes;
	OneRankStats(stats, sc);
}
// a host call's rays (n records of 32 bytes) into the rank's staging buffer, behind whatever `st` holds; its results go through qOut
static bool StageRays(RankCtx& R, const void* rays, int32_t n, size_t outBytes, hipStream_t st)
{
	if (!R.qRays.Grow((size_t)n * sizeof(RaylibAMDRay)) || !R.qOut.Grow(outBytes)) return false;
	HIP_OK(hipMemcpyAsync(R.qRays.ptr, rays, (size_t)n * sizeof(RaylibAMDRay), hipMemcpyHostToDevice, st));
	return true;
}
// enough workgroups to fill the device once (the waves take their work from a counter: rl_k_query.inl, rl_k_radiance.inl); 0: the occupancy query failed (logged)
static uint64_t FillingGrid(RankCtx& R, const void* kernel, int32_t n)
{
	const int blocksPerCU = OccupancyOf(R, kernel);
	if (blocksPerCU < 0) return 0;
	return std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)R.numCUs * (uint64_t)std::max(1, blocksPerCU), ((uint64_t)n + RL_BLOCK - 1) / RL_BLOCK));
}
// A synchronous call on `st`, around its launch: the counters cleared and the first event in front of the kernel ...
static bool BeginSync(RankCtx& R, hipStream_t st)
{
	HIP_OK(hipMemsetAsync(R.qStats.ptr, 0, 8 * sizeof(unsigned long long), st));
	HIP_OK(hipEventRecord(R.qEv[0], st));
	return true;
}
// ... and behind it the second event, the counters and a host call's results (`back`: those with a host address) on their way to the host, the one wait, the numbers
struct CopyBack { void* host; const void* dev; size_t bytes; };
static bool FinishSync(RankCtx& R, hipStream_t st, std::initializer_list<CopyBack> back, std::chrono::steady_clock::time_point t0, RaylibAMDStats& stats)
{
	HIP_OK(hipEventRecord(R.qEv[1], st));
	HIP_OK(hipMemcpyAsync(R.qStatsHost.ptr, R.qStats.ptr, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	for (const CopyBack& b : back) if (b.host) HIP_OK(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	float ms = 0.0f;
	HIP_OK(hipEventElapsedTime(&ms, R.qEv[0], R.qEv[1]));
	const unsigned long long* cnt = R.qStatsHost.ptr;   // (k_query leaves the last two at 0)
	stats.rays = cnt[CNT_RAYS]; stats.nodesVisited = cnt[CNT_NODES]; stats.trisTested = cnt[CNT_TRIS];
	stats.shadedHits = cnt[CNT_SHADED]; stats.texFetches = cnt[CNT_TEXELS]; stats.cameraSamples = cnt[CNT_SAMPLES]; stats.waveTrips = cnt[CNT_TRIPS];
	stats.kernelMs = ms; stats.traceKernelMs = ms; stats.traceLaunches = 1;
	stats.wallMs = MsSince(t0);
	return true;
}

bool DeviceTraceRays(Scene& sc, int32_t kind, const void* rays, int32_t n, float rayTime, void* out, int32_t* outPrim, bool hostMem, void* stream,
                     RaylibAMDStats& stats)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	const QueryPlan plan = PlanQuery(sc, kind, ReadRenderKnobs());
	if (!plan.ok) { Log("RaylibAMD_TraceRays: BVH depth %u exceeds the traversal stack (64)", sc.bvh.depth); return false; }
	const size_t outBytes = (size_t)n * (kind == RAYLIB_AMD_QUERY_ANY ? sizeof(uint32_t) : kind == RAYLIB_AMD_QUERY_CLOSEST ? sizeof(DQueryHit) : sizeof(DHitOut));
	if (!hostMem && n > 0 && !DevicePointersOk("RaylibAMD_TraceRaysDevice", R.device, rays, out, kind == RAYLIB_AMD_QUERY_CLOSEST ? 15u : 3u, outPrim, kind == RAYLIB_AMD_QUERY_SURFACE)) return false;
	if (!UploadScene(sc)) return false;
	DeviceSceneCopy* Cp = sc.device->copy[(size_t)R.devSlot];
	if (!EnsureWideTree(Cp, sc, plan.tree)) return false;
	const bool wantPrim = kind == RAYLIB_AMD_QUERY_CLOSEST || (kind == RAYLIB_AMD_QUERY_SURFACE && outPrim);
	if (wantPrim && !Cp->slotIndex.ptr && !sc.bvh.triOrder.empty()) {
		std::vector<int32_t> idx(sc.bvh.triOrder.begin(), sc.bvh.triOrder.end());
		if (!Cp->slotIndex.Upload(idx.data(), idx.size())) { Cp->slotIndex.Free(); return false; }
	}
	const hipStream_t st = stream ? (hipStream_t)stream : R.stream;
	const bool sync = !stream;
	if (!R.qRing.ptr) {
		if (!R.qRing.Grow(RL_QUERY_RING * sizeof(unsigned int))) return false;
		for (int k = 0; k < RL_QUERY_RING; ++k) HIP_OK(hipEventCreateWithFlags(&R.qRingEv[k], hipEventDisableTiming));
	}
	const uint32_t slot = R.qRingNext;
	if (R.qRingUsed[slot]) HIP_OK(hipEventSynchronize(R.qRingEv[slot]));   // RL_QUERY_RING launches ago: long done, unless a caller's stream is that far behind
	unsigned int* counter = R.qRing.ptr + slot;
	if (sync && !EnsureSyncStats(R)) return false;
	StatsHeader(stats, plan, sc);
	if (n == 0) return true;
	const float4* dRays = (const float4*)rays; void* dOut = out; int32_t* dPrim = (kind == RAYLIB_AMD_QUERY_SURFACE) ? outPrim : nullptr;
	if (hostMem) {
		if (dPrim && !R.qPrim.Grow((size_t)n * sizeof(int32_t))) return false;
		if (!StageRays(R, rays, n, outBytes, st)) return false;
		dRays = R.qRays.ptr; dOut = R.qOut.ptr; if (dPrim) dPrim = R.qPrim.ptr;
	}
	const QueryKernel kernel = kind == RAYLIB_AMD_QUERY_ANY ? QueryKernelOfKind<RL_QK_ANY>(plan) : kind == RAYLIB_AMD_QUERY_CLOSEST ? QueryKernelOfKind<RL_QK_CLOSEST>(plan)
	                         : QueryKernelOfKind<RL_QK_SURFACE>(plan);
	const uint32_t blocks = (uint32_t)FillingGrid(R, (const void*)kernel, n);
	if (!blocks) return false;
	const DSceneView view = Cp->view;
	HIP_OK(hipMemsetAsync(counter, 0, sizeof(unsigned int), st));
	if (sync && !BeginSync(R, st)) return false;
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RL_BLOCK), 0, st, view, dRays, (uint32_t)n, rayTime, dOut, dPrim, Cp->slotIndex.ptr, counter, sync ? R.qStats.ptr : nullptr);
	HIP_OK(hipGetLastError());
	HIP_OK(hipEventRecord(R.qRingEv[slot], st));
	R.qRingUsed[slot] = true;
	R.qRingNext = (slot + 1u) % RL_QUERY_RING;
	if (!sync) return true;
	return FinishSync(R, st, { { hostMem ? out : nullptr, dOut, outBytes }, { hostMem && dPrim ? outPrim : nullptr, dPrim, (size_t)n * sizeof(int32_t) } }, t0, stats);
}

bool DeviceTraceRadiance(Scene& sc, const RaylibAMDRadianceParams& prm, uint64_t seed, const void* rays, int32_t n, float* out, bool hostMem, void* stream,
                         RaylibAMDStats& stats)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	const QueryPlan plan = PlanRadiance(sc, ReadRenderKnobs());
	if (!plan.ok) { Log("RaylibAMD_TraceRadiance: BVH depth %u exceeds the traversal stack (64)", sc.bvh.depth); return false; }
	if (!hostMem && n > 0 && !DevicePointersOk("RaylibAMD_TraceRadianceDevice", R.device, rays, out, 15u, nullptr, false)) return false;
	if (!UploadScene(sc) || !SyncSky(sc)) return false;
	DeviceSceneCopy* Cp = sc.device->copy[(size_t)R.devSlot];
	if (!EnsureWideTree(Cp, sc, plan.tree)) return false;
	const hipStream_t st = stream ? (hipStream_t)stream : R.stream;
	const bool sync = !stream;
	if (!R.radCounter.Grow(sizeof(unsigned int))) return false;
	if (!R.radEv) HIP_OK(hipEventCreateWithFlags(&R.radEv, hipEventDisableTiming));
	if (sync && !EnsureSyncStats(R)) return false;
	StatsHeader(stats, plan, sc);
	if (n == 0) return true;
	const RadianceKernel kernel = RadianceKernelFor(plan);
	uint64_t blocks64 = FillingGrid(R, (const void*)kernel, n);
	if (!blocks64) return false;
	// ... but no more than whose path stack (32 bytes per bounce and resident lane) fits RL_RADIANCE_STACK_BUDGET: long paths run on a smaller grid,
	// which changes no result (a job's arithmetic does not depend on the lane that takes it)
	const size_t depthSlots = (size_t)(prm.maxPathLength > 1 ? prm.maxPathLength : 1);
	const uint64_t stackPerBlock = (uint64_t)depthSlots * 8 * sizeof(float) * RL_BLOCK;
	blocks64 = std::min<uint64_t>(blocks64, RL_RADIANCE_STACK_BUDGET / stackPerBlock);   // (>= 1: RaylibAMD_TraceRadiance refuses a longer path)
	const uint32_t blocks = (uint32_t)blocks64;
	DRadianceParams Q; memset(&Q, 0, sizeof(Q));
	Q.seedMixed = raylib_rng_mix64(seed); Q.maxPathLength = prm.maxPathLength; Q.rayTMin = prm.rayTMin;
	Q.sampleFirst = prm.sampleFirst; Q.sampleCount = prm.sampleCount; Q.skipDraws = prm.skipDraws;
	Q.stackStride = blocks * RL_BLOCK; Q.timeMin = prm.timeMin; Q.timeMax = prm.timeMax;
	// the path stack of the grid: one record per bounce and resident lane.  The scratch is one per rank: a launch waits, on its stream, for the launch before it
	// (whatever stream that ran on), and growing the stack frees it with hipFree, which waits for the device
	if (!R.radStack.Grow(depthSlots * 8 * Q.stackStride * sizeof(float))) return false;
	const float4* dRays = (const float4*)rays; float4* dOut = (float4*)out;
	const size_t outBytes = (size_t)n * sizeof(float4);
	if (hostMem) {
		if (!StageRays(R, rays, n, outBytes, st)) return false;
		dRays = R.qRays.ptr; dOut = (float4*)R.qOut.ptr;
	}
	const DSceneView view = Cp->view;
	const SkyRot skyRot = sc.device->skyRot;
	if (R.radEvUsed) HIP_OK(hipStreamWaitEvent(st, R.radEv, 0));
	HIP_OK(hipMemsetAsync(R.radCounter.ptr, 0, sizeof(unsigned int), st));
	if (sync && !BeginSync(R, st)) return false;
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RL_BLOCK), 0, st, view, skyRot, Q, dRays, (uint32_t)n, dOut, R.radStack.ptr, R.radCounter.ptr, sync ? R.qStats.ptr : nullptr);
	HIP_OK(hipGetLastError());
	HIP_OK(hipEventRecord(R.radEv, st));
	R.radEvUsed = true;
	if (!sync) return true;
	return FinishSync(R, st, { { hostMem ? out : nullptr, dOut, outBytes } }, t0, stats);
}

} // namespace rl
