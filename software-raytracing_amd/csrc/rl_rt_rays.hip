// Host runtime: calls on rays, points and triangles of the caller's, on rank 0's device -- from host memory or from device pointers, on the library's stream
// (synchronous, with stats) or enqueued on a stream of the caller's (rl_host.h).  Three families and what they share:
//   The queries -- the camera's G-buffer, ray, ordered multi-hit, nearest-point, K-nearest, swept-sphere and triangle-overlap queries with their contacts -- are one call (RunQuery) that each entry
//   describes by data (QueryDesc: plan, kernel, input records, outputs, dynamic LDS) and gives its launch; a distance-field bake is several launches on the
//   same pieces.  Their scratch is a ring of work counters with an event per slot (LaunchOnRing).
//   The path calls -- radiance along caller rays, and the gathers, which are that call with another generator -- share BeginPathCall and PathGrid, one counter
//   and one path stack ordered by radEv.  A plain and an adaptive gather are one driver (GatherLocked): one prologue, one launch -- counter, event pair,
//   k_gather, the launch's resolve --, one tail; a plain call loops over its cut's launches, an adaptive call over its passes of a shrinking, compacted set.
//   The plane calls -- the temporal accumulations and the variance-guided filter: planes in, planes out, no scene, no plan, no work counter -- are one call
//   (RunPlanes) that each entry describes by data (PlaneCall: the planes read and written) and gives what it prepares and what it launches.
//   All share the refusals of a device call's pointers (DevicePointersOk), the staging of a host call through qRays / qOut (StageOutputs), and a synchronous
//   call's counter block, event pair and tail (BeginSync, FinishSync); the first two also the grid that fills the device once (FillingGrid) and the stats' header.
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

typedef void (*NearestKernel)(const DSceneView, const float4*, uint32_t, void*, const int32_t*, unsigned int*, unsigned long long*);
template <int KIND>
static NearestKernel NearestKernelOfKind(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (NearestKernel)k_nearest<4, KIND, 32> : (NearestKernel)k_nearest<4, KIND, 64>;
	return p.stack <= 32 ? (NearestKernel)k_nearest<2, KIND, 32> : (NearestKernel)k_nearest<2, KIND, 64>;
}
static_assert(RAYLIB_AMD_NEAREST_WITHIN == RL_NK_WITHIN && RAYLIB_AMD_NEAREST_CLOSEST == RL_NK_CLOSEST, "nearest kinds");
static_assert(sizeof(RaylibAMDNearestQuery) == 16 && sizeof(RaylibAMDNearestHit) == sizeof(DNearestHit), "nearest records");

typedef void (*SweepKernel)(const DSceneView, const float4*, uint32_t, void*, const int32_t*, unsigned int*, unsigned long long*);
template <int KIND>
static SweepKernel SweepKernelOfKind(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (SweepKernel)k_sweep<4, KIND, 32> : (SweepKernel)k_sweep<4, KIND, 64>;
	return p.stack <= 32 ? (SweepKernel)k_sweep<2, KIND, 32> : (SweepKernel)k_sweep<2, KIND, 64>;
}
static_assert(RAYLIB_AMD_SWEEP_ANY == RL_SK_ANY && RAYLIB_AMD_SWEEP_CLOSEST == RL_SK_CLOSEST, "sweep kinds");
static_assert(sizeof(RaylibAMDSweepQuery) == 32 && sizeof(RaylibAMDSweepHit) == 32 && sizeof(RaylibAMDSweepHit) == sizeof(DSweepHit), "sweep records");

typedef void (*OverlapKernel)(const DSceneView, const float4*, uint32_t, uint32_t, uint32_t, void*, uint32_t*, const int32_t*, unsigned int*, unsigned long long*);
template <int KIND>
static OverlapKernel OverlapKernelOfKind(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (OverlapKernel)k_overlap<4, KIND, 32> : (OverlapKernel)k_overlap<4, KIND, 64>;
	return p.stack <= 32 ? (OverlapKernel)k_overlap<2, KIND, 32> : (OverlapKernel)k_overlap<2, KIND, 64>;
}
static_assert(RAYLIB_AMD_OVERLAP_ANY == RL_OK_ANY && RAYLIB_AMD_OVERLAP_LIST == RL_OK_LIST && RAYLIB_AMD_OVERLAP_SKIP_SHARED == RL_OVERLAP_SKIP_SHARED, "overlap kinds and flags");
static_assert(sizeof(RaylibAMDOverlapQuery) == 48 && RAYLIB_AMD_MAX_OVERLAPS == RL_MAX_OVERLAPS, "overlap records");
typedef void (*OverlapContactsKernel)(const DSceneView, const float4*, uint32_t, uint32_t, uint32_t, void*, uint32_t*, const int32_t*, unsigned int*, unsigned long long*, float4*,
                                      const int32_t*);
static OverlapContactsKernel OverlapContactsKernelOf(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (OverlapContactsKernel)k_overlap_contacts<4, 32> : (OverlapContactsKernel)k_overlap_contacts<4, 64>;
	return p.stack <= 32 ? (OverlapContactsKernel)k_overlap_contacts<2, 32> : (OverlapContactsKernel)k_overlap_contacts<2, 64>;
}
static_assert(sizeof(RaylibAMDContact) == 2 * sizeof(float4), "contact records");

typedef void (*OverlapBoxKernel)(const DSceneView, const float4*, uint32_t, uint32_t, void*, uint32_t*, const int32_t*, unsigned int*, unsigned long long*);
template <int KIND>
static OverlapBoxKernel OverlapBoxKernelOfKind(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (OverlapBoxKernel)k_overlap_box<4, KIND, 32> : (OverlapBoxKernel)k_overlap_box<4, KIND, 64>;
	return p.stack <= 32 ? (OverlapBoxKernel)k_overlap_box<2, KIND, 32> : (OverlapBoxKernel)k_overlap_box<2, KIND, 64>;
}
static_assert(RAYLIB_AMD_BOX_ANY == RL_BK_ANY && RAYLIB_AMD_BOX_LIST == RL_BK_LIST && RAYLIB_AMD_BOX_MARK == RL_BK_MARK, "box kinds");
static_assert(sizeof(RaylibAMDBoxQuery) == 64, "box records");

typedef void (*RadianceKernel)(const DSceneView, const SkyRot, const DRadianceParams, const float4*, uint32_t, float4*, float*, unsigned int*, unsigned long long*);
static RadianceKernel RadianceKernelFor(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (RadianceKernel)k_radiance<4, 32, false> : (RadianceKernel)k_radiance<4, 64, false>;
	if (p.stack <= 32) return p.prims ? (RadianceKernel)k_radiance<2, 32, true> : (RadianceKernel)k_radiance<2, 32, false>;
	return p.prims ? (RadianceKernel)k_radiance<2, 64, true> : (RadianceKernel)k_radiance<2, 64, false>;
}
static_assert(sizeof(RaylibAMDPathRay) == sizeof(RaylibAMDRay), "radiance records");
typedef void (*GatherKernel)(const DSceneView, const SkyRot, const DRadianceParams, const float4*, uint32_t, const DGatherJobs, float4*, float*, unsigned int*, unsigned long long*);
template <int GEN>
static GatherKernel GatherKernelOfKind(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (GatherKernel)k_gather<4, 32, false, GEN> : (GatherKernel)k_gather<4, 64, false, GEN>;
	if (p.stack <= 32) return p.prims ? (GatherKernel)k_gather<2, 32, true, GEN> : (GatherKernel)k_gather<2, 32, false, GEN>;
	return p.prims ? (GatherKernel)k_gather<2, 64, true, GEN> : (GatherKernel)k_gather<2, 64, false, GEN>;
}
typedef void (*GatherResolveKernel)(const float4*, uint32_t, uint32_t, float*, float*, int, int, uint32_t);
static_assert(RAYLIB_AMD_GATHER_IRRADIANCE + 1 == RL_GEN_HEMISPHERE && RAYLIB_AMD_GATHER_SH9 + 1 == RL_GEN_SPHERE, "gather kinds");
static_assert(sizeof(RaylibAMDGatherPoint) == sizeof(RaylibAMDRay), "gather records");
static_assert(RL_RADIANCE_STACK_BUDGET / ((uint64_t)RL_RADIANCE_MAX_PATH * 8 * sizeof(float) * RL_BLOCK) >= 1, "one workgroup's path stack fits the budget");

typedef void (*QueryAllKernel)(const DSceneView, const float4*, uint32_t, uint32_t, float4*, uint32_t*, const int32_t*, unsigned int*, unsigned long long*);
template <bool COUNT>
static QueryAllKernel QueryAllKernelOf(const QueryPlan& p)
{
	if (p.tree == TREE_WIDE8) return (QueryAllKernel)k_query_all<8, 2 * RL_POOL8_MAXLEVELS, COUNT>;
	return p.stack <= 32 ? (QueryAllKernel)k_query_all<2, 32, COUNT> : (QueryAllKernel)k_query_all<2, 64, COUNT>;
}
static_assert(RAYLIB_AMD_MAX_HITS == RL_MAX_HITS, "multi-hit capacity");
typedef void (*NearestAllKernel)(const DSceneView, const float4*, uint32_t, uint32_t, float4*, uint32_t*, const int32_t*, unsigned int*, unsigned long long*);
template <bool COUNT>
static NearestAllKernel NearestAllKernelOf(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (NearestAllKernel)k_nearest_all<4, 32, COUNT> : (NearestAllKernel)k_nearest_all<4, 64, COUNT>;
	return p.stack <= 32 ? (NearestAllKernel)k_nearest_all<2, 32, COUNT> : (NearestAllKernel)k_nearest_all<2, 64, COUNT>;
}
static_assert(RAYLIB_AMD_MAX_NEAREST == RL_MAX_NEAREST, "K-nearest capacity");
typedef void (*SdfRowsKernel)(const DSceneView, const DSdfGrid, uint32_t, uint32_t*, unsigned int*, unsigned long long*);
static SdfRowsKernel SdfRowsKernelOf(const QueryPlan& p)
{
	if (p.tree == TREE_WIDE8) return (SdfRowsKernel)k_sdf_rows<8, 2 * RL_POOL8_MAXLEVELS>;
	return p.stack <= 32 ? (SdfRowsKernel)k_sdf_rows<2, 32> : (SdfRowsKernel)k_sdf_rows<2, 64>;
}
typedef void (*SdfDistKernel)(const DSceneView, const DSdfGrid, float*, int32_t*, const uint32_t*, const int32_t*, unsigned int*, unsigned long long*);
template <bool SIGNED>
static SdfDistKernel SdfDistKernelOf(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (SdfDistKernel)k_sdf_dist<4, 32, SIGNED> : (SdfDistKernel)k_sdf_dist<4, 64, SIGNED>;
	return p.stack <= 32 ? (SdfDistKernel)k_sdf_dist<2, 32, SIGNED> : (SdfDistKernel)k_sdf_dist<2, 64, SIGNED>;
}

// a device pointer a call may use: memory of rank 0's device
bool OnDevice(const void* p, int device)
{
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
	return (a.type == hipMemoryTypeDevice || a.isManaged) && a.device == device;
}
// An output of a call: the caller's pointer; the bytes the call writes there (0: it writes none -- the pointer was not given, or is not this kind's); the mask
// of its alignment (15: records stored as one 16-byte word, 3: 4-byte words); the rank's buffer a host call stages it through; and, once StageOutputs has run,
// the device pointer the kernel gets (null for an output that is not written).
#define RL_QUERY_OUTS 7   /* the outputs a call may have: a G-buffer's planes (most calls have one to three) */
struct QueryOut { void* user = nullptr; size_t bytes = 0; uintptr_t align = 3u; DevBuf<void> RankCtx::* stage = nullptr; void* dev = nullptr; };
// An input of a call: the caller's pointer; the bytes the call reads there (0: none -- such an input is not checked, not staged, and null on the device); the
// mask of its alignment (15: the kernels read it as 16-byte loads, 7: as 8-byte pairs, 3: as 4-byte words).
struct CallIn { const void* user = nullptr; size_t bytes = 0; uintptr_t align = 15u; };
// The refusals of a device call (`api`): every input the call reads (`what` names a query's records; null: planes) and every output it writes are memory of
// the device; every input read is aligned as the kernels load it; every output pointer given, written or not, is aligned as its records are stored.
static bool DevicePointersOk(const char* api, const char* what, int device, const CallIn* ins, size_t numIns, const QueryOut* outs, size_t numOuts)
{
	bool onDevice = true;
	for (size_t k = 0; k < numIns; ++k) if (ins[k].bytes && !OnDevice(ins[k].user, device)) onDevice = false;
	for (size_t k = 0; k < numOuts; ++k) if (outs[k].bytes && !OnDevice(outs[k].user, device)) onDevice = false;
	if (!onDevice) { Log("%s: a pointer is not device memory of device %d", api, device); return false; }
	for (size_t k = 0; k < numIns; ++k) {
		if (!ins[k].bytes || ((uintptr_t)ins[k].user & ins[k].align) == 0) continue;
		if (what) Log("%s: the %s are not %u-byte aligned", api, what, (unsigned)ins[k].align + 1u);
		else Log("%s: an input plane is not %u-byte aligned", api, (unsigned)ins[k].align + 1u);
		return false;
	}
	for (size_t k = 0; k < numOuts; ++k)
		if (((uintptr_t)outs[k].user & outs[k].align) != 0) { Log("%s: the output is not %u-byte aligned", api, (unsigned)outs[k].align + 1u); return false; }
	return true;
}
// where the kernel writes each output: the caller's memory, or, for a host call, the staging buffer grown to it
static bool StageOutputs(RankCtx& R, QueryOut* outs, size_t numOuts, bool hostMem)
{
	for (size_t k = 0; k < numOuts; ++k) {
		QueryOut& o = outs[k];
		o.dev = o.bytes ? o.user : nullptr;
		if (!o.bytes || !hostMem) continue;
		if (!(R.*o.stage).Grow(o.bytes)) return false;
		o.dev = (R.*o.stage).ptr;
	}
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
// a host path call's rays or points (n records of 32 bytes) into the rank's staging buffer, behind whatever `st` holds; its results go through qOut
static bool StageRays(RankCtx& R, const void* rays, int32_t n, size_t outBytes, hipStream_t st)
{
	if (!R.qRays.Grow((size_t)n * sizeof(RaylibAMDRay)) || !R.qOut.Grow(outBytes)) return false;
	HIP_OK(hipMemcpyAsync(R.qRays.ptr, rays, (size_t)n * sizeof(RaylibAMDRay), hipMemcpyHostToDevice, st));
	return true;
}
// triangle slot -> index in the scene's triangle order, on the device when a call first needs it
static bool EnsureSlotIndex(DeviceSceneCopy* Cp, const Scene& sc)
{
	if (Cp->slotIndex.ptr || sc.bvh.triOrder.empty()) return true;
	std::vector<int32_t> idx(sc.bvh.triOrder.begin(), sc.bvh.triOrder.end());
	if (!Cp->slotIndex.Upload(idx.data(), idx.size())) { Cp->slotIndex.Free(); return false; }
	return true;
}
// its inverse, index in the scene's triangle order -> triangle slot, for the call that reads a listed triangle again (the contacts kind of k_overlap)
static bool EnsureExportSlot(DeviceSceneCopy* Cp, const Scene& sc)
{
	if (Cp->exportSlot.ptr || sc.bvh.triOrder.empty()) return true;
	const size_t m = sc.bvh.triOrder.size();
	std::vector<int32_t> inv(m, 0);
	for (size_t slot = 0; slot < m; ++slot) {
		const size_t k = (size_t)sc.bvh.triOrder[slot];
		if (k >= m) { Log("RaylibAMD_OverlapContacts: triangle slot %zu names triangle %zu of %zu", slot, k, m); return false; }
		inv[k] = (int32_t)slot;
	}
	if (!Cp->exportSlot.Upload(inv.data(), inv.size())) { Cp->exportSlot.Free(); return false; }
	return true;
}
// The ring of work counters the queries' launches take in turn: the next slot, free again (RL_QUERY_RING launches ago: long done, unless a caller's stream is that
// far behind) ...
static bool TakeRingCounter(RankCtx& R, uint32_t& slot)
{
	if (!R.qRing.ptr) {
		if (!R.qRing.Grow(RL_QUERY_RING * sizeof(unsigned int))) return false;
		for (int k = 0; k < RL_QUERY_RING; ++k) HIP_OK(hipEventCreateWithFlags(&R.qRingEv[k], hipEventDisableTiming));
	}
	slot = R.qRingNext;
	if (R.qRingUsed[slot]) HIP_OK(hipEventSynchronize(R.qRingEv[slot]));
	return true;
}
// ... and one launch on it: the counter cleared on `st`, what `launch` enqueues there (it gets the counter; false: it failed, and said so), the launch's error,
// and the event behind it, with which the slot is the ring's last
template <typename Launch>
static bool LaunchOnRing(RankCtx& R, uint32_t slot, hipStream_t st, Launch launch)
{
	unsigned int* counter = R.qRing.ptr + slot;
	HIP_OK(hipMemsetAsync(counter, 0, sizeof(unsigned int), st));
	if (!launch(counter)) return false;
	HIP_OK(hipGetLastError());
	HIP_OK(hipEventRecord(R.qRingEv[slot], st));
	R.qRingUsed[slot] = true;
	R.qRingNext = (slot + 1u) % RL_QUERY_RING;
	return true;
}
// Enough workgroups to fill the device once (the waves take their work from a counter: rl_k_query.inl, rl_k_radiance.inl), n jobs at most a lane each; 0: refused
// or failed (logged).  A kernel without dynamic LDS is asked for its occupancy once; with `ldsBytes` of it the answer depends on the call (`api`), which is
// refused when no workgroup fits.
static uint64_t FillingGrid(RankCtx& R, const void* kernel, uint64_t n, size_t ldsBytes = 0, const char* api = "")
{
	int blocksPerCU = 0;
	if (!ldsBytes) {
		blocksPerCU = OccupancyOf(R, kernel);
		if (blocksPerCU < 0) return 0;
		blocksPerCU = std::max(1, blocksPerCU);
	} else {
		HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocksPerCU, kernel, RL_BLOCK, ldsBytes));
		if (blocksPerCU < 1) { Log("%s: no workgroup of the kernel fits a compute unit with %zu bytes of list", api, ldsBytes); return 0; }
	}
	return std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)R.numCUs * (uint64_t)blocksPerCU, (n + RL_BLOCK - 1) / RL_BLOCK));
}
// A synchronous call on `st`, around its launch: the counters cleared and the first event in front of the kernel ...
static bool BeginSync(RankCtx& R, hipStream_t st)
{
	HIP_OK(hipMemsetAsync(R.qStats.ptr, 0, 8 * sizeof(unsigned long long), st));
	HIP_OK(hipEventRecord(R.qEv[0], st));
	return true;
}
// ... and behind it the second event, the counters and a host call's results (`back`: those with a host address) on their way to the host, the one wait, the numbers
struct CopyBack {
	void* host; const void* dev; size_t bytes;
	CopyBack(void* host_, const void* dev_, size_t bytes_) : host(host_), dev(dev_), bytes(bytes_) {}
	CopyBack(const QueryOut& o, bool hostMem) : host(hostMem && o.bytes ? o.user : nullptr), dev(o.dev), bytes(o.bytes) {}   // (only an output the caller gave)
};
static bool FinishSync(RankCtx& R, hipStream_t st, const std::vector<CopyBack>& back, std::chrono::steady_clock::time_point t0, RaylibAMDStats& stats)
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

// What a query and a distance-field bake do between the refusals of their pointers and their first enqueue: the scene on the device (which orders the call
// behind a move and behind multi-rank frames in flight), the plan's tree and, where the call writes export indices, the slot table; the stream; the ring's next
// counter; a synchronous call's counter block; the stats' header.
struct QueryCall { DeviceSceneCopy* Cp = nullptr; hipStream_t st = nullptr; bool sync = false; uint32_t slot = 0; };
static bool BeginQueryCall(Scene& sc, RankCtx& R, const QueryPlan& plan, bool wantSlotIndex, void* stream, QueryCall& U, RaylibAMDStats& stats)
{
	if (!UploadScene(sc)) return false;
	U.Cp = sc.device->copy[(size_t)R.devSlot];
	if (!EnsureWideTree(U.Cp, sc, plan.tree)) return false;
	if (wantSlotIndex && !EnsureSlotIndex(U.Cp, sc)) return false;
	U.st = stream ? (hipStream_t)stream : R.stream;
	U.sync = !stream;
	if (!TakeRingCounter(R, U.slot)) return false;
	if (U.sync && !EnsureSyncStats(R)) return false;
	StatsHeader(stats, plan, sc);
	return true;
}

// ---- the queries: one call, described by data ----
// What an entry says of its call.  It is made first in the entry: the clock starts and the runtime lock is taken there, so the entry plans under the lock.
// api / apiDevice: the entry's names in the log, `what` its input records'; recordBytes: 32 (rays), 16 (points) or 48 (triangles); out: the outputs in the
// order of the kernel's arguments; slotIndex / exportSlot: the call needs that table of the scene's on the device; ldsBytes: the launch's dynamic LDS.
// inBytes / inAlign: n records of recordBytes read as 16-byte loads, unless the entry says otherwise (a motion call's input is not a record per pixel).
struct QueryDesc {
	const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	const std::lock_guard<std::mutex> lock{ Rt().lock };
	const char *api, *apiDevice, *what;
	const void* in; size_t recordBytes; int32_t n; bool hostMem; void* stream;
	size_t inBytes; uintptr_t inAlign = 15u;
	QueryPlan plan;
	QueryOut out[RL_QUERY_OUTS];
	bool slotIndex = false, exportSlot = false;
	const void* kernel = nullptr; size_t ldsBytes = 0;
	QueryDesc(const char* api_, const char* apiDevice_, const char* what_, const void* in_, size_t recordBytes_, int32_t n_, bool hostMem_, void* stream_)
		: api(api_), apiDevice(apiDevice_), what(what_), in(in_), recordBytes(recordBytes_), n(n_), hostMem(hostMem_), stream(stream_), inBytes((size_t)n_ * recordBytes_) {}
};
// what the entry's launch gets: the scene, the input and the outputs on the device (null: not written), the work counter, a synchronous call's counter block
// (else null), the grid and the stream
struct QueryLaunch {
	const DSceneView& view; const int32_t* slotIndex; const int32_t* exportSlot;
	const float4* in; void* out[RL_QUERY_OUTS];
	unsigned int* counter; unsigned long long* stats;
	dim3 grid; hipStream_t st;
};
// The call.  The refusals -- the plan's, then a device call's pointers' -- come before the scene is touched; an empty call still brings the scene, the plan's
// tree and the tables to the device and fills the stats' header; every buffer is grown before anything is enqueued; the input of a host call is copied on the
// call's stream; a synchronous call's event pair brackets the kernel alone (the counter is cleared in front of it); the outputs of a host call are copied back
// where the caller gave them.
template <typename Launch>
static bool RunQuery(Scene& sc, QueryDesc& D, RaylibAMDStats& stats, Launch launch)
{
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (!D.plan.ok) { Log("%s: BVH depth %u exceeds the traversal stack (64)", D.api, sc.bvh.depth); return false; }
	const CallIn in = { D.in, D.inBytes, D.inAlign };
	if (!D.hostMem && D.n > 0 && !DevicePointersOk(D.apiDevice, D.what, R.device, &in, 1, D.out, RL_QUERY_OUTS)) return false;
	QueryCall U;
	if (!BeginQueryCall(sc, R, D.plan, D.slotIndex, D.stream, U, stats)) return false;
	if (D.exportSlot && !EnsureExportSlot(U.Cp, sc)) return false;
	if (D.n == 0) return true;
	const hipStream_t st = U.st;
	const size_t inBytes = D.inBytes;
	if (!StageOutputs(R, D.out, RL_QUERY_OUTS, D.hostMem)) return false;
	if (D.hostMem && inBytes) {
		if (!R.qRays.Grow(inBytes)) return false;
		HIP_OK(hipMemcpyAsync(R.qRays.ptr, D.in, inBytes, hipMemcpyHostToDevice, st));
	}
	const uint32_t blocks = (uint32_t)FillingGrid(R, D.kernel, (uint64_t)D.n, D.ldsBytes, D.api);
	if (!blocks) return false;
	const bool launched = LaunchOnRing(R, U.slot, st, [&](unsigned int* counter) -> bool {
		if (U.sync && !BeginSync(R, st)) return false;
		QueryLaunch L{ U.Cp->view, U.Cp->slotIndex.ptr, U.Cp->exportSlot.ptr, D.hostMem ? R.qRays.ptr : (const float4*)D.in, {}, counter, U.sync ? R.qStats.ptr : nullptr, dim3(blocks), st };
		for (int k = 0; k < RL_QUERY_OUTS; ++k) L.out[k] = D.out[k].dev;
		launch(L);
		return true;
	});
	if (!launched || !U.sync) return launched;
	std::vector<CopyBack> back;
	for (const QueryOut& o : D.out) back.emplace_back(o, D.hostMem);
	return FinishSync(R, st, back, D.t0, stats);
}

bool DeviceTraceRays(Scene& sc, int32_t kind, const void* rays, int32_t n, float rayTime, void* out, int32_t* outPrim, bool hostMem, void* stream,
                     RaylibAMDStats& stats)
{
	QueryDesc D("RaylibAMD_TraceRays", "RaylibAMD_TraceRaysDevice", "rays", rays, sizeof(RaylibAMDRay), n, hostMem, stream);
	D.plan = PlanQuery(sc, kind, ReadRenderKnobs());
	const bool closest = kind == RAYLIB_AMD_QUERY_CLOSEST, surface = kind == RAYLIB_AMD_QUERY_SURFACE;
	const QueryKernel kernel = surface ? QueryKernelOfKind<RL_QK_SURFACE>(D.plan) : closest ? QueryKernelOfKind<RL_QK_CLOSEST>(D.plan) : QueryKernelOfKind<RL_QK_ANY>(D.plan);
	D.kernel = (const void*)kernel;
	D.out[0] = { out, (size_t)n * (surface ? sizeof(DHitOut) : closest ? sizeof(DQueryHit) : sizeof(uint32_t)), closest ? 15u : 3u, &RankCtx::qOut };
	D.out[1] = { outPrim, surface && outPrim ? (size_t)n * sizeof(int32_t) : 0, 3u, &RankCtx::qPrim };   // (written by SURFACE alone)
	D.slotIndex = closest || (surface && outPrim);
	return RunQuery(sc, D, stats, [&](const QueryLaunch& L) {
		hipLaunchKernelGGL(kernel, L.grid, dim3(RL_BLOCK), 0, L.st, L.view, L.in, (uint32_t)n, rayTime, L.out[0], (int32_t*)L.out[1], L.slotIndex, L.counter, L.stats);
	});
}

// A G-buffer call (RaylibAMD_RenderGBuffer, statements G1 to G6): a query without input records -- the kernel generates the camera's rays -- and with up to
// seven outputs, the planes asked for, in the order of RaylibAMDGBufferPlanes.  The plan is the SURFACE query's (PlanGBuffer); the call's size, for the grid
// and the refusals, is the frame's pixels.  The kernel counts no camera samples: a synchronous call reports the frame's pixels as both.
typedef void (*GBufferKernel)(const DSceneView, const DGBuffer, const int32_t*, unsigned int*, unsigned long long*);
static GBufferKernel GBufferKernelOf(const QueryPlan& p)
{
	if (p.tree == TREE_WIDE8) return (GBufferKernel)k_gbuffer<8, 2 * RL_POOL8_MAXLEVELS, false>;
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (GBufferKernel)k_gbuffer<4, 32, false> : (GBufferKernel)k_gbuffer<4, 64, false>;
	if (p.stack <= 32) return p.prims ? (GBufferKernel)k_gbuffer<2, 32, true> : (GBufferKernel)k_gbuffer<2, 32, false>;
	return p.prims ? (GBufferKernel)k_gbuffer<2, 64, true> : (GBufferKernel)k_gbuffer<2, 64, false>;
}
static_assert(sizeof(RaylibAMDGBufferPlanes) == 7 * sizeof(void*) && RL_QUERY_OUTS >= 7, "a G-buffer's planes are the call's outputs");
// a frame of W x H pixels in 8 x 8 cells, a wave's worth each: the shape members of DGBuffer and DTemporal
template <typename Frame>
static void SetFrameShape(Frame& F, uint32_t W, uint32_t H)
{
	F.width = W; F.height = H; F.cellsX = (W + 7u) / 8u; F.numCells = F.cellsX * ((H + 7u) / 8u);
}
// a G-buffer or motion call's record without its planes and their mask
static DGBuffer MakeGBuffer(const RendererSettings& settings, const DCamera& camera, uint64_t seed)
{
	DGBuffer G; memset(&G, 0, sizeof(G));
	G.camera = camera; G.seed = seed; G.rayTMin = settings.rayTMin;
	SetFrameShape(G, settings.viewportWidth, settings.viewportHeight);
	return G;
}
bool DeviceRenderGBuffer(Scene& sc, const RendererSettings& settings, const DCamera& camera, uint64_t seed, const RaylibAMDGBufferPlanes& planes, bool hostMem, void* stream,
                         RaylibAMDStats& stats)
{
	const size_t pixels = (size_t)settings.viewportWidth * settings.viewportHeight;   // (1 .. 2^31 - 1: the ABI checked)
	QueryDesc D("RaylibAMD_RenderGBuffer", "RaylibAMD_RenderGBufferDevice", nullptr, nullptr, 0, (int32_t)pixels, hostMem, stream);
	D.plan = PlanGBuffer(sc, ReadRenderKnobs());
	const GBufferKernel kernel = GBufferKernelOf(D.plan);
	D.kernel = (const void*)kernel;
	void* const user[7] = { planes.hit, planes.surface, planes.albedo, planes.surfaceNormal, planes.microNormal, planes.texcoord, planes.emission };
	DevBuf<void> RankCtx::* const stage[7] = { &RankCtx::qOut, &RankCtx::qPrim, &RankCtx::qContact, &RankCtx::qPlane3, &RankCtx::qPlane4, &RankCtx::qPlane5, &RankCtx::qPlane6 };
	DGBuffer G = MakeGBuffer(settings, camera, seed);
	for (int k = 0; k < 7; ++k) {
		const bool surface = k == 1;
		D.out[k] = { user[k], user[k] ? pixels * (surface ? sizeof(DHitOut) : sizeof(float4)) : 0, surface ? 3u : 15u, stage[k] };
		if (user[k]) G.mask |= 1u << k;
	}
	D.slotIndex = planes.hit != nullptr;
	const bool ok = RunQuery(sc, D, stats, [&](const QueryLaunch& L) {
		G.hit = (float4*)L.out[0]; G.surface = (DHitOut*)L.out[1];
		G.albedo = (float4*)L.out[2]; G.surfaceNormal = (float4*)L.out[3]; G.microNormal = (float4*)L.out[4]; G.texcoord = (float4*)L.out[5]; G.emission = (float4*)L.out[6];
		hipLaunchKernelGGL(kernel, L.grid, dim3(RL_BLOCK), 0, L.st, L.view, G, L.slotIndex, L.counter, L.stats);
	});
	if (ok && !stream) { stats.cameraSamples = pixels; stats.pixels = pixels; }
	return ok;
}
static_assert(RL_GB_HIT == 1u && RL_GB_SURFACE == 2u && RL_GB_ALBEDO == 4u && RL_GB_SURFACE_NORMAL == 8u && RL_GB_MICRO_NORMAL == 16u && RL_GB_TEXCOORD == 32u && RL_GB_EMISSION == 64u,
              "the plane mask's bits are in the order of RaylibAMDGBufferPlanes");

// A motion call (RaylibAMD_RenderMotion, statements T1 to T6): a G-buffer call with two outputs, the hit plane and the motion plane, and with an input -- the
// previous positions of the moved range, count * 9 floats read as 4-byte words, none when count is 0.  The plan is the G-buffer's; the slot table is always
// needed (the range is in the scene's triangle order).
typedef void (*MotionKernel)(const DSceneView, const DGBuffer, const DMotion, const int32_t*, unsigned int*, unsigned long long*);
static MotionKernel MotionKernelOf(const QueryPlan& p)
{
	if (p.tree == TREE_WIDE8) return (MotionKernel)k_motion<8, 2 * RL_POOL8_MAXLEVELS, false>;
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (MotionKernel)k_motion<4, 32, false> : (MotionKernel)k_motion<4, 64, false>;
	if (p.stack <= 32) return p.prims ? (MotionKernel)k_motion<2, 32, true> : (MotionKernel)k_motion<2, 32, false>;
	return p.prims ? (MotionKernel)k_motion<2, 64, true> : (MotionKernel)k_motion<2, 64, false>;
}
static_assert(sizeof(RaylibAMDMotion) == sizeof(float4), "motion records");
bool DeviceRenderMotion(Scene& sc, const RendererSettings& settings, const DCamera& camera, const DCamera& prevCamera, uint64_t seed, int32_t first, int32_t count,
                        const float* prevPositions, const RaylibAMDMotionPlanes& planes, bool hostMem, void* stream, RaylibAMDStats& stats)
{
	const size_t pixels = (size_t)settings.viewportWidth * settings.viewportHeight;   // (1 .. 2^31 - 1: the ABI checked)
	QueryDesc D("RaylibAMD_RenderMotion", "RaylibAMD_RenderMotionDevice", count > 0 ? "previous positions" : nullptr, count > 0 ? prevPositions : nullptr, 0, (int32_t)pixels,
	            hostMem, stream);
	D.inBytes = (size_t)count * 9u * sizeof(float); D.inAlign = 3u;
	D.plan = PlanGBuffer(sc, ReadRenderKnobs());
	const MotionKernel kernel = MotionKernelOf(D.plan);
	D.kernel = (const void*)kernel;
	D.out[0] = { planes.hit, planes.hit ? pixels * sizeof(float4) : 0, 15u, &RankCtx::qOut };
	D.out[1] = { planes.motion, planes.motion ? pixels * sizeof(float4) : 0, 15u, &RankCtx::qPrim };
	D.slotIndex = true;
	DGBuffer G = MakeGBuffer(settings, camera, seed);
	G.mask = planes.hit ? RL_GB_HIT : 0u;
	DMotion M; memset(&M, 0, sizeof(M));
	M.prevCamera = prevCamera; M.first = first; M.count = count;
	const bool ok = RunQuery(sc, D, stats, [&](const QueryLaunch& L) {
		G.hit = (float4*)L.out[0];
		M.motion = (float4*)L.out[1]; M.prevPositions = count > 0 ? (const float*)L.in : nullptr;
		hipLaunchKernelGGL(kernel, L.grid, dim3(RL_BLOCK), 0, L.st, L.view, G, M, L.slotIndex, L.counter, L.stats);
	});
	if (ok && !stream) { stats.cameraSamples = pixels; stats.pixels = pixels; }
	return ok;
}

// ---- the plane calls: one call, described by data ----
// What an entry says of its call: planes in, planes out, on rank 0's device -- no scene, no plan, no work counter.  Made first in the entry, as a QueryDesc:
// the clock starts and the runtime lock is taken there.  api / apiDevice: the entry's names in the log; in: the planes read, in the order the launch gets
// them and a host call stages them; out: the planes written; launches: what a synchronous call reports when it is more than one.
#define RL_PLANE_INS 7
#define RL_PLANE_OUTS 3
struct PlaneCall {
	const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	const std::lock_guard<std::mutex> lock{ Rt().lock };
	const char *api, *apiDevice;
	uint32_t W, H; bool hostMem; void* stream;
	CallIn in[RL_PLANE_INS];
	QueryOut out[RL_PLANE_OUTS];
	uint32_t launches = 1;
	PlaneCall(const char* api_, const char* apiDevice_, uint32_t W_, uint32_t H_, bool hostMem_, void* stream_)
		: api(api_), apiDevice(apiDevice_), W(W_), H(H_), hostMem(hostMem_), stream(stream_) {}
	size_t Pixels() const { return (size_t)W * H; }   // (1 .. 2^31 - 1: the ABI checked)
};
// what the entry's launch gets: the rank, the planes on the device (null: not read, not written) and the stream
struct PlaneLaunch { RankCtx& R; const void* in[RL_PLANE_INS]; void* out[RL_PLANE_OUTS]; hipStream_t st; };
// The call.  A device call's refusals come first; then `prepare(R, behind)` grows the entry's scratch, asks what its grid needs and may name in `behind` an
// event the stream has to wait for -- all of it before anything is enqueued.  A host call's inputs are copied back to back into qRays in the entry's order,
// which therefore lists them by descending alignment (16-byte planes, 8-byte pairs, 4-byte words: every plane's size is a multiple of its own alignment); an
// entry that does not is refused here, on the host.  A synchronous call's event pair brackets the launches alone; `launch(L)` enqueues them and asks
// hipGetLastError behind each (false: it failed, and said so); the outputs of a host call are copied back where the caller gave them.
template <typename Prepare, typename Launch>
static bool RunPlanes(PlaneCall& P, RaylibAMDStats& stats, Prepare prepare, Launch launch)
{
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (!P.hostMem && !DevicePointersOk(P.apiDevice, nullptr, R.device, P.in, RL_PLANE_INS, P.out, RL_PLANE_OUTS)) return false;
	const hipStream_t st = P.stream ? (hipStream_t)P.stream : R.stream;
	const bool sync = !P.stream;
	if (sync && !EnsureSyncStats(R)) return false;
	memset(&stats, 0, sizeof(stats));
	stats.ranks = 1; stats.devices = 1;
	if (!StageOutputs(R, P.out, RL_PLANE_OUTS, P.hostMem)) return false;
	hipEvent_t behind = nullptr;
	if (!prepare(R, behind)) return false;
	PlaneLaunch L{ R, {}, {}, st };
	for (int k = 0; k < RL_PLANE_OUTS; ++k) L.out[k] = P.out[k].dev;
	for (int k = 0; k < RL_PLANE_INS; ++k) L.in[k] = P.in[k].bytes ? P.in[k].user : nullptr;
	if (P.hostMem) {
		size_t total = 0;
		for (const CallIn& i : P.in) {
			if (i.bytes && (total & i.align) != 0) { Log("%s: an input plane would be staged at offset %zu, not %u-byte aligned", P.api, total, (unsigned)i.align + 1u); return false; }
			total += i.bytes;
		}
		if (!R.qRays.Grow(total)) return false;
		size_t at = 0;
		for (int k = 0; k < RL_PLANE_INS; ++k) {
			if (!P.in[k].bytes) continue;
			L.in[k] = (const char*)R.qRays.ptr + at;
			HIP_OK(hipMemcpyAsync((void*)L.in[k], P.in[k].user, P.in[k].bytes, hipMemcpyHostToDevice, st));
			at += P.in[k].bytes;
		}
	}
	if (behind) HIP_OK(hipStreamWaitEvent(st, behind, 0));
	if (sync && !BeginSync(R, st)) return false;
	if (!launch(L)) return false;
	if (!sync) return true;
	std::vector<CopyBack> back;
	for (const QueryOut& o : P.out) back.emplace_back(o, P.hostMem);
	if (!FinishSync(R, st, back, P.t0, stats)) return false;
	stats.pixels = P.Pixels();
	if (P.launches > 1) stats.traceLaunches = P.launches;
	return true;
}

// A temporal accumulation (RaylibAMD_TemporalAccumulate, statements T7 and T8; with C.moments RaylibAMD_TemporalAccumulateMoments, statements S1 and S2:
// k_temporal_moments with the history's moments and outMoments beside the rest).  A host call's outputs go through qOut, qPrim and qContact.
static_assert(sizeof(RaylibAMDHitT) == sizeof(float4), "hit records");
bool DeviceTemporalAccumulate(const TemporalCall& C, bool hostMem, void* stream, RaylibAMDStats& stats)
{
	PlaneCall P(C.moments ? "RaylibAMD_TemporalAccumulateMoments" : "RaylibAMD_TemporalAccumulate",
	            C.moments ? "RaylibAMD_TemporalAccumulateMomentsDevice" : "RaylibAMD_TemporalAccumulateDevice", C.width, C.height, hostMem, stream);
	const size_t plane = P.Pixels() * sizeof(float4), lengths = P.Pixels() * sizeof(float), pairs = P.Pixels() * sizeof(float2);
	const size_t hist = C.hasHistory ? 1 : 0;   // (without a history none of its planes is read)
	P.in[0] = { C.colour, plane }; P.in[1] = { C.hit, plane }; P.in[2] = { C.motion, plane };
	P.in[3] = { C.history.colour, hist * plane }; P.in[4] = { C.history.hit, hist * plane };
	P.in[5] = { C.history.moments, C.moments ? hist * pairs : 0, 7u }; P.in[6] = { C.history.length, hist * lengths, 3u };
	P.out[0] = { C.outColour, plane, 15u, &RankCtx::qOut }; P.out[1] = { C.outLength, lengths, 3u, &RankCtx::qPrim };
	P.out[2] = { C.outMoments, C.moments ? pairs : 0, 7u, &RankCtx::qContact };
	DTemporal T; memset(&T, 0, sizeof(T));
	SetFrameShape(T, C.width, C.height);
	T.depthTolerance = C.params->depthTolerance; T.maxLength = C.params->maxLength;
	uint32_t blocks = 0;
	return RunPlanes(P, stats, [&](RankCtx& R, hipEvent_t&) -> bool {
		// a wave per cell at a time: workgroups enough for the cells, at most the device filled once at the kernel's occupancy
		const int perCU = OccupancyOf(R, C.moments ? (const void*)k_temporal_moments : (const void*)k_temporal);
		if (perCU < 0) return false;
		const uint64_t cellBlocks = ((uint64_t)T.numCells + RL_BLOCK / 64u - 1u) / (RL_BLOCK / 64u);
		blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)R.numCUs * (uint64_t)std::max(1, perCU), cellBlocks));
		return true;
	}, [&](const PlaneLaunch& L) -> bool {
		T.colour = (const float4*)L.in[0]; T.hit = (const float4*)L.in[1]; T.motion = (const float4*)L.in[2];
		T.histColour = (const float4*)L.in[3]; T.histHit = (const float4*)L.in[4]; T.histLength = (const float*)L.in[6];
		T.outColour = (float4*)L.out[0]; T.outLength = (float*)L.out[1];
		if (C.moments) hipLaunchKernelGGL(k_temporal_moments, dim3(blocks), dim3(RL_BLOCK), 0, L.st, T, (const float2*)L.in[5], (float2*)L.out[2]);
		else hipLaunchKernelGGL(k_temporal, dim3(blocks), dim3(RL_BLOCK), 0, L.st, T);
		HIP_OK(hipGetLastError());
		return true;
	});
}

// A variance-guided filter call (RaylibAMD_FilterVariance, statements S3 to S7): 2 + K launches on the call's stream with the library's scratch between them
// -- the guides (32 bytes per pixel) and the two value planes of the iterations' ping-pong (16 each), kept and grown.  Calls on different streams share that
// scratch: every call waits on its own stream for the event behind the last call's last launch (vfEv), as the path calls do with radEv.  A host call's
// outputs go through qOut and qPrim.
static_assert(sizeof(DHitOut) == 11 * sizeof(float), "surface records are 11 words");
bool DeviceFilterVariance(uint32_t W, uint32_t H, const RaylibAMDVarianceFilterParams& params, const RaylibAMDVarianceFilterPlanes& planes, float* outColour, float* outVariance,
                          bool hostMem, void* stream, RaylibAMDStats& stats)
{
	PlaneCall P("RaylibAMD_FilterVariance", "RaylibAMD_FilterVarianceDevice", W, H, hostMem, stream);
	const size_t pixels = P.Pixels();
	P.in[0] = { planes.colour, pixels * sizeof(float4) }; P.in[1] = { planes.hit, pixels * sizeof(float4) };
	P.in[2] = { planes.moments, pixels * sizeof(float2), 7u }; P.in[3] = { planes.surface, pixels * sizeof(DHitOut), 3u }; P.in[4] = { planes.length, pixels * sizeof(float), 3u };
	P.out[0] = { outColour, pixels * sizeof(float4), 15u, &RankCtx::qOut }; P.out[1] = { outVariance, outVariance ? pixels * sizeof(float) : 0, 3u, &RankCtx::qPrim };
	P.launches = 2u + (uint32_t)params.iterations;
	return RunPlanes(P, stats, [&](RankCtx& R, hipEvent_t& behind) -> bool {
		if (!R.vfGuides.Grow(pixels * sizeof(VfGuide)) || !R.vfValues[0].Grow(pixels * sizeof(VfValue)) || !R.vfValues[1].Grow(pixels * sizeof(VfValue))) return false;
		if (!R.vfEv) HIP_OK(hipEventCreateWithFlags(&R.vfEv, hipEventDisableTiming));
		if (R.vfEvUsed) behind = R.vfEv;
		return true;
	}, [&](const PlaneLaunch& L) -> bool {
		RankCtx& R = L.R;
		const hipStream_t st = L.st;
		const VfConst c = MakeVfConst(params.sigmaLuminance, params.sigmaNormal, params.sigmaPlane, params.historyLength);
		const uint32_t n = (uint32_t)pixels;
		const dim3 linear((n + RL_BLOCK - 1u) / RL_BLOCK), tiles(((W + 15u) / 16u) * ((H + 15u) / 16u));   // (at most 2^23 + 1 and 2^27 workgroups)
		hipLaunchKernelGGL(k_vf_pack, linear, dim3(RL_BLOCK), 0, st, (const float4*)L.in[0], (const float4*)L.in[1], (const float*)L.in[3], n, R.vfGuides.ptr, R.vfValues[0].ptr);
		HIP_OK(hipGetLastError());
		hipLaunchKernelGGL(k_vf_variance, tiles, dim3(RL_BLOCK), 0, st, (const VfGuide*)R.vfGuides.ptr, (const float*)L.in[2], (const float*)L.in[4], W, H, c, R.vfValues[0].ptr);
		HIP_OK(hipGetLastError());
		int cur = 0;
		for (int i = 0; i < params.iterations; ++i, cur ^= 1) {
			if (i + 1 < params.iterations)
				hipLaunchKernelGGL(k_vf_iter<false>, tiles, dim3(RL_BLOCK), 0, st, (const VfValue*)R.vfValues[cur].ptr, (const VfGuide*)R.vfGuides.ptr, W, H, (int32_t)(1 << i), c,
				                   R.vfValues[cur ^ 1].ptr, (float4*)nullptr, (float*)nullptr);
			else
				hipLaunchKernelGGL(k_vf_iter<true>, tiles, dim3(RL_BLOCK), 0, st, (const VfValue*)R.vfValues[cur].ptr, (const VfGuide*)R.vfGuides.ptr, W, H, (int32_t)(1 << i), c,
				                   (VfValue*)nullptr, (float4*)L.out[0], (float*)L.out[1]);
			HIP_OK(hipGetLastError());
		}
		HIP_OK(hipEventRecord(R.vfEv, st));
		R.vfEvUsed = true;
		return true;
	});
}

// An ordered multi-hit call: rows of maxHits records and, when asked for, a count per ray (staged through qPrim); the launch carries the lanes' lists as
// dynamic LDS (2 * maxHits * RL_BLOCK words), which its grid's occupancy accounts for.
bool DeviceTraceRaysAll(Scene& sc, const void* rays, int32_t n, int32_t maxHits, void* outHits, uint32_t* outCount, bool hostMem, void* stream, RaylibAMDStats& stats)
{
	QueryDesc D("RaylibAMD_TraceRaysAll", "RaylibAMD_TraceRaysAllDevice", "rays", rays, sizeof(RaylibAMDRay), n, hostMem, stream);
	D.plan = PlanQueryAll(sc, ReadRenderKnobs());
	const QueryAllKernel kernel = outCount ? QueryAllKernelOf<true>(D.plan) : QueryAllKernelOf<false>(D.plan);
	D.kernel = (const void*)kernel;
	D.ldsBytes = 2u * (size_t)maxHits * RL_BLOCK * sizeof(uint32_t);
	D.out[0] = { outHits, (size_t)n * (size_t)maxHits * sizeof(DQueryHit), 15u, &RankCtx::qOut };
	D.out[1] = { outCount, outCount ? (size_t)n * sizeof(uint32_t) : 0, 3u, &RankCtx::qPrim };
	D.slotIndex = true;
	return RunQuery(sc, D, stats, [&](const QueryLaunch& L) {
		hipLaunchKernelGGL(kernel, L.grid, dim3(RL_BLOCK), (uint32_t)D.ldsBytes, L.st, L.view, L.in, (uint32_t)n, (uint32_t)maxHits, (float4*)L.out[0], (uint32_t*)L.out[1], L.slotIndex, L.counter,
		                   L.stats);
	});
}

// A nearest-point call: 16-byte records in, a word (WITHIN) or a record (CLOSEST) per point out.
bool DeviceNearestPoints(Scene& sc, int32_t kind, const void* points, int32_t n, void* out, bool hostMem, void* stream, RaylibAMDStats& stats)
{
	QueryDesc D("RaylibAMD_NearestPoints", "RaylibAMD_NearestPointsDevice", "points", points, sizeof(RaylibAMDNearestQuery), n, hostMem, stream);
	D.plan = PlanNearest(sc, kind, ReadRenderKnobs());
	const bool closest = kind == RAYLIB_AMD_NEAREST_CLOSEST;
	const NearestKernel kernel = closest ? NearestKernelOfKind<RL_NK_CLOSEST>(D.plan) : NearestKernelOfKind<RL_NK_WITHIN>(D.plan);
	D.kernel = (const void*)kernel;
	D.out[0] = { out, (size_t)n * (closest ? sizeof(DNearestHit) : sizeof(uint32_t)), closest ? 15u : 3u, &RankCtx::qOut };
	D.slotIndex = closest;
	return RunQuery(sc, D, stats, [&](const QueryLaunch& L) {
		hipLaunchKernelGGL(kernel, L.grid, dim3(RL_BLOCK), 0, L.st, L.view, L.in, (uint32_t)n, L.out[0], L.slotIndex, L.counter, L.stats);
	});
}

// A swept-sphere call: 32-byte records in, a word (ANY) or a 32-byte record (CLOSEST, two 16-byte stores) per query out.
bool DeviceSweepSpheres(Scene& sc, int32_t kind, const void* queries, int32_t n, void* out, bool hostMem, void* stream, RaylibAMDStats& stats)
{
	QueryDesc D("RaylibAMD_SweepSpheres", "RaylibAMD_SweepSpheresDevice", "queries", queries, sizeof(RaylibAMDSweepQuery), n, hostMem, stream);
	D.plan = PlanSweep(sc, kind, ReadRenderKnobs());
	const bool closest = kind == RAYLIB_AMD_SWEEP_CLOSEST;
	const SweepKernel kernel = closest ? SweepKernelOfKind<RL_SK_CLOSEST>(D.plan) : SweepKernelOfKind<RL_SK_ANY>(D.plan);
	D.kernel = (const void*)kernel;
	D.out[0] = { out, (size_t)n * (closest ? sizeof(DSweepHit) : sizeof(uint32_t)), closest ? 15u : 3u, &RankCtx::qOut };
	D.slotIndex = closest;
	return RunQuery(sc, D, stats, [&](const QueryLaunch& L) {
		hipLaunchKernelGGL(kernel, L.grid, dim3(RL_BLOCK), 0, L.st, L.view, L.in, (uint32_t)n, L.out[0], L.slotIndex, L.counter, L.stats);
	});
}

// A K-nearest call: a nearest-point call's input with the multi-hit call's outputs; the lanes' lists (2 * maxHits * RL_BLOCK words of dynamic LDS) lie beside
// the instance's stack and packed distances (48 KB or 96 KB), which its grid's occupancy accounts for.
bool DeviceNearestPointsAll(Scene& sc, const void* points, int32_t n, int32_t maxHits, void* outHits, uint32_t* outCount, bool hostMem, void* stream, RaylibAMDStats& stats)
{
	QueryDesc D("RaylibAMD_NearestPointsAll", "RaylibAMD_NearestPointsAllDevice", "points", points, sizeof(RaylibAMDNearestQuery), n, hostMem, stream);
	D.plan = PlanNearestAll(sc, ReadRenderKnobs());
	const NearestAllKernel kernel = outCount ? NearestAllKernelOf<true>(D.plan) : NearestAllKernelOf<false>(D.plan);
	D.kernel = (const void*)kernel;
	D.ldsBytes = 2u * (size_t)maxHits * RL_BLOCK * sizeof(uint32_t);
	D.out[0] = { outHits, (size_t)n * (size_t)maxHits * sizeof(DNearestHit), 15u, &RankCtx::qOut };
	D.out[1] = { outCount, outCount ? (size_t)n * sizeof(uint32_t) : 0, 3u, &RankCtx::qPrim };
	D.slotIndex = true;
	return RunQuery(sc, D, stats, [&](const QueryLaunch& L) {
		hipLaunchKernelGGL(kernel, L.grid, dim3(RL_BLOCK), (uint32_t)D.ldsBytes, L.st, L.view, L.in, (uint32_t)n, (uint32_t)maxHits, (float4*)L.out[0], (uint32_t*)L.out[1], L.slotIndex, L.counter,
		                   L.stats);
	});
}

// A triangle-overlap call: 48-byte records in; a word per query (ANY), or rows of maxHits indices and, when asked for, a count per query (LIST), whose launch
// carries the lanes' lists as dynamic LDS (maxHits * RL_BLOCK words).  `contacts` (RaylibAMD_OverlapContacts): kind is LIST, the kernel is the contacts
// instance of the same plan, which reads a listed triangle again through exportSlot, and a third output, n * maxHits records of 32 bytes (two float4 stores
// each), is staged through qContact.
bool DeviceOverlapTriangles(Scene& sc, int32_t kind, uint32_t flags, const void* queries, int32_t n, int32_t maxHits, void* out, uint32_t* outCount, bool hostMem, void* stream,
                            RaylibAMDStats& stats, void* outContact, bool contacts)
{
	QueryDesc D("RaylibAMD_OverlapTriangles", contacts ? "RaylibAMD_OverlapContactsDevice" : "RaylibAMD_OverlapTrianglesDevice", "queries", queries, sizeof(RaylibAMDOverlapQuery), n,
	            hostMem, stream);
	D.plan = PlanOverlap(sc, kind, ReadRenderKnobs());
	const bool list = kind == RAYLIB_AMD_OVERLAP_LIST;
	const OverlapKernel kernel = list ? OverlapKernelOfKind<RL_OK_LIST>(D.plan) : OverlapKernelOfKind<RL_OK_ANY>(D.plan);
	const OverlapContactsKernel contactsKernel = OverlapContactsKernelOf(D.plan);
	D.kernel = contacts ? (const void*)contactsKernel : (const void*)kernel;
	D.ldsBytes = list ? (size_t)maxHits * RL_BLOCK * sizeof(uint32_t) : 0;
	D.out[0] = { out, list ? (size_t)n * (size_t)maxHits * sizeof(int32_t) : (size_t)n * sizeof(uint32_t), 3u, &RankCtx::qOut };
	D.out[1] = { outCount, outCount ? (size_t)n * sizeof(uint32_t) : 0, 3u, &RankCtx::qPrim };
	if (contacts) D.out[2] = { outContact, (size_t)n * (size_t)maxHits * sizeof(RaylibAMDContact), 15u, &RankCtx::qContact };
	D.slotIndex = list; D.exportSlot = contacts;
	return RunQuery(sc, D, stats, [&](const QueryLaunch& L) {
		if (contacts)
			hipLaunchKernelGGL(contactsKernel, L.grid, dim3(RL_BLOCK), (uint32_t)D.ldsBytes, L.st, L.view, L.in, (uint32_t)n, flags, (uint32_t)maxHits, L.out[0], (uint32_t*)L.out[1], L.slotIndex,
			                   L.counter, L.stats, (float4*)L.out[2], L.exportSlot);
		else
			hipLaunchKernelGGL(kernel, L.grid, dim3(RL_BLOCK), (uint32_t)D.ldsBytes, L.st, L.view, L.in, (uint32_t)n, flags, (uint32_t)(list ? maxHits : 0), L.out[0], (uint32_t*)L.out[1], L.slotIndex,
			                   L.counter, L.stats);
	});
}

// An oriented-box call: 64-byte records in; a word per query (ANY), rows of maxHits indices and, when asked for, a count per query (LIST, with the lanes' lists
// as dynamic LDS), or one mask of (triangles + 31) / 32 words for the whole call (MARK), which is cleared on the call's stream in front of the kernel that ORs
// into it.  An empty MARK call still writes the mask -- all zero -- after the refusals of its pointers.
bool DeviceOverlapBoxes(Scene& sc, int32_t kind, const void* queries, int32_t n, int32_t maxHits, void* out, uint32_t* outCount, bool hostMem, void* stream, RaylibAMDStats& stats)
{
	QueryDesc D("RaylibAMD_OverlapBoxes", "RaylibAMD_OverlapBoxesDevice", "queries", queries, sizeof(RaylibAMDBoxQuery), n, hostMem, stream);
	D.plan = PlanOverlapBoxes(sc, kind, ReadRenderKnobs());
	const bool list = kind == RAYLIB_AMD_BOX_LIST, mark = kind == RAYLIB_AMD_BOX_MARK;
	const OverlapBoxKernel kernel = mark ? OverlapBoxKernelOfKind<RL_BK_MARK>(D.plan) : list ? OverlapBoxKernelOfKind<RL_BK_LIST>(D.plan) : OverlapBoxKernelOfKind<RL_BK_ANY>(D.plan);
	D.kernel = (const void*)kernel;
	D.ldsBytes = list ? (size_t)maxHits * RL_BLOCK * sizeof(uint32_t) : 0;
	const size_t maskBytes = (sc.triangles.size() + 31u) / 32u * sizeof(uint32_t);
	D.out[0] = { out, mark ? maskBytes : list ? (size_t)n * (size_t)maxHits * sizeof(int32_t) : (size_t)n * sizeof(uint32_t), 3u, &RankCtx::qOut };
	D.out[1] = { outCount, outCount ? (size_t)n * sizeof(uint32_t) : 0, 3u, &RankCtx::qPrim };
	D.slotIndex = list || mark;
	if (mark && n == 0 && out && maskBytes) {
		// (RunQuery asks an empty call's pointers nothing: this one writes)
		if (!EnsureRuntime()) return false;
		RankCtx& R = Rank0();
		HIP_OK(hipSetDevice(R.device));
		if (!hostMem && !DevicePointersOk(D.apiDevice, nullptr, R.device, nullptr, 0, D.out, 1)) return false;
	}
	if (!RunQuery(sc, D, stats, [&](const QueryLaunch& L) {
		if (mark) (void)hipMemsetAsync(L.out[0], 0, maskBytes, L.st);   // (a failure is the launch's error: LaunchOnRing asks hipGetLastError behind it)
		hipLaunchKernelGGL(kernel, L.grid, dim3(RL_BLOCK), (uint32_t)D.ldsBytes, L.st, L.view, L.in, (uint32_t)n, (uint32_t)(list ? maxHits : 0), L.out[0], (uint32_t*)L.out[1], L.slotIndex,
		                   L.counter, L.stats);
	})) return false;
	if (mark && n == 0 && out && maskBytes) {
		if (hostMem) memset(out, 0, maskBytes);
		else {
			const hipStream_t st = stream ? (hipStream_t)stream : Rank0().stream;
			HIP_OK(hipMemsetAsync(out, 0, maskBytes, st));
			if (!stream) HIP_OK(hipStreamSynchronize(st));
		}
	}
	return true;
}

// A distance-field bake (RaylibAMD_BakeDistanceField) is a nearest-point call without points and a multi-hit call without rays: up to three launches on one
// stream -- k_sdf_rows into the zeroed bit volumes and k_sdf_parity over them (a signed bake), then k_sdf_dist -- each walk on its own plan's tree, each with a
// ring counter of its own (LaunchOnRing).  The volumes are the rank's (sdfBits), ordered between bakes by sdfEv as the radiance scratch is by radEv.  A host
// call's outputs go through qOut and qPrim, as a query's.
bool DeviceBakeDistanceField(Scene& sc, const RaylibAMDDistanceFieldParams& prm, float* outDist, int32_t* outPrim, bool hostMem, void* stream, RaylibAMDStats& stats)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	const DistanceFieldPlan plan = PlanDistanceField(sc, ReadRenderKnobs());
	if (!plan.nearest.ok || !plan.rows.ok) { Log("RaylibAMD_BakeDistanceField: BVH depth %u exceeds the traversal stack (64)", sc.bvh.depth); return false; }
	// the grid, and the rows and bit volumes of the sign axes
	DSdfGrid G; memset(&G, 0, sizeof(G));
	for (int a = 0; a < 3; ++a) { G.origin[a] = prm.origin[a]; G.spacing[a] = prm.spacing[a]; G.dims[a] = (uint32_t)prm.dims[a]; }
	G.maxDist = prm.maxDist;
	G.axes = prm.sign == RAYLIB_AMD_SDF_UNSIGNED ? 0u : prm.sign == RAYLIB_AMD_SDF_SIGN_MAJORITY ? 7u : 1u << (prm.sign - RAYLIB_AMD_SDF_SIGN_X);
	const uint64_t voxels = (uint64_t)G.dims[0] * G.dims[1] * G.dims[2];
	uint64_t rows = 0, words = 0;
	for (int a = 0; a < 3; ++a) {
		const uint64_t rowsA = ((G.axes >> a) & 1u) ? voxels / G.dims[a] : 0u;   // the product of the other two dims
		G.words[a] = (G.dims[a] + 1u + 31u) / 32u;
		G.wordBase[a] = words;
		rows += rowsA; words += rowsA * G.words[a];
		G.rowEnd[a] = (uint32_t)rows;   // (three axes of at most 2^31 - 1 voxels: at most 2^32 - 1 rows; the launches below are cut at 2^31 - 1)
	}
	QueryOut outs[2] = { { outDist, (size_t)voxels * sizeof(float), 3u, &RankCtx::qOut }, { outPrim, outPrim ? (size_t)voxels * sizeof(int32_t) : 0, 3u, &RankCtx::qPrim } };
	if (!hostMem && !DevicePointersOk("RaylibAMD_BakeDistanceFieldDevice", nullptr, R.device, nullptr, 0, outs, 2)) return false;
	QueryCall U;
	if (!BeginQueryCall(sc, R, plan.nearest, true, stream, U, stats)) return false;
	if (G.axes && !EnsureWideTree(U.Cp, sc, plan.rows.tree)) return false;
	const hipStream_t st = U.st;
	if (G.axes && !R.sdfBits.Grow((size_t)words * sizeof(uint32_t))) return false;
	if (!R.sdfEv) HIP_OK(hipEventCreateWithFlags(&R.sdfEv, hipEventDisableTiming));
	if (!StageOutputs(R, outs, 2, hostMem)) return false;
	const SdfDistKernel distKernel = G.axes ? SdfDistKernelOf<true>(plan.nearest) : SdfDistKernelOf<false>(plan.nearest);
	const uint64_t bricks = (uint64_t)((G.dims[0] + 3u) / 4u) * ((G.dims[1] + 3u) / 4u) * ((G.dims[2] + 3u) / 4u);
	const uint32_t distBlocks = (uint32_t)FillingGrid(R, (const void*)distKernel, bricks * 64u);
	if (!distBlocks) return false;
	const DSceneView view = U.Cp->view;
	if (R.sdfEvUsed) HIP_OK(hipStreamWaitEvent(st, R.sdfEv, 0));   // a bake enqueued on a caller's stream may still be using the volumes
	if (U.sync && !BeginSync(R, st)) return false;
	unsigned long long* counters = U.sync ? R.qStats.ptr : nullptr;
	uint32_t slot = U.slot;
	if (G.axes) HIP_OK(hipMemsetAsync(R.sdfBits.ptr, 0, (size_t)words * sizeof(uint32_t), st));
	if (G.axes && !sc.triangles.empty()) {   // (an empty scene has no crossing: the zeroed volumes are its inside bits)
		const SdfRowsKernel rowsKernel = SdfRowsKernelOf(plan.rows);
		// one launch for all the axes' rows, or, past 2^31 - 1 of them (the row counter runs ahead of n by a chunk per wave), one per axis
		const bool cut = rows > 0x7fffffffull;
		for (int a = 0; a < (cut ? 3 : 1); ++a) {
			DSdfGrid L = G;
			uint64_t n = rows;
			if (cut) {
				if (!((G.axes >> a) & 1u)) continue;
				n = voxels / G.dims[a];
				for (int b = 0; b < 3; ++b) L.rowEnd[b] = b < a ? 0u : (uint32_t)n;
			}
			const uint32_t blocks = (uint32_t)FillingGrid(R, (const void*)rowsKernel, n);
			if (!blocks) return false;
			const bool launched = LaunchOnRing(R, slot, st, [&](unsigned int* counter) -> bool {
				hipLaunchKernelGGL(rowsKernel, dim3(blocks), dim3(RL_BLOCK), 0, st, view, L, (uint32_t)n, R.sdfBits.ptr, counter, counters);
				HIP_OK(hipGetLastError());
				hipLaunchKernelGGL(k_sdf_parity, dim3((uint32_t)((n + RL_BLOCK - 1) / RL_BLOCK)), dim3(RL_BLOCK), 0, st, L, (uint32_t)n, R.sdfBits.ptr);
				return true;
			});
			if (!launched || !TakeRingCounter(R, slot)) return false;
		}
	}
	const bool launched = LaunchOnRing(R, slot, st, [&](unsigned int* counter) -> bool {
		hipLaunchKernelGGL(distKernel, dim3(distBlocks), dim3(RL_BLOCK), 0, st, view, G, (float*)outs[0].dev, (int32_t*)outs[1].dev, (const uint32_t*)R.sdfBits.ptr,
		                   (const int32_t*)U.Cp->slotIndex.ptr, counter, counters);
		return true;
	});
	if (!launched) return false;
	HIP_OK(hipEventRecord(R.sdfEv, st));
	R.sdfEvUsed = true;
	if (!U.sync) return true;
	return FinishSync(R, st, { CopyBack(outs[0], hostMem), CopyBack(outs[1], hostMem) }, t0, stats);
}

// ---- what a radiance call and a gather share ----
// The call up to its first launch: the plan, the refusals of a device call's pointers, the scene, its sky and the plan's tree on the device, the stream, the
// scratch's counter and event, a synchronous call's counter block, and the stats' header.  `api` / `apiDevice`: the entry's names in the log, `what` its input records' ("rays", "points").
struct PathCall { QueryPlan plan; DeviceSceneCopy* Cp = nullptr; hipStream_t st = nullptr; bool sync = false; };
static bool BeginPathCall(const char* api, const char* apiDevice, const char* what, Scene& sc, RankCtx& R, const RenderKnobs& knobs, const void* in, const void* out, uintptr_t outAlign,
                          int32_t n, bool hostMem, void* stream, PathCall& U, RaylibAMDStats& stats)
{
	U.plan = PlanRadiance(sc, knobs);
	if (!U.plan.ok) { Log("%s: BVH depth %u exceeds the traversal stack (64)", api, sc.bvh.depth); return false; }
	const QueryOut result = { const_cast<void*>(out), (size_t)(n > 0), outAlign };   // (written whenever the call has input)
	const CallIn records = { in, (size_t)n * sizeof(RaylibAMDRay) };
	if (!hostMem && n > 0 && !DevicePointersOk(apiDevice, what, R.device, &records, 1, &result, 1)) return false;
	if (!UploadScene(sc) || !SyncSky(sc)) return false;
	U.Cp = sc.device->copy[(size_t)R.devSlot];
	if (!EnsureWideTree(U.Cp, sc, U.plan.tree)) return false;
	U.st = stream ? (hipStream_t)stream : R.stream;
	U.sync = !stream;
	if (!R.radCounter.Grow(sizeof(unsigned int))) return false;
	if (!R.radEv) HIP_OK(hipEventCreateWithFlags(&R.radEv, hipEventDisableTiming));
	if (U.sync && !EnsureSyncStats(R)) return false;
	StatsHeader(stats, U.plan, sc);
	return true;
}
static DRadianceParams PathParams(const RaylibAMDRadianceParams& prm, uint64_t seed)
{
	DRadianceParams Q; memset(&Q, 0, sizeof(Q));
	Q.seedMixed = raylib_rng_mix64(seed); Q.maxPathLength = prm.maxPathLength; Q.rayTMin = prm.rayTMin;
	Q.sampleFirst = prm.sampleFirst; Q.sampleCount = prm.sampleCount; Q.skipDraws = prm.skipDraws;
	Q.timeMin = prm.timeMin; Q.timeMax = prm.timeMax;
	return Q;
}
// The grid of a launch of `jobs` jobs: enough workgroups to fill the device once ...
static uint32_t PathGrid(RankCtx& R, const void* kernel, uint64_t jobs, DRadianceParams& Q)
{
	uint64_t blocks64 = FillingGrid(R, kernel, jobs);
	if (!blocks64) return 0;
	// ... but no more than whose path stack (32 bytes per bounce and resident lane) fits RL_RADIANCE_STACK_BUDGET: long paths run on a smaller grid,
	// which changes no result (a job's arithmetic does not depend on the lane that takes it)
	const size_t depthSlots = (size_t)(Q.maxPathLength > 1 ? Q.maxPathLength : 1);
	const uint64_t stackPerBlock = (uint64_t)depthSlots * 8 * sizeof(float) * RL_BLOCK;
	blocks64 = std::min<uint64_t>(blocks64, RL_RADIANCE_STACK_BUDGET / stackPerBlock);   // (>= 1: RaylibAMD_TraceRadiance refuses a longer path)
	const uint32_t blocks = (uint32_t)blocks64;
	Q.stackStride = blocks * RL_BLOCK;
	// the path stack of the grid: one record per bounce and resident lane.  The scratch is one per rank: a launch waits, on its stream, for the launch before it
	// (whatever stream that ran on), and growing the stack frees it with hipFree, which waits for the device
	if (!R.radStack.Grow(depthSlots * 8 * Q.stackStride * sizeof(float))) return 0;
	return blocks;
}

bool DeviceTraceRadiance(Scene& sc, const RaylibAMDRadianceParams& prm, uint64_t seed, const void* rays, int32_t n, float* out, bool hostMem, void* stream,
                         RaylibAMDStats& stats)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	PathCall U;
	if (!BeginPathCall("RaylibAMD_TraceRadiance", "RaylibAMD_TraceRadianceDevice", "rays", sc, R, ReadRenderKnobs(), rays, out, 15u, n, hostMem, stream, U, stats)) return false;
	if (n == 0) return true;
	const hipStream_t st = U.st;
	const RadianceKernel kernel = RadianceKernelFor(U.plan);
	DRadianceParams Q = PathParams(prm, seed);
	const uint32_t blocks = PathGrid(R, (const void*)kernel, (uint64_t)n, Q);
	if (!blocks) return false;
	const float4* dRays = (const float4*)rays; float4* dOut = (float4*)out;
	const size_t outBytes = (size_t)n * sizeof(float4);
	if (hostMem) {
		if (!StageRays(R, rays, n, outBytes, st)) return false;
		dRays = R.qRays.ptr; dOut = (float4*)R.qOut.ptr;
	}
	const DSceneView view = U.Cp->view;
	const SkyRot skyRot = sc.device->skyRot;
	if (R.radEvUsed) HIP_OK(hipStreamWaitEvent(st, R.radEv, 0));
	HIP_OK(hipMemsetAsync(R.radCounter.ptr, 0, sizeof(unsigned int), st));
	if (U.sync && !BeginSync(R, st)) return false;
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RL_BLOCK), 0, st, view, skyRot, Q, dRays, (uint32_t)n, dOut, R.radStack.ptr, R.radCounter.ptr, U.sync ? R.qStats.ptr : nullptr);
	HIP_OK(hipGetLastError());
	HIP_OK(hipEventRecord(R.radEv, st));
	R.radEvUsed = true;
	if (!U.sync) return true;
	return FinishSync(R, st, { { hostMem ? out : nullptr, dOut, outBytes } }, t0, stats);
}

// ---- the gathers: RaylibAMD_Gather and RaylibAMD_GatherAdaptive (include/raylib_amd.h statements A1 to A5; kernels of rl_gather_adaptive.hip), one driver ----
typedef void (*GatherAdaptiveResolveKernel)(const float4*, uint32_t, uint32_t, const uint32_t*, uint32_t, const GatherAdaptiveState, int, uint32_t, float*, uint32_t*);
static uint32_t CompactTiles(uint32_t numLive) { return (uint32_t)(((uint64_t)numLive + RL_GATHER_COMPACT_TILE - 1) / RL_GATHER_COMPACT_TILE); }

bool EnqueueGatherCompact(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const float4* points, uint32_t* outLive, float4* outPoints, uint32_t* tiles,
                          uint32_t* countHost, hipStream_t st)
{
	const uint32_t numTiles = CompactTiles(numLive);   // (numLive >= 1)
	hipLaunchKernelGGL(k_gather_compact_count, dim3(numTiles), dim3(RL_BLOCK), 0, st, live, stopped, numLive, tiles);
	HIP_OK(hipGetLastError());
	hipLaunchKernelGGL(k_gather_compact_scan, dim3(1), dim3(RL_GATHER_COMPACT_SCAN_BLOCK), 0, st, tiles, numTiles, tiles + numTiles);
	HIP_OK(hipGetLastError());
	hipLaunchKernelGGL(k_gather_compact_move, dim3(numTiles), dim3(RL_BLOCK), 0, st, live, stopped, numLive, (const uint32_t*)tiles, points, outLive, outPoints);
	HIP_OK(hipGetLastError());
	HIP_OK(hipMemcpyAsync(countHost, tiles + numTiles, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	return true;
}

bool DeviceGather(Scene& sc, int32_t kind, const RaylibAMDRadianceParams& prm, uint64_t seed, const void* points, int32_t n, float* out, bool hostMem, void* stream,
                  RaylibAMDStats& stats, const RaylibAMDGatherAdaptiveParams* A, uint32_t* outSamples)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	return GatherLocked(sc, R, kind, prm, seed, points, n, out, hostMem, stream, t0, stats, A, outSamples);
}
// ... the call behind its locked entry: the runtime lock is held and R's device is current.  A lightmap bake (rl_rt_lightmap.hip) enters here with its points
// on the device.
// The plain call (A null): n points x prm.sampleCount samples as the launches of rl_plan.cc PlanGatherCut -- sample ranges of all the points while one sample of
// each fits the sample buffer, point ranges too when not -- each k_gather launch followed by its resolve.  The sums of a point range carry from launch to launch
// in gAcc, so the sum's order does not depend on how the call was cut.  The loop runs over the launch index, 64-bit, and ends at the cut's count.
// The adaptive call (A given) runs in passes.  Pass p traces the samples [(p - 1) * passSamples, n_p) of the live points: the launches of PlanGatherCut over
// (numLive, the pass's samples), each followed by the adaptive resolve, which decides behind the pass's last sample range; then, unless the pass was the last,
// the compaction into the other list and point array, and the wait for the live count.  The first pass reads the caller's points with no list (the identity).
// Everything is allocated before anything is enqueued; the sample buffer, the grid and the path stack are sized for the largest launch of the call.
bool GatherLocked(Scene& sc, RankCtx& R, int32_t kind, const RaylibAMDRadianceParams& prm, uint64_t seed, const void* points, int32_t n, float* out, bool hostMem, void* stream,
                  std::chrono::steady_clock::time_point t0, RaylibAMDStats& stats, const RaylibAMDGatherAdaptiveParams* A, uint32_t* outSamples)
{
	const RenderKnobs knobs = ReadRenderKnobs();
	const bool sphere = kind == RAYLIB_AMD_GATHER_SH9;
	const uint32_t outFloats = sphere ? 27u : 4u, sums = sphere ? 27u : 3u;
	const char* api = A ? "RaylibAMD_GatherAdaptive" : "RaylibAMD_Gather";
	const char* apiDevice = A ? "RaylibAMD_GatherAdaptiveDevice" : "RaylibAMD_GatherDevice";
	PathCall U;
	if (!BeginPathCall(api, apiDevice, "points", sc, R, knobs, points, out, sphere ? 3u : 15u, n, hostMem, stream, U, stats)) return false;
	if (!hostMem && n > 0 && outSamples && (!OnDevice(outSamples, R.device) || ((uintptr_t)outSamples & 3u) != 0)) {
		Log("%s: outSamples is not 4-byte aligned memory of device %d", apiDevice, R.device);
		return false;
	}
	if (n == 0) return true;
	const hipStream_t st = U.st;
	const GatherKernel kernel = sphere ? GatherKernelOfKind<RL_GEN_SPHERE>(U.plan) : GatherKernelOfKind<RL_GEN_HEMISPHERE>(U.plan);
	const GatherResolveKernel resolve = sphere ? (GatherResolveKernel)k_gather_resolve<RL_GEN_SPHERE> : (GatherResolveKernel)k_gather_resolve<RL_GEN_HEMISPHERE>;
	const GatherAdaptiveResolveKernel resolveAdaptive = sphere ? (GatherAdaptiveResolveKernel)k_gather_adaptive_resolve<RL_GEN_SPHERE>
	                                                           : (GatherAdaptiveResolveKernel)k_gather_adaptive_resolve<RL_GEN_HEMISPHERE>;
	const uint32_t N = (uint32_t)n, cap = prm.sampleCount;
	const uint32_t perPass = A ? std::min(A->passSamples, cap) : cap;
	const uint32_t passes = (uint32_t)(((uint64_t)cap + perPass - 1) / perPass);   // (<= 4096: the ABI refused more)
	// the plain call's cut (rl_plan.cc PlanGatherCut): the first launch is the largest, so its grid -- and the path stack of that grid -- serves every launch of the
	// call; a smaller launch on it leaves waves that find the counter drained and end.  No launch of an adaptive call holds more slots than the first pass's points x
	// samples, nor more than the slots per launch (what a cut of very many points gives each launch)
	const GatherCut cut = PlanGatherCut(N, cap, sphere, knobs);
	const uint64_t maxSlots = A ? std::min<uint64_t>(PlanGatherCut(0xffffffffu, 1u, sphere, knobs).pointsPer, (uint64_t)N * perPass) : (uint64_t)cut.pointsPer * cut.samplesPer;
	const uint64_t slotBytes = (sphere ? 2u : 1u) * sizeof(float4);
	if (!R.gSamples.Grow((size_t)(maxSlots * slotBytes))) return false;   // (as the path stack: growing waits for the device)
	if (!A && cut.sampleRanges > 1 && !R.gAcc.Grow((size_t)cut.pointsPer * sums * sizeof(float))) return false;
	if (A) {
		if (!R.gaState.Grow((size_t)N * (sums + 2u) * sizeof(float)) || !R.gaStopped.Grow(N) || !R.gaHost.Grow(sizeof(uint32_t))) return false;
		if (passes > 1) {
			for (int k = 0; k < 2; ++k) if (!R.gaLive[k].Grow((size_t)N * sizeof(uint32_t)) || !R.gaPoints[k].Grow((size_t)N * 2 * sizeof(float4))) return false;
			if (!R.gaTiles.Grow(((size_t)CompactTiles(N) + 1) * sizeof(uint32_t))) return false;
		}
		if (hostMem && outSamples && !R.gaCounts.Grow((size_t)N * sizeof(uint32_t))) return false;
	}
	DRadianceParams Q = PathParams(prm, seed);
	const uint32_t blocks = PathGrid(R, (const void*)kernel, maxSlots, Q);
	if (!blocks) return false;
	const float4* dPoints = (const float4*)points; float* dOut = out; uint32_t* dCounts = outSamples;
	const size_t outBytes = (size_t)n * outFloats * sizeof(float);
	if (hostMem) {
		if (!StageRays(R, points, n, outBytes, st)) return false;
		dPoints = R.qRays.ptr; dOut = (float*)R.qOut.ptr; if (outSamples) dCounts = R.gaCounts.ptr;
	}
	GatherAdaptiveState S = {};
	if (A) {
		S.sum = R.gaState.ptr; S.s1 = R.gaState.ptr + (size_t)N * sums; S.s2 = S.s1 + N; S.stopped = R.gaStopped.ptr;
		S.numPoints = N; S.cap = cap; S.threshold = A->threshold; S.minSamples = A->minSamples;
	}
	const DSceneView view = U.Cp->view;
	const SkyRot skyRot = sc.device->skyRot;
	if (R.radEvUsed) HIP_OK(hipStreamWaitEvent(st, R.radEv, 0));
	if (U.sync && !BeginSync(R, st)) return false;
	// a synchronous call times its trace launches apart from the rest (stats.traceKernelMs), with an event pair per launch -- up to RL_GATHER_TIMED launches: a
	// plain call of more does not begin, an adaptive call, which knows its launches only as the passes go, stops when it gets there
	bool timed = U.sync && (A || cut.launches <= RL_GATHER_TIMED);
	uint64_t launches = 0;
	// one launch, L of the cut of `pts` (the pass's points, listed by `live`; its samples begin at `done` and end the point's first `now`), and its resolve
	auto enqueue = [&](const float4* pts, const uint32_t* live, const GatherLaunch& L, uint32_t done, uint32_t now) -> bool {
		const uint32_t jobs = L.numPoints * L.numSamples;   // (<= maxSlots <= RL_GATHER_MAX_SLOTS: a launch's jobs fit 32 bits with room for the counter's overshoot)
		DGatherJobs J; J.pointFirst = L.pointFirst; J.numPoints = L.numPoints; J.sampleBase = done + L.sampleBase;
		if (launches >= RL_GATHER_TIMED) timed = false;
		if (timed) while (R.gEv.size() < 2 * (launches + 1)) { hipEvent_t e = nullptr; HIP_OK(hipEventCreate(&e)); R.gEv.push_back(e); }
		HIP_OK(hipMemsetAsync(R.radCounter.ptr, 0, sizeof(unsigned int), st));
		if (timed) HIP_OK(hipEventRecord(R.gEv[2 * launches], st));
		hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RL_BLOCK), 0, st, view, skyRot, Q, pts, jobs, J, R.gSamples.ptr, R.radStack.ptr, R.radCounter.ptr,
		                   U.sync ? R.qStats.ptr : nullptr);
		HIP_OK(hipGetLastError());
		if (timed) HIP_OK(hipEventRecord(R.gEv[2 * launches + 1], st));
		const dim3 grid((L.numPoints + RL_BLOCK - 1) / RL_BLOCK);
		if (A) {
			hipLaunchKernelGGL(resolveAdaptive, grid, dim3(RL_BLOCK), 0, st, (const float4*)R.gSamples.ptr, L.numPoints, L.numSamples, live, L.pointFirst, S, (int)L.last, now, dOut, dCounts);
		} else {
			hipLaunchKernelGGL(resolve, grid, dim3(RL_BLOCK), 0, st, (const float4*)R.gSamples.ptr, L.numPoints, L.numSamples, R.gAcc.ptr, dOut + (size_t)L.pointFirst * outFloats,
			                   (int)L.first, (int)L.last, cap);
		}
		HIP_OK(hipGetLastError());
		++launches;
		return true;
	};
	auto enqueueAll = [&]() -> bool {
		if (!A) {
			for (uint64_t k = 0; k < cut.launches; ++k) if (!enqueue(dPoints, nullptr, GatherLaunchAt(cut, N, cap, k), 0u, cap)) return false;
			return true;
		}
		HIP_OK(hipMemsetAsync(R.gaState.ptr, 0, (size_t)N * (sums + 2u) * sizeof(float), st));   // +0 in every sum
		HIP_OK(hipMemsetAsync(R.gaStopped.ptr, 0, N, st));
		const uint32_t* live = nullptr;   // the pass's list (null: the identity) and its points
		const float4* passPoints = dPoints;
		uint32_t numLive = N, done = 0;
		for (uint32_t p = 1; numLive; ++p) {
			const uint32_t now = (uint32_t)std::min<uint64_t>(cap, (uint64_t)p * perPass), take = now - done;
			const GatherCut pc = PlanGatherCut(numLive, take, sphere, knobs);
			for (uint64_t k = 0; k < pc.launches; ++k) if (!enqueue(passPoints, live, GatherLaunchAt(pc, numLive, take, k), done, now)) return false;
			done = now;
			if (p == passes) {
				// every live point stopped at the cap; the call returns when the pass is complete
				if (!U.sync) HIP_OK(hipStreamSynchronize(st));
				break;
			}
			const int to = (int)(p & 1u);
			if (!EnqueueGatherCompact(live, numLive, R.gaStopped.ptr, passPoints, R.gaLive[to].ptr, R.gaPoints[to].ptr, R.gaTiles.ptr, R.gaHost.ptr, st)) return false;
			HIP_OK(hipStreamSynchronize(st));
			const uint32_t next = R.gaHost.ptr[0];
			if (next > numLive) { Log("RaylibAMD_GatherAdaptive: the live set grew from %u to %u points", numLive, next); return false; }
			numLive = next; live = R.gaLive[to].ptr; passPoints = R.gaPoints[to].ptr;
		}
		return true;
	};
	const bool ok = enqueueAll();
	// the event behind whatever was enqueued, a failed call's launches included: the next call on any stream must wait for them before it touches the scratch
	const hipError_t evErr = hipEventRecord(R.radEv, st);
	if (evErr == hipSuccess) R.radEvUsed = true;
	else { Log("HIP error %s recording the gather's event", hipGetErrorName(evErr)); (void)hipStreamSynchronize(st); }   // (no event: the scratch is free again only once the stream is idle)
	if (!ok || evErr != hipSuccess) return false;
	if (!U.sync) return true;
	if (!FinishSync(R, st, { { hostMem ? out : nullptr, dOut, outBytes }, { hostMem ? outSamples : nullptr, dCounts, (size_t)n * sizeof(uint32_t) } }, t0, stats)) return false;
	stats.traceLaunches = (uint32_t)std::min<uint64_t>(launches, 0xffffffffull);
	if (timed) {
		double traceMs = 0.0;
		for (uint64_t k = 0; k < launches; ++k) { float ms = 0.0f; HIP_OK(hipEventElapsedTime(&ms, R.gEv[2 * k], R.gEv[2 * k + 1])); traceMs += ms; }
		stats.traceKernelMs = traceMs;
	}
	return true;
}

} // namespace rl
