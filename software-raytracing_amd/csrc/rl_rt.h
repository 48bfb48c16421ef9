// Host runtime of the MI355X raylib, internal header of its units (rl_rt_*.hip): devices, streams, per-rank work buffers, scene copies, and what a frame
// is while it is queued.  The units are compiled in HIP mode because they launch kernels (rl_kernels.h); none of them holds one.
//   rl_rt_core.hip    the device probe, the RCCL binding, occupancy, DeviceAvailable / DeviceNumRanks / DeviceDrain
//   rl_rt_scene.hip   a flattened scene (rl_scene.cc FlattenScene) to every device, its sky and wide trees; images: read-back, RGB dump, post-processing
//   rl_rt_frame.hip   kernel selection and the one enqueue path of every render (EnqueueFrame), a rank's one-view render, a batch of views
//   rl_rt_render.hip  whole frames over N ranks (gather, scatter, two frames in flight), DeviceRender, progressive sessions
//   rl_rt_rays.hip    caller rays, points and triangles, and the camera's pixels: the queries (DeviceRenderGBuffer, DeviceRenderMotion, DeviceTraceRays, DeviceTraceRaysAll, DeviceNearestPoints, DeviceNearestPointsAll, DeviceSweepSpheres, DeviceOverlapTriangles
//                     and its contacts, DeviceOverlapBoxes: one driver, RunQuery), DeviceBakeDistanceField on the same pieces, DeviceTraceRadiance, DeviceGather (plain and adaptive: one driver, GatherLocked),
//                     the plane calls (DeviceTemporalAccumulate, DeviceFilterVariance: planes in, planes out, no scene; one driver, RunPlanes)
//   rl_rt_lightmap.hip  lightmaps: DeviceLightmapPoints, DeviceBakeLightmap (the raster stages, then DeviceGather's body or the caller's atlas, the filter, the atlas stages)
//   rl_rt_move.hip    RaylibAMD_SceneMoveTriangles: the moved records and the refit of every tree on the device, the host copies' read-back, RaylibAMD_SceneCheckTrees
//   rl_rt_hooks.hip   test hooks
//
// Ranks.  RAYLIB_NUM_GPUS = N (default 1) makes the library drive N devices from this one process: the frame's 8x8
// cells are dealt round-robin to N logical ranks (rank r renders cells r, r + N, ...), every rank has its own
// device, stream, work buffers and scene copy and a host thread that enqueues its work, and the ranks' cell buffers are
// gathered on rank 0's device -- RCCL grouped send / recv over xGMI (librccl is loaded at run time, only then), or
// hipMemcpyPeerAsync pushes (RAYLIB_GATHER=peer, and the fallback when RCCL cannot be initialised) -- where one small
// kernel scatters them into the row-major frame.  Streams are keyed by (seed, pixel, sample), so the assembled frame is
// bit-identical to the one-device frame.  Raylib_Render keeps the reference's shape (raylib.cc:231-239): synchronous, no
// new arguments.  RAYLIB_GPU_MAP = "d0,d1,..." names the physical device of every logical rank; naming one device
// several times (e.g. "0,0,0,0") runs the whole N-rank path on one GPU, which is how the GPU test suite covers it.
// RAYLIB_GATHER_SELF=1 (tests) sends rank 0's own cells through the gather mechanism too.
//
// Which kernel instance a render launches, on which tree, and its job layout are decided in rl_plan.cc; the runtime launches what it says.
#pragma once

#include "rl_kernels.h"
#include "rl_plan.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <thread>

namespace rl {

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
	Log("HIP error %s at %s:%d: %s", hipGetErrorName(e_), __FILE__, __LINE__, #expr); return false; } } while (0)
// the same without leaving the function: clears the local `ok` and goes on (code that has work enqueued and must still reach the place that waits for it)
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
	Log("HIP error %s at %s:%d: %s", hipGetErrorName(e_), __FILE__, __LINE__, #expr); ok = false; } } while (0)

// ---- one owner per buffer: device memory (DevBuf) or pinned host memory (PinBuf), freed when the owner goes -- on the device that is current then, which the
// owner's owner selects.  `ptr` is public: kernel argument arrays take its address.  Grow: at least `need` bytes; it frees, then allocates, and does
// neither when need <= bytes (hipFree waits for the whole device: DeviceTraceRadiance relies on it).  Upload: `count` records of `src`, in a buffer grown to them.
template <typename T, bool PINNED = false>
struct DevBuf {
	T* ptr = nullptr;
	size_t bytes = 0;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { Free(); }
	void Free() { if (ptr) (void)(PINNED ? hipHostFree(ptr) : hipFree(ptr)); ptr = nullptr; bytes = 0; }
	bool Grow(size_t need)
	{
		if (need <= bytes && ptr) return true;
		Free();
		if (PINNED) HIP_OK(hipHostMalloc((void**)&ptr, need, hipHostMallocDefault));
		else HIP_OK(hipMalloc((void**)&ptr, need));
		bytes = need;
		return true;
	}
	bool Upload(const T* src, size_t count)
	{
		if (!Grow((count ? count : 1) * sizeof(T))) return false;
		if (count) HIP_OK(hipMemcpy(ptr, src, count * sizeof(T), hipMemcpyHostToDevice));
		return true;
	}
};
template <typename T> using PinBuf = DevBuf<T, true>;

// One physical device's copy of a scene.  Deleted with its device current (rl_rt_scene.hip FreeScene).
struct DeviceSceneCopy {
	int device = 0;
	DevBuf<DNode4Q> nodes4; DevBuf<DNode4> nodes4f, leafList; DevBuf<DNode8> nodes8;
	DevBuf<DNode> nodes; DevBuf<DTriIsect> isect; DevBuf<DTriShade> shade; DevBuf<int32_t> alphaTex;
	DevBuf<DMaterial> materials; DevBuf<DTexture> textures; DevBuf<float> texels;
	DevBuf<DSphere> spheres; DevBuf<DCube> cubes;
	DevBuf<float> lmTris;        // the scene's triangles in RaylibAMD_SceneExportTriangles order (26 floats each), uploaded when a lightmap call first needs them
	DevBuf<int32_t> slotIndex;   // triangle slot -> index in the scene's triangle order (the ray queries' primitive numbers), uploaded when a query first needs it
	DevBuf<int32_t> exportSlot;  // its inverse, index in the scene's triangle order -> slot: uploaded when a contacts query first needs it (made, and remade, where slotIndex is)
	// the sky panorama is read when a render starts, as the reference does (renderer.cc:159-176 dereferences the handle per miss)
	DevBuf<float4> sky;
	const Image* skyImage = nullptr; uint64_t skyVersion = 0;
	DSceneView view;
	// What moves of the scene's triangles need beside the scene (rl_rt_move.hip), made at the first move: the inverse of triOrder, the binary nodes sorted by
	// level (levelStart[d] ... levelStart[d + 1]: level d), the wide records' box ids (rl_host.h BVH::boxOf*), a host call's values, the status block
	// (rl_kernels.h RL_MOVE_*) and the pinned copy of it and of the root node (16 words behind the block) that the last move's event guards.
	struct Move {
		DevBuf<int32_t> slotOf, boxOf4, boxOf8, boxOfLeafList; DevBuf<uint32_t> levelNodes; std::vector<uint32_t> levelStart;
		DevBuf<float> staging; DevBuf<uint32_t> status; PinBuf<uint32_t> statusHost;
		hipEvent_t ev = nullptr;
		hipEvent_t inEv = nullptr, copiedEv = nullptr;   // several devices, a device call: the values are ready on the call's stream / have reached this device
		bool pending = false;        // a move has been enqueued and its status not yet read (SettleMove)
		int32_t fastBaryBase = 1;    // RAYLIB_FAST_BARY as a fresh upload reads it
	};
	Move* move = nullptr;
	bool lmTrisStale = false;    // lmTris predates a move: uploaded again when a lightmap call next needs it
	~DeviceSceneCopy() { if (move) { for (hipEvent_t e : { move->ev, move->inEv, move->copiedEv }) if (e) (void)hipEventDestroy(e); delete move; } }
};
struct DeviceScene {
	std::vector<DeviceSceneCopy*> copy;   // by device slot (Runtime::devices)
	SkyRot skyRot;
	uint64_t serial = 0;                                             // 1, 2, 3, ... per upload in this process: a progressive session notices a scene uploaded anew
};

// A progressive render (include/raylib_amd.h RaylibAMD_BeginProgressive): what it was begun on, and its state on rank 0's device.  Every cell that is
// still sampled ("live") has the same number of samples, `samples`: a pass renders the samples [samples, passEnd) of the live cells through
// EnqueueRender, with the session's lists as the job list and k_progressive_resolve as the resolve.  Deleted with rank 0's device current.
struct ProgressiveSession {
	Scene* scene = nullptr;
	uint64_t sceneSerial = 0;                      // DeviceScene::serial of the upload the session began on
	const Image* sky = nullptr; uint64_t skyVersion = 0;
	float accelT0 = 0.0f, accelT1 = 0.0f;          // the shutter interval the scene's boxes were built for
	RenderRequest req;                             // settings, camera and seed as of Begin
	uint32_t width = 0, height = 0, numCells = 0, cap = 1;
	DevBuf<float4> sum; DevBuf<float> s1, s2; DevBuf<uint32_t> cellSamples; DevBuf<uint8_t> stopped;
	ProgressiveState st;                           // ... as the kernels take them: sums, moments, per-cell samples and stop flags + the rule's parameters
	DevBuf<uint32_t> live;                         // the live cells, ascending
	DevBuf<uint32_t> trace;                        // ... those of them inside the scene's silhouette: the megakernel's job list
	DevBuf<uint8_t> empty;                         // per cell: outside the silhouette (the cull's flags)
	DevBuf<uint32_t> counts; PinBuf<uint32_t> countsHost;   // k_progressive_compact's counts; pinned copy
	uint32_t samples = 0, passes = 0, passEnd = 0;
	uint32_t numLive = 0, numTrace = 0;
	uint64_t emptyLivePixels = 0;                  // valid pixels of the live cells outside the silhouette
	float emptyL[3] = { 0, 0, 0 }; uint32_t culledRays = 1;
	bool seeded = false;                           // the lists hold the cull's result (its first pass)
};

// ---- RCCL, bound at run time (a one-device render never loads it) -------------------------------------------------
struct RcclApi {
	bool tried = false, ok = false;
	void* lib = nullptr;
	int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;
	int (*CommDestroy)(void* comm) = nullptr;
	int (*Send)(const void* buf, size_t count, int dtype, int peer, void* comm, hipStream_t stream) = nullptr;
	int (*Recv)(void* buf, size_t count, int dtype, int peer, void* comm, hipStream_t stream) = nullptr;
	int (*GroupStart)() = nullptr;
	int (*GroupEnd)() = nullptr;
	const char* (*GetErrorString)(int) = nullptr;
	std::vector<void*> comms;   // one per device slot
};
constexpr int kRcclFloat = 7;   // ncclFloat32 (rccl.h)

// ---- a host thread per rank beyond the first: enqueues that rank's work on its device --------------------------------
struct Worker {
	std::mutex m;
	std::condition_variable cv;
	std::function<bool()> job;
	bool pending = false, result = true;
	void Start(int device)
	{
		std::thread([this, device]() {
			(void)hipSetDevice(device);
			for (;;) {
				std::function<bool()> f;
				{ std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return pending; }); f = job; }
				const bool r = f();
				{ std::lock_guard<std::mutex> lk(m); result = r; pending = false; }
				cv.notify_all();
			}
		}).detach();
	}
	void Post(std::function<bool()> f) { { std::lock_guard<std::mutex> lk(m); job = std::move(f); pending = true; } cv.notify_all(); }
	bool Wait() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return !pending; }); return result; }
};

#define RL_QUERY_RING 64   /* work counters of the queries and the distance-field bakes, used in turn (rl_rt_rays.hip LaunchOnRing) */
struct RankCtx {
	int rank = 0, device = 0, devSlot = 0, numCUs = 0;
	hipStream_t stream = nullptr;
	// Two frame slots (a whole-frame render over several ranks keeps frame i in flight while frame i + 1 is enqueued; everything else uses slot 0).
	// Per slot: 0/1 render, 2/3 megakernel, 4 "my cells are on rank 0's device", (rank 0) 5 every rank's cells are here, 6 frame assembled, 7 counters are on the host
	hipEvent_t ev[2][8] = {};
	PinBuf<unsigned long long> cntHost[2];   // pinned: the counter read-back must not block the enqueuing thread
	// reusable work buffers
	DevBuf<SampleRGB> samples;
	DevBuf<float4> accum, image;
	DevBuf<float> pathStack;
	DevBuf<float4> cells;   // N > 1: this rank's cells back to back, when they are not rendered into the gather buffer
	DevBuf<unsigned long long> counters;
	DevBuf<unsigned int> jobCounter;
	DevBuf<float4> litList; DevBuf<uint32_t> litCtl;   // the lazy-reflectance instance's lit list and its chunk counter (rl_device.h DLitList), reset per sample batch
	DevBuf<uint32_t> litMask;   // ... and its lit-sample mask (rl_lit_mask.h), zeroed per sample batch
	// cells outside the scene's silhouette (CullCells), per frame slot: the list of the others and a flag per cell, pinned on the host and on the device;
	// cullKey = what they were computed from (camera, frame, cells, bounds): an unchanged view re-uses them without a copy
	PinBuf<uint32_t> cellListHost[2]; DevBuf<uint32_t> cellList[2]; size_t cellListCells[2] = { 0, 0 };
	std::vector<unsigned char> cullKey[2];
	uint32_t cullActive[2] = { 0, 0 }; uint64_t cullEmptyPixels[2] = { 0, 0 }; float cullL[2][3] = { { 0, 0, 0 }, { 0, 0, 0 } }; uint32_t cullRays[2] = { 1, 1 };
	std::map<const void*, int> occupancy;   // blocks per CU, asked once per kernel
	Worker* worker = nullptr;
	// the queries (rl_rt_rays.hip RunQuery): staging buffers of the host entries, kept and grown; a ring of work counters, one per launch in turn, each with the
	// event recorded behind its last launch (a slot is reused once that launch is done, whatever stream it ran on); the synchronous queries' counters and events
	DevBuf<float4> qRays;
	DevBuf<void> qOut, qPrim;  // a host call's first output; its second (primitives, counts)
	DevBuf<void> qContact;     // a host contacts call's records (RaylibAMD_OverlapContacts), staged as qPrim is
	DevBuf<void> qPlane3, qPlane4, qPlane5, qPlane6;   // a host G-buffer call's fourth to seventh plane (RaylibAMD_RenderGBuffer), staged as qPrim is
	// a variance filter call's scratch (DeviceFilterVariance), kept and grown: the packed guides, the two value planes of the iterations' ping-pong, and the
	// event behind the last call's last launch -- every call waits for it on its own stream
	DevBuf<VfGuide> vfGuides; DevBuf<VfValue> vfValues[2];
	hipEvent_t vfEv = nullptr; bool vfEvUsed = false;
	// a distance-field bake's bit volumes (DeviceBakeDistanceField), kept and grown, and the event behind the last bake's last kernel -- every bake waits for it
	// on its own stream, so that two bakes on two streams never share the volumes at the same time
	DevBuf<uint32_t> sdfBits;
	hipEvent_t sdfEv = nullptr; bool sdfEvUsed = false;
	DevBuf<unsigned int> qRing; hipEvent_t qRingEv[RL_QUERY_RING] = {}; bool qRingUsed[RL_QUERY_RING] = {}; uint32_t qRingNext = 0;
	DevBuf<unsigned long long> qStats; PinBuf<unsigned long long> qStatsHost;
	hipEvent_t qEv[2] = { nullptr, nullptr };
	// path-traced caller rays (DeviceTraceRadiance): the ray counter and the path stack of the grid, kept and grown, and the event behind the last launch --
	// every launch waits for it on its own stream, so that two calls on two streams never share the scratch at the same time
	DevBuf<unsigned int> radCounter;
	DevBuf<float> radStack;
	hipEvent_t radEv = nullptr; bool radEvUsed = false;
	// a gather's launches between those (DeviceGather), behind the same event: the launch's sample buffer, the per-point sums that carry from launch to launch,
	// and the event pairs with which a synchronous call times its trace launches
	DevBuf<float4> gSamples;
	DevBuf<float> gAcc;
	std::vector<hipEvent_t> gEv;
	// an adaptive gather's state between its passes (GatherLocked with adaptive parameters), behind the same event: the sums and the two moments per point of the call, the stop
	// flags, a host call's sample counts, the two live lists and the two arrays of live points' records of the compaction's ping-pong, the tiles' counts with
	// the live count behind them, and the pinned word that count is read back through
	DevBuf<float> gaState;
	DevBuf<uint8_t> gaStopped;
	DevBuf<uint32_t> gaCounts, gaLive[2], gaTiles;
	DevBuf<float4> gaPoints[2];
	PinBuf<uint32_t> gaHost;
	// a lightmap bake's scratch (rl_rt_lightmap.hip), kept and grown, behind the same event: the raster records and the counts of the range's triangles with
	// the scans' tile sums, a host call's uv, the owner map and the ranks (one word per texel each), the points, their texel indices and values, the two
	// atlases and coverage maps of the dilation's ping-pong; the pinned word the counts are read back through and the events around the stages
	// (lmEv[5]: behind the filter).  lmFilt: the values again, the other half of the filter iterations' ping-pong (a filtered bake, RaylibAMD_FilterLightmap)
	DevBuf<DLmTri> lmRec; DevBuf<unsigned long long> lmCounts, lmSums; DevBuf<float> lmUv;
	DevBuf<uint32_t> lmOwner, lmRank, lmTexel; DevBuf<float4> lmPoints; DevBuf<float> lmValues, lmFilt, lmAtlas[2]; DevBuf<uint8_t> lmCov[2];
	PinBuf<unsigned long long> lmHost;
	hipEvent_t lmEv[6] = {};
	DevBuf<uint32_t> lmSamples, lmSampleAtlas;   // an adaptive bake's sample counts: per point, and scattered into the atlas
	hipEvent_t lmInEv = nullptr;   // recorded on a caller's stream when a bake enters: the raster stages, on the library's stream, wait for it before they read the caller's uv
};

// The one runtime of the process (Rt()): never destroyed, so no buffer is freed behind the HIP runtime's back at exit.
struct Runtime {
	bool probed = false, ok = false;
	std::vector<RankCtx*> ranks;
	std::vector<int> devices;          // the distinct physical devices, rank 0's first
	DevBuf<float4> gather[2];                            // on rank 0's device: every rank's cells, rank by rank; one per frame slot
	hipStream_t gatherStream = nullptr;                  // rank 0's device: receives / waits for the ranks' cells and assembles the frame, beside rank 0's own rendering
	bool gatherSelf = false, wantRccl = true, pipeline = true;
	uint64_t frameNo = 0;                                // whole-frame renders over several ranks so far: slot = frameNo & 1
	struct Inflight;                                     // (rl_rt_render.hip)
	Inflight* inflight[2] = { nullptr, nullptr };        // enqueued, not yet waited for (oldest first by frameNo)
	RaylibAMDStats deferredStats = {};                   // of the last frame in flight that was completed (FinishInflight)
	bool deferredUnreported = false;                     // ... and no caller has read them yet (DeviceDrain)
	uint64_t statsSerial = 0;                            // bumped by every call whose numbers the caller reads next: a frame in flight carries the value it was enqueued
	                                                     // under, and its numbers are reported late only while no such call has come since (FinishInflight, DeviceOwnStats)
	RcclApi rccl;
	std::mutex lock;
};
Runtime& Rt();
inline RankCtx& Rank0() { return *Rt().ranks[0]; }

// What EnqueueFrame leaves for FinishRender: everything is queued on the rank's stream, nothing has been waited for.
struct PendingRender {
	bool pathTrace = false, lastBatchPending = false;
	float traceMs = 0.0f;
	uint32_t launches = 0, jobHeads = 0, pathsPerWave = 64, treeWidth = 2, nodeBytes = 64;   // (the last three: TracePlan's)
	uint64_t pixels = 0;
	uint64_t culledSamples = 0; uint32_t culledRaysPerSample = 0, culledSkyTexels = 0;   // camera samples of cells outside the scene's silhouette: reported apart, not traced (CullCells)
	uint32_t culledCells = 0, listedCells = 0;
	bool lazy = false;                         // the lazy-reflectance instance ran: the counter block's RL_CNT_LIT pair is read back too
	bool enqueuedToEnd = false;                // EnqueueFrame reached the ev[slot][7] record (FinishRender waits for it; otherwise for the whole stream)
	float4* out = nullptr; size_t outBytes = 0;
	int slot = 0;                              // frame slot: which of the rank's event sets / pinned counter buffers this render uses
	const unsigned long long* cnt = nullptr;   // -> the rank's cntHost[slot], valid once ev[slot][7] has fired
};

// ---- what crosses the units; the runtime lock is held by the caller of every one of them ----
bool EnsureRuntime();                                  // rl_rt_core.hip
bool EnsureRccl();
int OccupancyOf(RankCtx& R, const void* kernel, const TracePlan* megakernel = nullptr);
bool UploadScene(Scene& sc);                           // rl_rt_scene.hip
bool SyncSky(Scene& sc);
bool EnsureWideTree(DeviceSceneCopy* C, Scene& sc, int32_t tree);
bool SettleMove(Scene& sc);                            // rl_rt_move.hip: a move in flight is complete and its status applied (the scene is on the device)
bool SyncMovedLocked(Scene& sc);                       // DeviceSyncMovedScene behind its entry
bool ReadbackLocked(Image& img);                       // device copy -> img.rgba
bool EnqueueRender(RankCtx& R, Scene& sc, const RenderRequest& req, PendingRender& pend, ProgressiveSession* prog = nullptr);   // rl_rt_frame.hip
bool FinishRender(RankCtx& R, PendingRender& pend, RaylibAMDStats& stats);
bool OnDevice(const void* p, int device);              // rl_rt_rays.hip: p is memory of that device
// DeviceGather behind its entry; R's device is current.  A (null: the plain gather): statements A1 to A5 in passes, and outSamples (may be null) is host memory
// with hostMem, else device memory.
bool GatherLocked(Scene& sc, RankCtx& R, int32_t kind, const RaylibAMDRadianceParams& prm, uint64_t seed, const void* points, int32_t n, float* out, bool hostMem, void* stream,
                  std::chrono::steady_clock::time_point t0, RaylibAMDStats& stats, const RaylibAMDGatherAdaptiveParams* A = nullptr, uint32_t* outSamples = nullptr);
// the compaction behind a pass (rl_gather_adaptive.hip), enqueued on st: the entries of live (null: the identity) whose points have not stopped into outLive, their
// records from slot i of points into outPoints, the count into tiles[numTiles] (tiles: ceil(numLive / RL_GATHER_COMPACT_TILE) + 1 words) and from there into *countHost (pinned)
bool EnqueueGatherCompact(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const float4* points, uint32_t* outLive, float4* outPoints, uint32_t* tiles,
                          uint32_t* countHost, hipStream_t st);
bool DrainLocked();                                    // rl_rt_render.hip: waits for the multi-rank frames in flight (RenderMulti)

// what every call reports beside its counters: the scene's size, (one rank's calls) one rank on one device, and the call's time on the host's clock
inline void SceneStats(RaylibAMDStats& stats, const Scene& sc)
{
	stats.numNodes = (uint32_t)sc.bvh.nodes.size(); stats.numTriangles = (uint32_t)sc.triangles.size(); stats.bvhDepth = sc.bvh.depth;
}
inline void OneRankStats(RaylibAMDStats& stats, const Scene& sc) { stats.ranks = 1; stats.devices = 1; SceneStats(stats, sc); }
inline double MsSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

} // namespace rl
