// Host runtime of the MI355X raylib: devices, streams, per-rank work buffers, scene upload, launches, and the frame
// split over several GPUs behind Raylib_Render.  Included at the end of rl_render.hip (the kernels launched here are
// templates defined or declared there: rl_kernels.h).
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
// Which kernel instance a render launches, on which tree, and its job layout are decided in rl_plan.cc; this file launches what it says.

#include "rl_plan.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <limits>
#include <map>
#include <mutex>
#include <thread>
#include <dlfcn.h>

namespace rl {

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
	Log("HIP error %s at %s:%d: %s", hipGetErrorName(e_), __FILE__, __LINE__, #expr); return false; } } while (0)
// the same without leaving the function: clears the local `ok` and goes on (code that has work enqueued and must still reach the place that waits for it)
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
	Log("HIP error %s at %s:%d: %s", hipGetErrorName(e_), __FILE__, __LINE__, #expr); ok = false; } } while (0)

// One physical device's copy of a scene.
struct DeviceSceneCopy {
	int device = 0;
	DNode4Q* nodes4 = nullptr; DNode4* nodes4f = nullptr; DNode4* leafList = nullptr; DNode8* nodes8 = nullptr;
	DNode* nodes = nullptr; DTriIsect* isect = nullptr; DTriShade* shade = nullptr; int32_t* alphaTex = nullptr;
	DMaterial* materials = nullptr; DTexture* textures = nullptr; float* texels = nullptr;
	DSphere* spheres = nullptr; DCube* cubes = nullptr;
	int32_t* slotIndex = nullptr;   // triangle slot -> index in the scene's triangle order (the ray queries' primitive numbers), uploaded when a query first needs it
	// the sky panorama is read when a render starts, as the reference does (renderer.cc:159-176 dereferences the handle per miss)
	float4* sky = nullptr; size_t skyBytes = 0;
	const Image* skyImage = nullptr; uint64_t skyVersion = 0;
	DSceneView view;
};
struct DeviceScene {
	std::vector<DeviceSceneCopy*> copy;   // by device slot (Runtime::devices)
	SkyRot skyRot;
	uint64_t serial = 0;                                             // 1, 2, 3, ... per upload in this process: a progressive session notices a scene uploaded anew
};

// A progressive render (include/raylib_amd.h RaylibAMD_BeginProgressive): what it was begun on, and its state on rank 0's device.  Every cell that is
// still sampled ("live") has the same number of samples, `samples`: a pass renders the samples [samples, passEnd) of the live cells through
// EnqueueRender, with the session's lists as the job list and k_progressive_resolve as the resolve.
struct ProgressiveSession {
	Scene* scene = nullptr;
	uint64_t sceneSerial = 0;                      // DeviceScene::serial of the upload the session began on
	const Image* sky = nullptr; uint64_t skyVersion = 0;
	float accelT0 = 0.0f, accelT1 = 0.0f;          // the shutter interval the scene's boxes were built for
	RenderRequest req;                             // settings, camera and seed as of Begin
	uint32_t width = 0, height = 0, numCells = 0, cap = 1;
	ProgressiveState st;                           // sums, moments, per-cell samples and stop flags (rl_render.hip) + the rule's parameters
	uint32_t* live = nullptr;                      // the live cells, ascending
	uint32_t* trace = nullptr;                     // ... those of them inside the scene's silhouette: the megakernel's job list
	uint8_t* empty = nullptr;                      // per cell: outside the silhouette (the cull's flags)
	uint32_t* counts = nullptr; uint32_t* countsHost = nullptr;   // k_progressive_compact's counts; pinned copy
	uint32_t samples = 0, passes = 0, passEnd = 0;
	uint32_t numLive = 0, numTrace = 0;
	uint64_t emptyLivePixels = 0;                  // valid pixels of the live cells outside the silhouette
	float emptyL[3] = { 0, 0, 0 }; uint32_t culledRays = 1;
	bool seeded = false;                           // the lists hold the cull's result (its first pass)
};

namespace {

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

#define RL_QUERY_RING 64   /* ray counters of the ray queries, used in turn (DeviceTraceRays) */
struct RankCtx {
	int rank = 0, device = 0, devSlot = 0, numCUs = 0;
	hipStream_t stream = nullptr;
	// Two frame slots (a whole-frame render over several ranks keeps frame i in flight while frame i + 1 is enqueued; everything else uses slot 0).
	// Per slot: 0/1 render, 2/3 megakernel, 4 "my cells are on rank 0's device", (rank 0) 5 every rank's cells are here, 6 frame assembled, 7 counters are on the host
	hipEvent_t ev[2][8] = {};
	unsigned long long* cntHost[2] = { nullptr, nullptr };   // pinned: the counter read-back must not block the enqueuing thread
	// reusable work buffers
	SampleRGB* samples = nullptr; size_t samplesBytes = 0;
	float4* accum = nullptr; size_t accumBytes = 0;
	float4* image = nullptr; size_t imageBytes = 0;
	float* pathStack = nullptr; size_t pathStackBytes = 0;
	float4* cells = nullptr; size_t cellsBytes = 0;   // N > 1: this rank's cells back to back, when they are not rendered into the gather buffer
	unsigned long long* counters = nullptr;
	unsigned int* jobCounter = nullptr;
	// cells outside the scene's silhouette (CullCells), per frame slot: the list of the others and a flag per cell, pinned on the host and on the device;
	// cullKey = what they were computed from (camera, frame, cells, bounds): an unchanged view re-uses them without a copy
	uint32_t* cellListHost[2] = { nullptr, nullptr }; uint32_t* cellList[2] = { nullptr, nullptr }; size_t cellListCells[2] = { 0, 0 };
	std::vector<unsigned char> cullKey[2];
	uint32_t cullActive[2] = { 0, 0 }; uint64_t cullEmptyPixels[2] = { 0, 0 }; float cullL[2][3] = { { 0, 0, 0 }, { 0, 0, 0 } }; uint32_t cullRays[2] = { 1, 1 };
	std::map<const void*, int> occupancy;   // blocks per CU, asked once per kernel
	Worker* worker = nullptr;
	// the ray queries (DeviceTraceRays): staging buffers of the host entry, kept and grown; a ring of ray counters, one per launch in turn, each with the
	// event recorded behind its last launch (a slot is reused once that launch is done, whatever stream it ran on); the synchronous queries' counters and events
	float4* qRays = nullptr; size_t qRaysBytes = 0;
	void* qOut = nullptr; size_t qOutBytes = 0;
	int32_t* qPrim = nullptr; size_t qPrimBytes = 0;
	unsigned int* qRing = nullptr; hipEvent_t qRingEv[RL_QUERY_RING] = {}; bool qRingUsed[RL_QUERY_RING] = {}; uint32_t qRingNext = 0;
	unsigned long long* qStats = nullptr; unsigned long long* qStatsHost = nullptr;
	hipEvent_t qEv[2] = { nullptr, nullptr };
	// path-traced caller rays (DeviceTraceRadiance): the ray counter and the path stack of the grid, kept and grown, and the event behind the last launch --
	// every launch waits for it on its own stream, so that two calls on two streams never share the scratch at the same time
	unsigned int* radCounter = nullptr;
	float* radStack = nullptr; size_t radStackBytes = 0;
	hipEvent_t radEv = nullptr; bool radEvUsed = false;
};

struct Runtime {
	bool probed = false, ok = false;
	std::vector<RankCtx*> ranks;
	std::vector<int> devices;          // the distinct physical devices, rank 0's first
	float4* gather[2] = { nullptr, nullptr }; size_t gatherBytes[2] = { 0, 0 };   // on rank 0's device: every rank's cells, rank by rank; one per frame slot
	hipStream_t gatherStream = nullptr;                  // rank 0's device: receives / waits for the ranks' cells and assembles the frame, beside rank 0's own rendering
	bool gatherSelf = false, wantRccl = true, pipeline = true;
	uint64_t frameNo = 0;                                // whole-frame renders over several ranks so far: slot = frameNo & 1
	struct Inflight;
	Inflight* inflight[2] = { nullptr, nullptr };        // enqueued, not yet waited for (oldest first by frameNo)
	RcclApi rccl;
	std::mutex lock;
};
Runtime g_rt;
inline RankCtx& Rank0() { return *g_rt.ranks[0]; }
bool ReadbackLocked(Image& img);   // device copy -> img.rgba; the runtime lock is held by the caller
bool DrainLocked();                // waits for the multi-rank frames in flight (RenderMulti); the runtime lock is held by the caller

bool EnsureRuntime()
{
	Runtime& R = g_rt;
	if (R.probed) return R.ok;
	R.probed = true;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
		Log("raylib(MI355X): no HIP device visible -- Raylib_Render cannot run (there is no CPU fallback)");
		return false;
	}
	int n = 1;
	if (const char* e = getenv("RAYLIB_NUM_GPUS")) n = atoi(e);
	if (n < 1 || n > 16) { Log("raylib(MI355X): RAYLIB_NUM_GPUS=%d is outside 1..16", n); return false; }
	std::vector<int> map;
	if (const char* m = getenv("RAYLIB_GPU_MAP")) {
		for (const char* p = m; *p; ) { char* end; const long v = strtol(p, &end, 10); if (end == p) break; map.push_back((int)v); p = (*end == ',') ? end + 1 : end; }
		if ((int)map.size() < n) { Log("raylib(MI355X): RAYLIB_GPU_MAP names %d device(s) for RAYLIB_NUM_GPUS=%d", (int)map.size(), n); return false; }
		map.resize((size_t)n);
		for (int d : map) if (d < 0 || d >= count) { Log("raylib(MI355X): RAYLIB_GPU_MAP names device %d, %d visible", d, count); return false; }
	} else {
		int base = 0;
		if (const char* e = getenv("RAYLIB_DEVICE")) base = atoi(e);
		else if (n == 1) { if (const char* l = getenv("LOCAL_RANK")) base = atoi(l); }
		base = ((base % count) + count) % count;
		if (n > count) {
			Log("raylib(MI355X): RAYLIB_NUM_GPUS=%d but %d device(s) visible (RAYLIB_GPU_MAP may name a device more than once, for tests)", n, count);
			return false;
		}
		for (int r = 0; r < n; ++r) map.push_back((base + r) % count);
	}
	for (int d : map) if (std::find(R.devices.begin(), R.devices.end(), d) == R.devices.end()) R.devices.push_back(d);
	if (const char* g = getenv("RAYLIB_GATHER")) R.wantRccl = strcmp(g, "peer") != 0;
	if (const char* g = getenv("RAYLIB_GATHER_SELF")) R.gatherSelf = atoi(g) != 0;
	if (const char* g = getenv("RAYLIB_PIPELINE")) R.pipeline = atoi(g) != 0;
	for (int r = 0; r < n; ++r) {
		RankCtx* C = new RankCtx;
		C->rank = r; C->device = map[(size_t)r];
		C->devSlot = (int)(std::find(R.devices.begin(), R.devices.end(), C->device) - R.devices.begin());
		HIP_OK(hipSetDevice(C->device));
		hipDeviceProp_t prop;
		HIP_OK(hipGetDeviceProperties(&prop, C->device));
		C->numCUs = prop.multiProcessorCount;
		HIP_OK(hipStreamCreateWithFlags(&C->stream, hipStreamNonBlocking));
		for (int q = 0; q < 2; ++q) {
			for (int i = 0; i < 8; ++i) HIP_OK(hipEventCreate(&C->ev[q][i]));
			HIP_OK(hipHostMalloc((void**)&C->cntHost[q], (CNT_COUNT + 24) * sizeof(unsigned long long), hipHostMallocDefault));
		}
		HIP_OK(hipMalloc(&C->counters, (CNT_COUNT + 24 + RL_TIMELINE_SLOTS) * sizeof(unsigned long long)));
		HIP_OK(hipMalloc(&C->jobCounter, RL_MAX_HEADS * RL_HEAD_STRIDE * sizeof(unsigned int)));   // the heads of the job list, one per XCD, 128 B apart
		if (r > 0) { C->worker = new Worker; C->worker->Start(C->device); }
		R.ranks.push_back(C);
		Log("raylib(MI355X): rank %d of %d on device %d %s (%s), %d CUs", r, n, C->device, prop.name, prop.gcnArchName, C->numCUs);
	}
	if (n > 1) {   // once per process: what a scaling number will have run on
		std::string matrix;
		for (size_t a = 0; a < R.devices.size(); ++a) {
			matrix += a ? " | " : "";
			for (size_t b2 = 0; b2 < R.devices.size(); ++b2) {
				int can = a == b2 ? 1 : 0;
				if (a != b2 && hipDeviceCanAccessPeer(&can, R.devices[a], R.devices[b2]) != hipSuccess) can = -1;
				matrix += can < 0 ? "?" : (can ? "1" : "0");
			}
		}
		(void)hipGetLastError();
		Log("raylib(MI355X): %d logical rank(s) on %d distinct device(s) of %d visible; peer access (row: from, column: to) %s; gather %s, pipeline %s",
		    n, (int)R.devices.size(), count, matrix.c_str(), R.wantRccl ? "rccl (peer copies if it cannot be initialised)" : "peer copies", R.pipeline ? "two frames in flight" : "off");
	}
	// peers write their cells straight into rank 0's gather buffer
	for (size_t s = 1; s < R.devices.size(); ++s) {
		int can = 0;
		if (hipDeviceCanAccessPeer(&can, R.devices[s], R.devices[0]) == hipSuccess && can) {
			(void)hipSetDevice(R.devices[s]);
			const hipError_t e = hipDeviceEnablePeerAccess(R.devices[0], 0);
			if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) Log("raylib(MI355X): peer access %d -> %d could not be enabled (%s); copies will be staged", R.devices[s], R.devices[0], hipGetErrorName(e));
			(void)hipGetLastError();
		}
	}
	HIP_OK(hipSetDevice(R.devices[0]));
	if (n > 1 || R.gatherSelf) HIP_OK(hipStreamCreateWithFlags(&R.gatherStream, hipStreamNonBlocking));
	R.ok = true;
	return true;
}

// RCCL communicators over the distinct devices (single process: ncclCommInitAll).  False: use peer copies.
bool EnsureRccl()
{
	Runtime& R = g_rt;
	RcclApi& A = R.rccl;
	if (A.tried) return A.ok;
	A.tried = true;
	// An RCCL the process already holds (a PyTorch process maps its own) is ADOPTED, never doubled: two copies of the library in one process would each keep
	// their own device state.  /proc/self/maps names the file that is mapped; dlopen(that path, RTLD_NOLOAD) returns the handle of exactly that copy, whatever
	// soname it was loaded under.  Only a process without any librccl loads one -- and when a mapped copy cannot be adopted the gather falls back to peer
	// copies and says so, instead of loading a second one beside it.
	std::string mapped;
	if (FILE* f = fopen("/proc/self/maps", "r")) {
		char line[1024];
		while (fgets(line, sizeof(line), f)) {
			const char* path = strchr(line, '/');
			if (!path) continue;
			const char* base = strrchr(path, '/');
			if (base && strncmp(base + 1, "librccl.so", 10) == 0) { mapped.assign(path); while (!mapped.empty() && (mapped.back() == '\n' || mapped.back() == ' ')) mapped.pop_back(); break; }
		}
		fclose(f);
	}
	const char* how = "adopted (already mapped by this process)";
	if (!mapped.empty()) {
		A.lib = dlopen(mapped.c_str(), RTLD_NOW | RTLD_NOLOAD);
		if (!A.lib) A.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
		if (!A.lib) A.lib = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
		if (!A.lib) { Log("raylib(MI355X): %s is mapped by this process but could not be adopted (%s); not loading a second RCCL -- the gather uses peer copies", mapped.c_str(), dlerror()); return false; }
	} else {
		how = "loaded by the library (no RCCL was mapped)";
		A.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
		if (!A.lib) A.lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
		if (!A.lib) { Log("raylib(MI355X): librccl could not be loaded (%s); the gather uses peer copies", dlerror()); return false; }
	}
	Log("raylib(MI355X): RCCL %s: %s", how, mapped.empty() ? "librccl.so.1" : mapped.c_str());
	A.CommInitAll = (int (*)(void**, int, const int*))dlsym(A.lib, "ncclCommInitAll");
	A.CommDestroy = (int (*)(void*))dlsym(A.lib, "ncclCommDestroy");
	A.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(A.lib, "ncclSend");
	A.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(A.lib, "ncclRecv");
	A.GroupStart = (int (*)())dlsym(A.lib, "ncclGroupStart");
	A.GroupEnd = (int (*)())dlsym(A.lib, "ncclGroupEnd");
	A.GetErrorString = (const char* (*)(int))dlsym(A.lib, "ncclGetErrorString");
	if (!A.CommInitAll || !A.CommDestroy || !A.Send || !A.Recv || !A.GroupStart || !A.GroupEnd) { Log("raylib(MI355X): librccl lacks an expected symbol; the gather uses peer copies"); return false; }
	A.comms.assign(R.devices.size(), nullptr);
	const int rc = A.CommInitAll(A.comms.data(), (int)R.devices.size(), R.devices.data());
	if (rc != 0) { Log("raylib(MI355X): ncclCommInitAll failed (%s); the gather uses peer copies", A.GetErrorString ? A.GetErrorString(rc) : "?"); A.comms.clear(); return false; }
	(void)hipSetDevice(R.devices[0]);
	Log("raylib(MI355X): RCCL communicator over %d device(s)", (int)R.devices.size());
	A.ok = true;
	return true;
}

template <typename T>
bool Grow(T*& ptr, size_t& have, size_t need)
{
	if (need <= have && ptr) return true;
	if (ptr) { (void)hipFree(ptr); ptr = nullptr; have = 0; }
	HIP_OK(hipMalloc(&ptr, need));
	have = need;
	return true;
}

template <typename T>
bool Upload(T*& dst, const T* src, size_t count)
{
	size_t bytes = (count ? count : 1) * sizeof(T);
	HIP_OK(hipMalloc(&dst, bytes));
	if (count) HIP_OK(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice));
	return true;
}

// the wide tree a render is about to walk (TracePlan::tree), on this rank's device: UploadScene puts the default plan's there (TracePlan::eagerTree), the other
// follows the first time a render asks for it.  The copy's pointers are set only once the tree is there.
template <typename T>
static bool UploadOnce(T*& have, const T*& inView, const std::vector<T>& src)
{
	if (have || src.empty()) return true;
	T* p = nullptr;
	if (!Upload(p, src.data(), src.size())) { if (p) (void)hipFree(p); return false; }
	have = p; inView = p;
	return true;
}
static bool EnsureWideTree(DeviceSceneCopy* C, const Scene& sc, int32_t tree)
{
	if (tree == TREE_WIDE8) return UploadOnce(C->nodes8, C->view.nodes8, sc.bvh.nodes8);
	if (tree == TREE_GRID4) return UploadOnce(C->nodes4, C->view.nodes4, sc.bvh.nodes4q);
	return true;
}
void FreeCopy(DeviceSceneCopy* C)
{
	if (!C) return;
	(void)hipSetDevice(C->device);
	(void)hipFree(C->nodes); if (C->nodes4) (void)hipFree(C->nodes4); if (C->nodes4f) (void)hipFree(C->nodes4f); if (C->nodes8) (void)hipFree(C->nodes8); if (C->leafList) (void)hipFree(C->leafList); (void)hipFree(C->isect); (void)hipFree(C->shade); if (C->alphaTex) (void)hipFree(C->alphaTex);
	(void)hipFree(C->materials); (void)hipFree(C->textures); (void)hipFree(C->texels); (void)hipFree(C->spheres); (void)hipFree(C->cubes);
	if (C->sky) (void)hipFree(C->sky);
	if (C->slotIndex) (void)hipFree(C->slotIndex);
	delete C;
}
void FreeScene(DeviceScene* D)
{
	if (!D) return;
	for (DeviceSceneCopy* C : D->copy) FreeCopy(C);
	delete D;
	if (g_rt.ok) (void)hipSetDevice(g_rt.devices[0]);
}

// Flatten the host scene into device records (leaf order) and upload a copy to every device in use.
bool UploadScene(Scene& sc)
{
	if (sc.device) return true;
	const size_t n = sc.triangles.size();
	std::vector<DTriIsect> isect(n);
	std::atomic<int> fastBary(1);
	if (const char* e = getenv("RAYLIB_FAST_BARY")) fastBary.store(atoi(e) != 0 ? 1 : 0);   // 0: the divisions, whatever the scene (parity tests compare the two)
	std::vector<DTriShade> shade(n);
	auto flatten = [&](size_t k0, size_t k1) { for (size_t k = k0; k < k1; ++k) {
		const HostTriangle& t = sc.triangles[sc.bvh.triOrder[k]];
		DTriIsect& I = isect[k];
		const f3 nrm = normalize(cross(t.v1 - t.v0, t.v2 - t.v0));   // geom/triangle.h:34-38
		const f3 u = t.v1 - t.v0, v = t.v2 - t.v0;                   // geom/triangle.cc:30-31
		const float uv = dot(u, v), uu = dot(u, u), vv = dot(v, v);  // :34-38
		const float uvuv = uv * uv, uuvv = uu * vv;                  // :39-40
		I.v0[0] = t.v0.x; I.v0[1] = t.v0.y; I.v0[2] = t.v0.z;
		I.n[0] = nrm.x; I.n[1] = nrm.y; I.n[2] = nrm.z;
		I.v1[0] = t.v1.x; I.v1[1] = t.v1.y; I.v1[2] = t.v1.z;
		I.v2[0] = t.v2.x; I.v2[1] = t.v2.y; I.v2[2] = t.v2.z;
		I.uv = uv; I.uu = uu; I.vv = vv;
		{   // the reciprocal of denom = uvuv - uuvv for the short barycentric divisions (rl_dev_walk.h Barycentric, which states the conditions)
			const float denom = uvuv - uuvv, mag = fabsf(denom);
			if (denom == 0.0f || denom != denom) I.rden = std::numeric_limits<float>::quiet_NaN();
			else if (mag >= 0x1p-62f && mag <= 0x1p125f) I.rden = 1.0f / denom;
			else { I.rden = std::numeric_limits<float>::quiet_NaN(); fastBary.store(0, std::memory_order_relaxed); }
		}
		DTriShade& Sh = shade[k];
		Sh.n0[0] = t.n0.x; Sh.n0[1] = t.n0.y; Sh.n0[2] = t.n0.z;
		Sh.n1[0] = t.n1.x; Sh.n1[1] = t.n1.y; Sh.n1[2] = t.n1.z;
		Sh.n2[0] = t.n2.x; Sh.n2[1] = t.n2.y; Sh.n2[2] = t.n2.z;
		Sh.s0 = t.s0; Sh.t0 = t.t0; Sh.s1 = t.s1; Sh.t1 = t.t1; Sh.s2 = t.s2; Sh.t2 = t.t2;
		Sh.material = t.material;
	} };
	{   // per-triangle records are independent: all host threads for large scenes (10 M triangles: 0.6 s on one thread)
		unsigned threads = n >= (1u << 17) ? std::min(32u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
		if (const char* e = getenv("RAYLIB_BUILD_THREADS")) { int v = atoi(e); if (v > 0 && n >= (1u << 17)) threads = (unsigned)std::min(v, 32); }
		std::vector<std::thread> pool;
		const size_t per = (n + threads - 1) / threads;
		for (unsigned t = 1; t < threads; ++t) { const size_t k0 = std::min(n, t * per), k1 = std::min(n, (t + 1) * per); if (k0 < k1) pool.emplace_back(flatten, k0, k1); }
		flatten(0, std::min(n, per));
		for (std::thread& th : pool) th.join();
	}
	std::vector<DMaterial> mats(sc.materials.size());
	for (size_t i = 0; i < mats.size(); ++i) {
		const HostMaterial& h = sc.materials[i];
		DMaterial& m = mats[i]; memset(&m, 0, sizeof(m));
		m.type = h.type;
		memcpy(m.albedo, h.albedo, 12); m.roughness = h.roughness; m.metallic = h.metallic;
		memcpy(m.emissive, h.emissive, 12); m.ior = h.ior; memcpy(m.transmission, h.transmission, 12);
		m.fuzziness = h.fuzziness; memcpy(m.tex, h.tex, 20);
	}
	std::vector<DTexture> texs(sc.textures.size());
	std::vector<float> pool;
	for (size_t i = 0; i < texs.size(); ++i) {
		const Image& im = *sc.textures[i];
		texs[i].offset = (uint32_t)(pool.size() / 4); texs[i].width = (int32_t)im.width; texs[i].height = (int32_t)im.height; texs[i].pad = 0;
		if (im.hostStale) {   // a rendered image used as a texture: fetch it (the runtime lock is held here)
			Image& w = const_cast<Image&>(im);
			if (!ReadbackLocked(w)) Log("UploadScene: texture %zu could not be read back from the device", i);
			w.hostStale = false;
		}
		pool.insert(pool.end(), im.rgba.begin(), im.rgba.end());
	}
	// Albedo maps are read through Texture2D::Sample(bSRGB = true): nearest texel, then pow(texel, 2.2) on all four channels
	// (reference render/texture.cc:44-50, material.cc:383,400) -- four powf per shading event and per alpha-tested candidate.
	// The power of a texel does not depend on the ray: every texture some material uses as albedo gets a converted copy here
	// (host powf = the reference's own function, the one csrc/rl_glibc_math.h restates), and the material points at the copy.
	{
		std::vector<int32_t> converted(texs.size(), -1);
		for (DMaterial& m : mats) {
			if (m.type != MAT_MICROFACET || m.tex[0] < 0 || (size_t)m.tex[0] >= converted.size()) continue;
			const size_t src = (size_t)m.tex[0];
			if (converted[src] < 0) {
				DTexture t = texs[src];
				const size_t count = (size_t)t.width * t.height * 4, from = (size_t)t.offset * 4;
				t.offset = (uint32_t)(pool.size() / 4);
				pool.resize(pool.size() + count);
				float* dst = pool.data() + (size_t)t.offset * 4; const float* in = pool.data() + from;
				unsigned threads = count >= (1u << 20) ? std::min(32u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
				std::vector<std::thread> workers;
				const size_t per = (count + threads - 1) / threads;
				auto run = [dst, in](size_t a, size_t b) { for (size_t i = a; i < b; ++i) dst[i] = powf(in[i], 2.2f); };
				for (unsigned w = 1; w < threads; ++w) { const size_t a = std::min(count, w * per), b = std::min(count, (w + 1) * per); if (a < b) workers.emplace_back(run, a, b); }
				run(0, std::min(count, per));
				for (std::thread& th : workers) th.join();
				converted[src] = (int32_t)texs.size();
				texs.push_back(t);
			}
			m.tex[0] = converted[src];
		}
	}
	// The cut-out test of a candidate (geom/triangle.cc:54 -> MicrofacetMaterial::AlphaTest) needs one texel of the triangle's material's albedo map: as a table per
	// triangle slot the texture is known from the triangle alone, and the test's chain of dependent loads inside the walk is triangle -> texture -> texel instead
	// of triangle -> material -> texture -> texel (round 5).
	std::vector<int32_t> alphaTex;
	{
		bool any = false;
		for (const DMaterial& m : mats) if (m.type == MAT_MICROFACET && m.tex[0] >= 0) any = true;
		if (any) {
			alphaTex.resize(n);
			for (size_t k = 0; k < n; ++k) {
				const int32_t mi = shade[k].material;
				alphaTex[k] = (mi >= 0 && (size_t)mi < mats.size() && mats[(size_t)mi].type == MAT_MICROFACET && mats[(size_t)mi].tex[0] >= 0) ? mats[(size_t)mi].tex[0] : -1;
			}
		}
	}
	std::vector<DSphere> dsph(sc.spheres.size());
	for (size_t i = 0; i < dsph.size(); ++i) {
		memset(&dsph[i], 0, sizeof(DSphere));
		dsph[i].center[0] = sc.spheres[i].center.x; dsph[i].center[1] = sc.spheres[i].center.y; dsph[i].center[2] = sc.spheres[i].center.z;
		dsph[i].radius = sc.spheres[i].radius; dsph[i].material = sc.spheres[i].material;
	}
	std::vector<DCube> dcub(sc.cubes.size());
	for (size_t i = 0; i < dcub.size(); ++i) {
		memset(&dcub[i], 0, sizeof(DCube));
		const HostCube& h = sc.cubes[i];
		dcub[i].minBounds[0] = h.minBounds.x; dcub[i].minBounds[1] = h.minBounds.y; dcub[i].minBounds[2] = h.minBounds.z; dcub[i].timeStartMove = h.timeStartMove;
		dcub[i].maxBounds[0] = h.maxBounds.x; dcub[i].maxBounds[1] = h.maxBounds.y; dcub[i].maxBounds[2] = h.maxBounds.z; dcub[i].material = h.material;
		dcub[i].velocity[0] = h.velocity.x; dcub[i].velocity[1] = h.velocity.y; dcub[i].velocity[2] = h.velocity.z;
	}

	DeviceScene* D = new DeviceScene;
	static uint64_t s_serial = 0;
	D->serial = ++s_serial;   // (under the runtime lock)
	{   // Rotator(yaw = 90).rotate rows, reference geom/transform.cc:47-65 (host libm, as the reference)
		const float pi_f = (float)3.1415926535897932385;
		const float ry = 90.0f * pi_f / 180.0f, rp = 0.0f * pi_f / 180.0f, rr = 0.0f * pi_f / 180.0f;
		const float ch = cosf(ry), sh = sinf(ry), cp = cosf(rp), sp = sinf(rp), cb = cosf(rr), sb = sinf(rr);
		D->skyRot.m0[0] = ch * cb + sh * sp * sb; D->skyRot.m0[1] = sb * cp; D->skyRot.m0[2] = -sh * cb + ch * sp * sb;
		D->skyRot.m1[0] = -ch * sb + sh * sp * cb; D->skyRot.m1[1] = cb * cp; D->skyRot.m1[2] = sb * sh + ch * sp * cb;
		D->skyRot.m2[0] = sh * cp; D->skyRot.m2[1] = -sp; D->skyRot.m2[2] = ch * cp;
	}
	// the float-box wide nodes (and the leaf list) for scenes small enough to stay in the caches (k_trace's class); of the two wide trees the pool schedule can walk, the
	// one the default plan walks goes to the device now, the other follows when a render asks for it (EnsureWideTree: the switches are read per render).  A 10 M-triangle
	// scene keeps 190 MB of nodes per device instead of 290.
	const bool wantFull = !sc.bvh.nodes4.empty() && n < RL_FLOAT_BOX_MAX_TRIS;
	const int32_t eager = EagerTree(sc);
	for (size_t slot = 0; slot < g_rt.devices.size(); ++slot) {
		DeviceSceneCopy* C = new DeviceSceneCopy;
		C->device = g_rt.devices[slot];
		memset(&C->view, 0, sizeof(C->view));
		D->copy.push_back(C);
		bool ok = hipSetDevice(C->device) == hipSuccess;
		ok = ok && Upload(C->nodes, sc.bvh.nodes.data(), sc.bvh.nodes.size());
		if (ok && eager == TREE_GRID4) ok = Upload(C->nodes4, sc.bvh.nodes4q.data(), sc.bvh.nodes4q.size());
		if (ok && eager == TREE_WIDE8) ok = Upload(C->nodes8, sc.bvh.nodes8.data(), sc.bvh.nodes8.size());
		if (ok && wantFull) ok = Upload(C->nodes4f, sc.bvh.nodes4.data(), sc.bvh.nodes4.size());
		if (ok && wantFull && !sc.bvh.leafList.empty()) ok = Upload(C->leafList, sc.bvh.leafList.data(), sc.bvh.leafList.size());
		ok = ok && Upload(C->isect, isect.data(), n) && Upload(C->shade, shade.data(), n);
		if (ok && !alphaTex.empty()) ok = Upload(C->alphaTex, alphaTex.data(), alphaTex.size());
		ok = ok && Upload(C->materials, mats.data(), mats.size()) && Upload(C->textures, texs.data(), texs.size()) && Upload(C->texels, pool.data(), pool.size());
		ok = ok && Upload(C->spheres, dsph.data(), dsph.size()) && Upload(C->cubes, dcub.data(), dcub.size());
		if (!ok) { Log("UploadScene: device %d could not take the scene", C->device); FreeScene(D); return false; }   // nothing of a failed upload is left behind
		DSceneView& V = C->view;
		V.nodes = C->nodes; V.nodes4 = C->nodes4; V.nodes4f = C->nodes4f; V.nodes8 = C->nodes8; V.isect = C->isect; V.shade = C->shade; V.alphaTex = C->alphaTex; V.materials = C->materials;
		V.textures = C->textures; V.numTextures = (int32_t)texs.size(); V.texels = C->texels; V.spheres = C->spheres; V.cubes = C->cubes;
		V.sunIlluminance[0] = sc.sunIlluminance.x; V.sunIlluminance[1] = sc.sunIlluminance.y; V.sunIlluminance[2] = sc.sunIlluminance.z;
		V.sunDirection[0] = sc.sunDirection.x; V.sunDirection[1] = sc.sunDirection.y; V.sunDirection[2] = sc.sunDirection.z;
		V.sky = nullptr; V.skyWidth = V.skyHeight = 0;
		V.hasSun = !(sc.sunIlluminance.x == 0.0f && sc.sunIlluminance.y == 0.0f && sc.sunIlluminance.z == 0.0f);   // renderer.cc:192
		V.numTriangles = (int32_t)n;
		V.numNodes4 = (int32_t)sc.bvh.nodes4.size(); V.numMaterials = (int32_t)mats.size();
		V.leafList = C->leafList; V.numLeafRecords = C->leafList ? (int32_t)sc.bvh.leafList.size() : 0;
		V.fastBary = fastBary.load();
		V.numNodes8 = (int32_t)sc.bvh.nodes8.size();

	}
	HIP_OK(hipSetDevice(g_rt.devices[0]));
	sc.device = D;
	return true;
}

// The sky panorama as it is NOW: the reference reads the image through the handle at every miss (renderer.cc:159-176), so pixels
// written after Raylib_FinalizeScene / Raylib_SetSkyPanorama are seen by the next render.  Only the sky texels move; triangles,
// BVH and textures stay where they are.  A frame that was rendered into the image and never left the device is copied on it.
bool SyncSky(Scene& sc)
{
	DeviceScene* D = sc.device;
	Image* sky = sc.sky;
	for (DeviceSceneCopy* C : D->copy) {
		if (!sky || (size_t)sky->width * sky->height == 0) { C->view.sky = nullptr; C->view.skyWidth = C->view.skyHeight = 0; C->skyImage = nullptr; continue; }
		if (C->skyImage == sky && C->skyVersion == sky->version && C->view.sky) continue;
		const size_t bytes = (size_t)sky->width * sky->height * sizeof(float4);
		(void)DrainLocked();   // a frame in flight reads the texels that are about to be replaced
		HIP_OK(hipSetDevice(C->device));
		if (!Grow(C->sky, C->skyBytes, bytes)) return false;
		if (sky->hostStale && sky->devValid && sky->devPixels) {
			HIP_OK(hipMemcpyPeer(C->sky, C->device, sky->devPixels, Rank0().device, bytes));   // images live on rank 0's device
		} else {
			HIP_OK(hipMemcpy(C->sky, sky->rgba.data(), bytes, hipMemcpyHostToDevice));
		}
		C->skyImage = sky; C->skyVersion = sky->version;
		C->view.sky = (const float*)C->sky; C->view.skyWidth = (int32_t)sky->width; C->view.skyHeight = (int32_t)sky->height;
	}
	HIP_OK(hipSetDevice(g_rt.devices[0]));
	return true;
}

// The kernels a render launches go by address (hipLaunchKernel): a one-view kernel and its views twin (RaylibAMD_RenderViews) differ by the twin's trailing DViews.
typedef void (*TraceKernel)(const DRenderParams, const DSceneView, const SkyRot, SampleRGB*, float*, unsigned long long*, unsigned int*);
typedef void (*TraceViewsKernel)(const DRenderParams, const DSceneView, const SkyRot, SampleRGB*, float*, unsigned long long*, unsigned int*, const DViews);
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
static std::atomic<int32_t> g_lastTracePlain{0};   // RaylibAMD_LastTracePlain

// What EnqueueFrame leaves for FinishRender: everything is queued on the rank's stream, nothing has been waited for.
struct PendingRender {
	bool pathTrace = false, lastBatchPending = false;
	float traceMs = 0.0f;
	uint32_t launches = 0, jobHeads = 0, pathsPerWave = 64, treeWidth = 2, nodeBytes = 64;   // (the last three: TracePlan's)
	uint64_t pixels = 0;
	uint64_t culledSamples = 0; uint32_t culledRaysPerSample = 0, culledSkyTexels = 0;   // camera samples of cells outside the scene's silhouette: reported apart, not traced (CullCells)
	uint32_t culledCells = 0, listedCells = 0;
	bool enqueuedToEnd = false;                // EnqueueFrame reached the ev[slot][7] record (FinishRender waits for it; otherwise for the whole stream)
	float4* out = nullptr; size_t outBytes = 0;
	int slot = 0;                              // frame slot: which of the rank's event sets / pinned counter buffers this render uses
	const unsigned long long* cnt = nullptr;   // -> the rank's cntHost[slot], valid once ev[slot][7] has fired
};

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
static bool TraceView(DeviceSceneCopy* D, const Scene& sc, const TracePlan& plan, DSceneView& view)
{
	if (!EnsureWideTree(D, sc, plan.tree)) return false;
	view = D->view;
	if (!plan.keepNodes4) view.nodes4 = nullptr;
	if (!plan.keepNodes4f) view.nodes4f = nullptr;
	return true;
}

// workgroups of `kernel` a CU holds, asked once per kernel and rank; -1: the query failed (logged).  RAYLIB_PRINT_OCCUPANCY: a megakernel's first answer is logged.
static int OccupancyOf(RankCtx& R, const void* kernel, const TracePlan* megakernel = nullptr)
{
	auto it = R.occupancy.find(kernel);
	if (it != R.occupancy.end()) return it->second;
	int blocksPerCU = 0;
	const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocksPerCU, kernel, RL_BLOCK, 0);
	if (e != hipSuccess) { Log("HIP error %s: hipOccupancyMaxActiveBlocksPerMultiprocessor", hipGetErrorName(e)); return -1; }
	R.occupancy[kernel] = blocksPerCU;
	if (megakernel && getenv("RAYLIB_PRINT_OCCUPANCY")) Log("megakernel (%u paths per lane, tree width %u): %d workgroups per CU", megakernel->pathsPerWave / 64u, megakernel->treeWidth, blocksPerCU);
	return blocksPerCU;
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
	pend.pathTrace = F.plan.pathTrace; pend.slot = q; pend.cnt = R.cntHost[q];
	pend.out = F.out; pend.outBytes = outBytes;
	HIP_OK(hipMemsetAsync(R.counters, 0, (CNT_COUNT + 24 + RL_TIMELINE_SLOTS) * sizeof(unsigned long long), R.stream));
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
		void* args[] = { &P, &F.view, &F.out, &R.counters, (void*)F.views };
		HIP_OK(hipLaunchKernel(AovKernelFor(plan, F.views != nullptr), dim3(rblocks), dim3(RL_BLOCK), args, 0, R.stream));
	} else {
		const void* traceKernel = KernelFor(plan, F.views != nullptr);
		if (!traceKernel) { Log("Raylib_Render: no megakernel instance for STACK %d, K %d, stack in LDS %d", plan.stack, plan.poolK, plan.lstack); return false; }
		const int blocksPerCU = OccupancyOf(R, traceKernel, &plan);
		if (blocksPerCU < 0) return false;
		g_lastTracePlain.store(plan.plain ? 1 : 0, std::memory_order_relaxed);
		pend.pathsPerWave = plan.pathsPerWave; pend.treeWidth = plan.treeWidth; pend.nodeBytes = plan.nodeBytes;
		pend.culledCells = F.numLive - F.numActive; pend.listedCells = F.numActive;
		const uint32_t batch = PlanLaunch(numCells, F.numActive, F.sEnd, F.sBegin, R.numCUs, blocksPerCU, plan, F.knobs).batch;
		if (!Grow(R.samples, R.samplesBytes, (size_t)numSlots * sizeof(SampleRGB) * std::min(batch, F.sEnd - F.sBegin))) return false;
		if (F.accum && batch < P.spp && !Grow(R.accum, R.accumBytes, (size_t)numSlots * sizeof(float4))) return false;
		const int depthSlots = P.maxPathLength > 1 ? P.maxPathLength : 1;
		void* traceArgs[] = { &P, &F.view, &skyRot, &R.samples, &R.pathStack, &R.counters, &R.jobCounter, (void*)F.views };
		void* resolveArgs[] = { &P, &F.view, &skyRot, &R.samples, F.resolveArgs[0], F.resolveArgs[1], F.resolveArgs[2], F.resolveArgs[3], F.resolveArgs[4] };
		for (uint32_t s0 = F.sBegin; s0 < F.sEnd; s0 += batch) {
			const LaunchPlan L = PlanLaunch(numCells, F.numActive, F.sEnd, s0, R.numCUs, blocksPerCU, plan, F.knobs);
			const uint32_t cnt = L.sampleCount;
			P.sampleBegin = s0; P.sampleCount = cnt;
			P.magicSamples = cnt > 1 ? (uint32_t)(0x100000000ull / cnt) : 0xFFFFFFFFu;
			if (L.jobs > 0xF0000000ull) { Log("Raylib_Render: job count overflow"); return false; }   // (a head overshoots its band by one chunk per wave and attempt)
			P.numJobs = (uint32_t)L.jobs;
			P.stackStride = L.stackStride; P.jobChunk = L.jobChunk;
			P.numHeads = L.heads; P.jobsPerHead = L.jobsPerHead; P.guideShift = L.guideShift;
			if (!Grow(R.pathStack, R.pathStackBytes, (size_t)depthSlots * 8 * P.stackStride * sizeof(float))) return false;
			pend.jobHeads = L.heads;
			F.firstBatch = s0 == F.sBegin; F.lastBatch = s0 + cnt >= F.sEnd;
			HIP_OK(hipMemsetAsync(R.jobCounter, 0, RL_MAX_HEADS * RL_HEAD_STRIDE * sizeof(unsigned int), R.stream));   // heads count from their band's first job: one memset
			HIP_OK(hipEventRecord(R.ev[q][2], R.stream));
			if (L.jobs > 0)   // (else no cell of this frame sees the scene: the resolve has all it needs)
				HIP_OK(hipLaunchKernel(traceKernel, dim3(L.blocks), dim3(RL_BLOCK), traceArgs, 0, R.stream));
			HIP_OK(hipEventRecord(R.ev[q][3], R.stream));
			HIP_OK(hipLaunchKernel(F.resolve, dim3(rblocks), dim3(RL_BLOCK), resolveArgs, 0, R.stream));
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
			                   S->live, S->trace, (const uint8_t*)S->st.stopped, (const uint8_t*)S->empty, S->numLive, P.width, P.height, P.cellsX, S->counts);
			HIP_OK(hipGetLastError());
			HIP_OK(hipMemcpyAsync(S->countsHost, S->counts, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, R.stream));
		}
	}
	if (!plan.pathTrace) pend.listedCells = numCells;
	HIP_OK(hipEventRecord(R.ev[q][1], R.stream));
	HIP_OK(hipMemcpyAsync(R.cntHost[q], R.counters, (CNT_COUNT + 24) * sizeof(unsigned long long), hipMemcpyDeviceToHost, R.stream));
	HIP_OK(hipEventRecord(R.ev[q][7], R.stream));
	pend.enqueuedToEnd = true;
	return true;
}

// One rank's share of a one-view render, queued on its stream (BeginFrame, EnqueueFrame).  `req.outDevice` receives the row-major frame (cellStride 1) or the rank's cells
// back to back.  The job list is the cull's, cached per frame slot.
// With `prog` (rank 0, the whole frame): one pass of a progressive session -- the samples [prog->samples, prog->passEnd) of its live cells, its lists in place
// of the cull's (seeded from the cull at its first pass), k_progressive_resolve in place of k_resolve, and k_progressive_compact behind the last batch.
bool EnqueueRender(RankCtx& R, Scene& sc, const RenderRequest& req, PendingRender& pend, ProgressiveSession* prog = nullptr)
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
	if (!F.out) { if (!Grow(R.image, R.imageBytes, outBytes ? outBytes : 16)) return false; F.out = R.image; }
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
					if (R.cellListHost[q]) { (void)hipHostFree(R.cellListHost[q]); R.cellListHost[q] = nullptr; }
					if (R.cellList[q]) { (void)hipFree(R.cellList[q]); R.cellList[q] = nullptr; }
					R.cellListCells[q] = 0;
					// the list (uint32 per cell) and the flags (one byte per cell, behind it) in one buffer
					HIP_OK(hipHostMalloc((void**)&R.cellListHost[q], (size_t)numLocalCells * 5 + 16, hipHostMallocDefault));
					HIP_OK(hipMalloc((void**)&R.cellList[q], (size_t)numLocalCells * 5 + 16));
					R.cellListCells[q] = numLocalCells;
				}
				// (the slot's staging buffer is free: the frame that used it last has been waited for -- FinishRender, or FinishInflight before a slot is re-used)
				memcpy(R.cellListHost[q], cr.active.data(), cr.active.size() * sizeof(uint32_t));
				memcpy((unsigned char*)(R.cellListHost[q] + R.cellListCells[q]), cr.empty.data(), numLocalCells);
				HIP_OK(hipMemcpyAsync(R.cellList[q], R.cellListHost[q], (size_t)R.cellListCells[q] * 5, hipMemcpyHostToDevice, R.stream));
				R.cullActive[q] = (uint32_t)cr.active.size(); R.cullEmptyPixels[q] = cr.emptyPixels;
				R.cullL[q][0] = cr.L[0]; R.cullL[q][1] = cr.L[1]; R.cullL[q][2] = cr.L[2]; R.cullRays[q] = cr.raysPerSample;
			}
			R.cullKey[q] = key;
		}
		const uint32_t* list = R.cellList[q]; const uint8_t* empty = (const uint8_t*)(R.cellList[q] + R.cellListCells[q]);
		if (!prog) {
			if (R.cullActive[q] < numLocalCells) ListCells(F, pend, list, empty, R.cullActive[q], numLocalCells, R.cullL[q], R.cullEmptyPixels[q], R.cullRays[q]);
		} else {   // the session's first pass: its lists start from the cull's (every cell is live)
			if (R.cullActive[q] < numLocalCells) {
				HIP_OK(hipMemcpyAsync(prog->trace, list, (size_t)R.cullActive[q] * sizeof(uint32_t), hipMemcpyDeviceToDevice, R.stream));
				HIP_OK(hipMemcpyAsync(prog->empty, empty, numLocalCells, hipMemcpyDeviceToDevice, R.stream));
				prog->emptyLivePixels = R.cullEmptyPixels[q]; prog->culledRays = R.cullRays[q];
				for (int k = 0; k < 3; ++k) prog->emptyL[k] = R.cullL[q][k];
			}
			prog->numLive = numLocalCells; prog->numTrace = R.cullActive[q];
			prog->seeded = true;
		}
	}
	if (prog) {
		if (F.plan.pathTrace && numLocalCells) ListCells(F, pend, prog->trace, prog->empty, prog->numTrace, prog->numLive, prog->emptyL, prog->emptyLivePixels, prog->culledRays);
		F.resolve = (const void*)k_progressive_resolve; F.resolveArgs[0] = &prog->st; F.resolveArgs[1] = &F.out; F.resolveArgs[2] = &F.lastBatch;
		F.accum = false; F.compact = prog;
	} else {
		F.resolve = (const void*)k_resolve; F.resolveArgs[0] = &R.accum; F.resolveArgs[1] = &F.out; F.resolveArgs[2] = &F.firstBatch; F.resolveArgs[3] = &F.lastBatch;
	}
	if (!EnqueueFrame(R, q, *sc.device, F, pend)) return false;
	pend.pixels = CoveredPixels(W, H, req.cellFirst, stride, numLocalCells);   // (counted while the device works)
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
	stats.pathsPerWave = pend.pathsPerWave; stats.treeWidth = pend.treeWidth; stats.nodeBytes = pend.nodeBytes;
	stats.pixels += pend.pixels;
	stats.kernelMs = std::max(stats.kernelMs, (double)totalMs);
	stats.traceKernelMs = std::max(stats.traceKernelMs, (double)(pend.pathTrace ? pend.traceMs : totalMs));
	stats.traceLaunches = std::max(stats.traceLaunches, pend.pathTrace ? pend.launches : 1u);
	if (R.rank >= 0 && R.rank < 16) { stats.rankKernelMs[R.rank] = (double)totalMs; stats.rankTraceMs[R.rank] = (double)(pend.pathTrace ? pend.traceMs : totalMs); }
	if (pend.jobHeads) stats.jobHeads = pend.jobHeads;
#ifdef RL_DIAG_TIMELINE
	if (getenv("RAYLIB_PRINT_STAMPS")) {
		std::vector<unsigned long long> tl(RL_TIMELINE_SLOTS);
		HIP_OK(hipMemcpy(tl.data(), R.counters + CNT_COUNT + 24, tl.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
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

// ---- whole frames over N ranks -------------------------------------------------------------------------------------
// cells round-robin, one gather to rank 0's device, one scatter kernel -- and up to two frames in flight: Raylib_Render returns when frame i
// is ENQUEUED on every rank's stream (after waiting for frame i - 1's predecessor, whose buffers frame i reuses), so that while rank 0's gather
// stream still receives and assembles frame i the ranks already render frame i + 1.  Whoever reads the pixels, the stats or changes anything
// a frame in flight uses goes through DrainLocked() first: to a front-end the call is as synchronous as the reference's (raylib.cc:231-239),
// it just finds out later.  RAYLIB_PIPELINE=0 waits at the end of every call.
struct Runtime::Inflight {
	std::vector<PendingRender> pend;
	RaylibAMDStats stats;                 // what is known when the frame is enqueued; FinishInflight adds counters and times
	int slot = 0;
	bool ok = true, timed = false;
	std::chrono::steady_clock::time_point t0;
};
RaylibAMDStats g_deferredStats;           // of the last frame FinishInflight completed
bool g_deferredUnreported = false;

bool FinishInflight(int slot)
{
	Runtime& R = g_rt;
	Runtime::Inflight* F = R.inflight[slot];
	if (!F) return true;
	R.inflight[slot] = nullptr;
	RankCtx& R0 = Rank0();
	bool ok = F->ok;
	for (int r = (int)F->pend.size() - 1; r >= 0; --r) {
		ok = FinishRender(*R.ranks[(size_t)r], F->pend[(size_t)r], F->stats) && ok;   // (a rank whose enqueue failed: its stream is drained)
	}
	(void)hipSetDevice(R0.device);
	if (F->timed) {
		if (hipEventSynchronize(R0.ev[slot][6]) != hipSuccess) ok = false;   // frame assembled (and copied to the host, if asked for)
		float g = 0.0f, sc = 0.0f;
		if (hipEventElapsedTime(&g, R0.ev[slot][1], R0.ev[slot][5]) == hipSuccess) F->stats.gatherMs = (double)g;
		if (hipEventElapsedTime(&sc, R0.ev[slot][5], R0.ev[slot][6]) == hipSuccess) F->stats.scatterMs = (double)sc;
	} else if (R.gatherStream) (void)hipStreamSynchronize(R.gatherStream);
	F->stats.wallMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - F->t0).count();
	g_deferredStats = F->stats; g_deferredUnreported = true;
	delete F;
	return ok;
}
// waits for every frame in flight (oldest first); the runtime lock is held by the caller
bool DrainLocked()
{
	Runtime& R = g_rt;
	if (!R.ok) return true;
	const int older = (int)(R.frameNo & 1);   // the slot the NEXT frame would take holds the older of two frames in flight
	bool ok = FinishInflight(older);
	return FinishInflight(older ^ 1) && ok;
}

bool RenderMulti(Scene& sc, const RenderRequest& req, RaylibAMDStats& stats, bool& deferred)
{
	Runtime& R = g_rt;
	const int N = (int)R.ranks.size();
	RankCtx& R0 = Rank0();
	const int b = (int)(R.frameNo & 1);
	deferred = false;
	// this slot's previous frame (two calls ago) gives up its buffers, events and counter blocks
	bool ok = FinishInflight(b);
	const uint32_t W = req.settings.viewportWidth, H = req.settings.viewportHeight;
	const uint32_t cellsX = (W + 7) / 8, numCells = cellsX * ((H + 7) / 8);
	ScatterPlan plan; memset(&plan, 0, sizeof(plan));
	plan.ranks = (uint32_t)N;
	std::vector<uint32_t> local((size_t)N);
	uint32_t total = 0;
	for (int r = 0; r < N; ++r) {
		local[(size_t)r] = (uint32_t)r < numCells ? (numCells - (uint32_t)r + (uint32_t)N - 1) / (uint32_t)N : 0;
		plan.offset[r] = total * 64u;
		total += local[(size_t)r];
	}
	HIP_OK(hipSetDevice(R0.device));
	if (!Grow(R.gather[b], R.gatherBytes[b], std::max<size_t>(16, (size_t)total * 64 * sizeof(float4)))) return false;
	float4* out = (float4*)req.outDevice;
	const size_t frameBytes = (size_t)W * H * sizeof(float4);
	if (!out) {
		if (frameBytes > R0.imageBytes) ok = FinishInflight(b ^ 1) && ok;   // the frame in flight may be writing the library's own image: not while it is re-allocated
		if (!Grow(R0.image, R0.imageBytes, frameBytes)) return false;
		out = R0.image;
	}

	// which ranks need a copy: those on another device than rank 0 (and rank 0 itself under RAYLIB_GATHER_SELF)
	std::vector<char> remote((size_t)N, 0);
	bool anyRemote = false;
	for (int r = 0; r < N; ++r) { remote[(size_t)r] = (R.ranks[(size_t)r]->device != R0.device) || (r == 0 && R.gatherSelf); anyRemote = anyRemote || remote[(size_t)r]; }
	const bool useRccl = anyRemote && R.wantRccl && EnsureRccl();

	// From here on work is enqueued that only FinishInflight waits for: no early return -- a failing call clears `ok` (HIP_TRY) and the function still
	// reaches the place that registers the frame and drains every stream.
	Runtime::Inflight* F = new Runtime::Inflight;
	F->pend.resize((size_t)N);
	F->slot = b; F->t0 = std::chrono::steady_clock::now();
	memset(&F->stats, 0, sizeof(F->stats));
	std::vector<PendingRender>& pend = F->pend;
	float4* gather = R.gather[b];
	auto run = [&](int r) -> bool {
		RankCtx& C = *R.ranks[(size_t)r];
		HIP_OK(hipSetDevice(C.device));
		RenderRequest q = req;
		q.cellFirst = (uint32_t)r; q.cellStride = (uint32_t)N; q.cellMajor = true; q.outHostRGBA = nullptr; q.slot = b;
		const size_t bytes = (size_t)local[(size_t)r] * 64 * sizeof(float4);
		float4* dst = gather + plan.offset[r];
		if (remote[(size_t)r]) { if (!Grow(C.cells, C.cellsBytes, std::max<size_t>(16, bytes))) return false; q.outDevice = C.cells; }
		else q.outDevice = dst;   // same device as rank 0: rendered in place, nothing to move
		if (!EnqueueRender(C, sc, q, pend[(size_t)r])) return false;
		if (remote[(size_t)r] && !useRccl && bytes) HIP_OK(hipMemcpyPeerAsync(dst, R0.device, C.cells, C.device, bytes, C.stream));
		HIP_OK(hipEventRecord(C.ev[b][4], C.stream));
		return true;
	};
	for (int r = 1; r < N; ++r) R.ranks[(size_t)r]->worker->Post([&run, r]() { return run(r); });
	ok = run(0) && ok;
	for (int r = 1; r < N; ++r) ok = R.ranks[(size_t)r]->worker->Wait() && ok;
	HIP_TRY(hipSetDevice(R0.device));
	if (ok && useRccl) {
		// one group: rank 0's GATHER stream receives every remote rank's cells, each remote rank's stream sends them (behind its kernels)
		RcclApi& A = R.rccl;
		// One stream per communicator inside the group: all ranks of a device send on the stream of that device's FIRST rank (the lead), which waits
		// for the others' kernels; rank 0 sending to itself (RAYLIB_GATHER_SELF, tests) sends and receives on the gather stream.  Afterwards the
		// other ranks' streams wait for the lead's sends, so that their next frame does not overwrite cells that are still being sent.
		std::vector<int> lead(R.devices.size(), -1);
		for (int r = 0; r < N; ++r) if (remote[(size_t)r] && local[(size_t)r] && lead[(size_t)R.ranks[(size_t)r]->devSlot] < 0) lead[(size_t)R.ranks[(size_t)r]->devSlot] = r;
		auto sendStream = [&](const RankCtx& C) { return C.devSlot == R0.devSlot ? R.gatherStream : R.ranks[(size_t)lead[(size_t)C.devSlot]]->stream; };
		for (int r = 0; r < N; ++r) {
			RankCtx& C = *R.ranks[(size_t)r];
			if (!remote[(size_t)r] || !local[(size_t)r] || lead[(size_t)C.devSlot] == r) continue;
			(void)hipSetDevice(C.device);
			HIP_TRY(hipStreamWaitEvent(sendStream(C), C.ev[b][4], 0));
		}
		if (remote[0] && local[0]) { (void)hipSetDevice(R0.device); HIP_TRY(hipStreamWaitEvent(R.gatherStream, R0.ev[b][4], 0)); }
		int rc = A.GroupStart();
		for (int r = 0; r < N && rc == 0; ++r) {
			if (!remote[(size_t)r] || !local[(size_t)r]) continue;
			RankCtx& C = *R.ranks[(size_t)r];
			const size_t floats = (size_t)local[(size_t)r] * 64 * 4;
			rc = A.Recv(gather + plan.offset[r], floats, kRcclFloat, C.devSlot, A.comms[(size_t)R0.devSlot], R.gatherStream);
			if (rc == 0) rc = A.Send(C.cells, floats, kRcclFloat, R0.devSlot, A.comms[(size_t)C.devSlot], sendStream(C));
		}
		const int rcEnd = A.GroupEnd();
		if (rc != 0 || rcEnd != 0) { Log("Raylib_Render: RCCL gather failed (%s)", A.GetErrorString ? A.GetErrorString(rc ? rc : rcEnd) : "?"); ok = false; }
		for (size_t sl = 0; sl < lead.size() && ok; ++sl) {
			if (lead[sl] < 0 || (int)sl == R0.devSlot) continue;
			RankCtx& L = *R.ranks[(size_t)lead[sl]];
			(void)hipSetDevice(L.device);
			HIP_TRY(hipEventRecord(L.ev[b][5], L.stream));   // (slots 5 and 6 belong to rank 0 on ITS device; a lead of another device uses its own 5 for "sends done")
			for (int r = 0; r < N; ++r) if (r != lead[sl] && remote[(size_t)r] && R.ranks[(size_t)r]->devSlot == (int)sl) HIP_TRY(hipStreamWaitEvent(R.ranks[(size_t)r]->stream, L.ev[b][5], 0));
		}
		(void)hipSetDevice(R0.device);
	}
	if (ok) {
		// the gather stream waits for every rank's "my cells are there" (rank 0's own render included), assembles the frame, and rank 0's
		// render stream is free for the next frame meanwhile
		for (int r = 0; r < N; ++r) HIP_TRY(hipStreamWaitEvent(R.gatherStream, R.ranks[(size_t)r]->ev[b][4], 0));
		HIP_TRY(hipEventRecord(R0.ev[b][5], R.gatherStream));
		const uint32_t blocks = (uint32_t)(((size_t)W * H + RL_BLOCK - 1) / RL_BLOCK);
		hipLaunchKernelGGL(k_scatter_cells, dim3(blocks), dim3(RL_BLOCK), 0, R.gatherStream, (const float4*)gather, out, W, H, cellsX, plan);
		HIP_TRY(hipGetLastError());
		if (req.outHostRGBA) HIP_TRY(hipMemcpyAsync(req.outHostRGBA, out, frameBytes, hipMemcpyDeviceToHost, R.gatherStream));
		HIP_TRY(hipEventRecord(R0.ev[b][6], R.gatherStream));
		if (remote[0] && useRccl) HIP_TRY(hipStreamWaitEvent(R0.stream, R0.ev[b][5], 0));   // rank 0's self-send has read its cell buffer before the next render writes it
		F->timed = ok;   // (events 5 and 6 are only read when both were recorded)
	}
	F->ok = ok;
	F->stats.ranks = (uint32_t)N; F->stats.devices = (uint32_t)R.devices.size();
	F->stats.gatherMode = !anyRemote ? 0u : (useRccl ? 1u : 2u);
	F->stats.rcclCommSize = R.rccl.ok ? (uint32_t)R.rccl.comms.size() : 0u;
	F->stats.numNodes = (uint32_t)sc.bvh.nodes.size(); F->stats.numTriangles = (uint32_t)sc.triangles.size(); F->stats.bvhDepth = sc.bvh.depth;
	R.inflight[b] = F;
	++R.frameNo;
	if (!ok || !R.pipeline || req.outHostRGBA || req.callerOwnsOut) {
		// synchronous after all: a failure (every stream is drained whatever happened), the switch, pixels wanted in host memory now, or a frame
		// into device memory of the caller's (RaylibAMD_RenderDevice: "the library's stream has been synchronised when it returns" -- nothing the
		// library owns would keep a reader or a free of that buffer behind the gather stream's scatter)
		ok = DrainLocked() && ok;
		stats = g_deferredStats; g_deferredUnreported = false;
		return ok;
	}
	stats = F->stats;   // counters and times follow when the frame is waited for (RaylibAMD_GetLastStats, any reader of the pixels, the call after next)
	deferred = true;
	return ok;
}

} // namespace

bool DeviceAvailable()
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	return EnsureRuntime();
}

int DeviceNumRanks()
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	return EnsureRuntime() ? (int)g_rt.ranks.size() : 0;
}

bool DeviceRender(Scene& sc, const RenderRequest& req, RaylibAMDStats& stats)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	const auto t0 = std::chrono::steady_clock::now();
	if (!EnsureRuntime()) return false;
	HIP_OK(hipSetDevice(Rank0().device));
	if (!UploadScene(sc)) return false;
	if (!SyncSky(sc)) return false;
	bool ok;
	const bool whole = req.cellFirst == 0 && (req.cellStride == 0 || req.cellStride == 1);
	if (whole && (g_rt.ranks.size() > 1 || g_rt.gatherSelf)) {
		bool deferred = false;
		ok = RenderMulti(sc, req, stats, deferred);
		if (deferred) return ok;    // scene numbers are in; counters, times and wallMs follow at the drain
	} else {
		(void)DrainLocked();        // this path uses rank 0's slot-0 events and counter block
		g_deferredUnreported = false;   // ... and its numbers are the ones the caller reads next
		PendingRender pend;
		ok = EnqueueRender(Rank0(), sc, req, pend);
		if (ok && req.outHostRGBA) HIP_OK(hipMemcpyAsync(req.outHostRGBA, pend.out, pend.outBytes, hipMemcpyDeviceToHost, Rank0().stream));
		ok = FinishRender(Rank0(), pend, stats) && ok;
		stats.ranks = 1; stats.devices = 1;
	}
	stats.numNodes = (uint32_t)sc.bvh.nodes.size(); stats.numTriangles = (uint32_t)sc.triangles.size(); stats.bvhDepth = sc.bvh.depth;
	if (!(whole && (g_rt.ranks.size() > 1 || g_rt.gatherSelf))) stats.wallMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return ok;
}

int32_t DeviceLastTracePlain() { return g_lastTracePlain.load(std::memory_order_relaxed); }

// ---- several views of one scene (RaylibAMD_RenderViews): rank 0's device and stream, whatever RAYLIB_NUM_GPUS says, as a progressive session ----
// The batch's output is ONE buffer, view-major (view v's row-major frame at v * W * H); the images get theirs by device-to-device copies behind the
// resolve.  The cull's list and flags and the camera table go through buffers of their own: the one-view renders' cached lists (RankCtx::cullKey) are
// never those of a batch, nor the reverse.
namespace {
struct ViewsBuffers {
	unsigned char* host = nullptr; size_t hostBytes = 0;   // pinned staging: the camera table, the list of listed cells, the flags
	unsigned char* dev = nullptr; size_t devBytes = 0;
	float4* out = nullptr; size_t outBytes = 0;             // the library's own output (RaylibAMD_RenderViewsDevice with no buffer of the caller's, and the images')
};
ViewsBuffers g_views;
}

bool DeviceRenderViews(Scene& sc, const RenderRequest& req, const DCamera* cameras, uint32_t count, void* outDevice, void* const* imagePixels, RaylibAMDStats& stats)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	const auto t0 = std::chrono::steady_clock::now();
	if (!EnsureRuntime() || count == 0 || count > RL_MAX_VIEWS) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (!UploadScene(sc) || !SyncSky(sc)) return false;
	(void)DrainLocked();            // rank 0's slot-0 events, counter block and work buffers
	g_deferredUnreported = false;   // (the numbers the caller reads next are this batch's)
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
	if (g_views.hostBytes < stageBytes) {
		if (g_views.host) (void)hipHostFree(g_views.host);
		g_views.host = nullptr; g_views.hostBytes = 0;
		HIP_OK(hipHostMalloc((void**)&g_views.host, stageBytes, hipHostMallocDefault));
		g_views.hostBytes = stageBytes;
	}
	if (!Grow(g_views.dev, g_views.devBytes, stageBytes)) return false;
	memcpy(g_views.host, cameras, camBytes);
	PendingRender pend;
	if (culled) {
		memcpy(g_views.host + listAt, VP.active.data(), VP.active.size() * sizeof(uint32_t));
		memcpy(g_views.host + flagsAt, VP.empty.data(), numCells);
		ListCells(F, pend, (const uint32_t*)(g_views.dev + listAt), (const uint8_t*)(g_views.dev + flagsAt), VP.numActive, numCells, VP.emptyL, VP.emptyPixels, VP.raysPerSample);
	}
	F.out = (float4*)outDevice;
	if (!F.out) { if (!Grow(g_views.out, g_views.outBytes, viewBytes * count)) return false; F.out = g_views.out; }
	DViews V;
	V.cameras = (const DCamera*)g_views.dev; V.cellsPerView = cellsPerView;
	V.magicCellsPerView = cellsPerView > 1 ? (uint32_t)(0x100000000ull / cellsPerView) : 0xFFFFFFFFu;
	F.views = &V;
	F.resolve = (const void*)k_resolve_views;
	F.resolveArgs[0] = &R.accum; F.resolveArgs[1] = &F.out; F.resolveArgs[2] = &F.firstBatch; F.resolveArgs[3] = &F.lastBatch; F.resolveArgs[4] = &V;

	auto enqueue = [&]() -> bool {   // the staged tables, the frame, and behind it every image's copy of its view
		HIP_OK(hipMemcpyAsync(g_views.dev, g_views.host, stageBytes, hipMemcpyHostToDevice, R.stream));
		if (!BeginFrame(R, 0, F, viewBytes * count, pend) || !EnqueueFrame(R, 0, *sc.device, F, pend)) return false;
		if (imagePixels)
			for (uint32_t v = 0; v < count; ++v) HIP_OK(hipMemcpyAsync(imagePixels[v], (const char*)F.out + viewBytes * v, viewBytes, hipMemcpyDeviceToDevice, R.stream));
		pend.pixels = CoveredPixels(W, H, 0, 1, cellsPerView) * count;
		return true;
	};
	bool ok = enqueue();
	ok = FinishRender(R, pend, stats) && ok;
	HIP_OK(hipStreamSynchronize(R.stream));   // (the images' copies)
	stats.ranks = 1; stats.devices = 1;
	stats.numNodes = (uint32_t)sc.bvh.nodes.size(); stats.numTriangles = (uint32_t)sc.triangles.size(); stats.bvhDepth = sc.bvh.depth;
	stats.wallMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return ok;
}

// Waits for whatever Raylib_Render left in flight.  True with `out` filled when that completed the LAST render call's numbers (counters, times)
// that the call itself could not report yet.
bool DeviceDrain(RaylibAMDStats* out)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!g_rt.ok) return false;
	(void)DrainLocked();
	if (!g_deferredUnreported) return false;
	g_deferredUnreported = false;
	if (out) *out = g_deferredStats;
	return true;
}

bool DeviceClosestHit(Scene& sc, const float* rays, int32_t n, float tMin, void* outHits)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (sc.bvh.depth > 64) { Log("RaylibAMD_ClosestHit: BVH depth %u exceeds the traversal stack (64)", sc.bvh.depth); return false; }
	if (!UploadScene(sc)) return false;
	if (n <= 0) return true;
	float* dRays = nullptr; DHitOut* dOut = nullptr;
	HIP_OK(hipMalloc(&dRays, (size_t)n * 6 * sizeof(float)));
	if (hipMalloc(&dOut, (size_t)n * sizeof(DHitOut)) != hipSuccess) { (void)hipFree(dRays); Log("RaylibAMD_ClosestHit: out of device memory"); return false; }
	const DSceneView& view = sc.device->copy[(size_t)R.devSlot]->view;
	bool ok = hipMemcpy(dRays, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
	if (ok) {
		const uint32_t blocks = ((uint32_t)n + RL_BLOCK - 1) / RL_BLOCK;
		if (sc.bvh.depth <= 32) hipLaunchKernelGGL((k_closest_hit<32, true>), dim3(blocks), dim3(RL_BLOCK), 0, R.stream, view, dRays, n, tMin, dOut);
		else hipLaunchKernelGGL((k_closest_hit<64, true>), dim3(blocks), dim3(RL_BLOCK), 0, R.stream, view, dRays, n, tMin, dOut);
		ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(R.stream) == hipSuccess;
		ok = ok && hipMemcpy(outHits, dOut, (size_t)n * sizeof(DHitOut), hipMemcpyDeviceToHost) == hipSuccess;
	}
	(void)hipFree(dRays); (void)hipFree(dOut);
	if (!ok) Log("RaylibAMD_ClosestHit: a HIP call failed");
	return ok;
}

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

// a device pointer the query may use: memory of rank 0's device
static bool OnDevice(const void* p, int device)
{
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
	return (a.type == hipMemoryTypeDevice || a.isManaged) && a.device == device;
}

bool DeviceTraceRays(Scene& sc, int32_t kind, const void* rays, int32_t n, float rayTime, void* out, int32_t* outPrim, bool hostMem, void* stream,
                     RaylibAMDStats& stats)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	const QueryPlan plan = PlanQuery(sc, kind, ReadRenderKnobs());
	if (!plan.ok) { Log("RaylibAMD_TraceRays: BVH depth %u exceeds the traversal stack (64)", sc.bvh.depth); return false; }
	const size_t outBytes = (size_t)n * (kind == RAYLIB_AMD_QUERY_ANY ? sizeof(uint32_t) : kind == RAYLIB_AMD_QUERY_CLOSEST ? sizeof(DQueryHit) : sizeof(DHitOut));
	if (!hostMem && n > 0) {
		if (!OnDevice(rays, R.device) || !OnDevice(out, R.device) || (outPrim && kind == RAYLIB_AMD_QUERY_SURFACE && !OnDevice(outPrim, R.device))) {
			Log("RaylibAMD_TraceRaysDevice: a pointer is not device memory of device %d", R.device);
			return false;
		}
		// the kernel reads a ray as two 16-byte loads and writes a RaylibAMDHitT as one 16-byte store, the other records as 4-byte words
		if (((uintptr_t)rays & 15u) != 0) { Log("RaylibAMD_TraceRaysDevice: the rays are not 16-byte aligned"); return false; }
		const uintptr_t outAlign = kind == RAYLIB_AMD_QUERY_CLOSEST ? 15u : 3u;
		if (((uintptr_t)out & outAlign) != 0 || ((uintptr_t)outPrim & 3u) != 0) { Log("RaylibAMD_TraceRaysDevice: the output is not %u-byte aligned", (unsigned)outAlign + 1u); return false; }
	}
	if (!UploadScene(sc)) return false;
	DeviceSceneCopy* Cp = sc.device->copy[(size_t)R.devSlot];
	if (!EnsureWideTree(Cp, sc, plan.tree)) return false;
	const bool wantPrim = kind == RAYLIB_AMD_QUERY_CLOSEST || (kind == RAYLIB_AMD_QUERY_SURFACE && outPrim);
	if (wantPrim && !Cp->slotIndex && !sc.bvh.triOrder.empty()) {
		std::vector<int32_t> idx(sc.bvh.triOrder.begin(), sc.bvh.triOrder.end());
		int32_t* p = nullptr;
		if (!Upload(p, idx.data(), idx.size())) { if (p) (void)hipFree(p); return false; }
		Cp->slotIndex = p;
	}
	const hipStream_t st = stream ? (hipStream_t)stream : R.stream;
	const bool sync = !stream;
	if (!R.qRing) {
		HIP_OK(hipMalloc(&R.qRing, RL_QUERY_RING * sizeof(unsigned int)));
		for (int k = 0; k < RL_QUERY_RING; ++k) HIP_OK(hipEventCreateWithFlags(&R.qRingEv[k], hipEventDisableTiming));
	}
	const uint32_t slot = R.qRingNext;
	if (R.qRingUsed[slot]) HIP_OK(hipEventSynchronize(R.qRingEv[slot]));   // RL_QUERY_RING launches ago: long done, unless a caller's stream is that far behind
	unsigned int* counter = R.qRing + slot;
	if (sync && !R.qStats) {
		HIP_OK(hipMalloc(&R.qStats, 8 * sizeof(unsigned long long)));
		HIP_OK(hipHostMalloc(&R.qStatsHost, 8 * sizeof(unsigned long long), hipHostMallocDefault));
		HIP_OK(hipEventCreate(&R.qEv[0])); HIP_OK(hipEventCreate(&R.qEv[1]));
	}
	memset(&stats, 0, sizeof(stats));
	stats.treeWidth = plan.treeWidth; stats.nodeBytes = plan.nodeBytes; stats.ranks = 1; stats.devices = 1;
	stats.numNodes = (uint32_t)sc.bvh.nodes.size(); stats.numTriangles = (uint32_t)sc.triangles.size(); stats.bvhDepth = sc.bvh.depth;
	if (n == 0) return true;
	const float4* dRays = (const float4*)rays; void* dOut = out; int32_t* dPrim = (kind == RAYLIB_AMD_QUERY_SURFACE) ? outPrim : nullptr;
	if (hostMem) {
		if (!Grow(R.qRays, R.qRaysBytes, (size_t)n * sizeof(RaylibAMDRay)) || !Grow(R.qOut, R.qOutBytes, outBytes)) return false;
		if (dPrim && !Grow(R.qPrim, R.qPrimBytes, (size_t)n * sizeof(int32_t))) return false;
		HIP_OK(hipMemcpyAsync(R.qRays, rays, (size_t)n * sizeof(RaylibAMDRay), hipMemcpyHostToDevice, st));
		dRays = R.qRays; dOut = R.qOut; if (dPrim) dPrim = R.qPrim;
	}
	const QueryKernel kernel = kind == RAYLIB_AMD_QUERY_ANY ? QueryKernelOfKind<RL_QK_ANY>(plan) : kind == RAYLIB_AMD_QUERY_CLOSEST ? QueryKernelOfKind<RL_QK_CLOSEST>(plan)
	                         : QueryKernelOfKind<RL_QK_SURFACE>(plan);
	const int blocksPerCU = OccupancyOf(R, (const void*)kernel);
	if (blocksPerCU < 0) return false;
	// enough workgroups to fill the device once; the waves take their rays from the counter (rl_k_query.inl)
	const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)R.numCUs * (uint64_t)std::max(1, blocksPerCU), ((uint64_t)n + RL_BLOCK - 1) / RL_BLOCK));
	const DSceneView view = Cp->view;
	HIP_OK(hipMemsetAsync(counter, 0, sizeof(unsigned int), st));
	if (sync) { HIP_OK(hipMemsetAsync(R.qStats, 0, 8 * sizeof(unsigned long long), st)); HIP_OK(hipEventRecord(R.qEv[0], st)); }
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RL_BLOCK), 0, st, view, dRays, (uint32_t)n, rayTime, dOut, dPrim, Cp->slotIndex, counter, sync ? R.qStats : nullptr);
	HIP_OK(hipGetLastError());
	HIP_OK(hipEventRecord(R.qRingEv[slot], st));
	R.qRingUsed[slot] = true;
	R.qRingNext = (slot + 1u) % RL_QUERY_RING;
	if (!sync) return true;
	HIP_OK(hipEventRecord(R.qEv[1], st));
	HIP_OK(hipMemcpyAsync(R.qStatsHost, R.qStats, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	if (hostMem) {
		HIP_OK(hipMemcpyAsync(out, dOut, outBytes, hipMemcpyDeviceToHost, st));
		if (dPrim) HIP_OK(hipMemcpyAsync(outPrim, dPrim, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	}
	HIP_OK(hipStreamSynchronize(st));
	float ms = 0.0f;
	HIP_OK(hipEventElapsedTime(&ms, R.qEv[0], R.qEv[1]));
	stats.rays = R.qStatsHost[CNT_RAYS]; stats.nodesVisited = R.qStatsHost[CNT_NODES]; stats.trisTested = R.qStatsHost[CNT_TRIS];
	stats.shadedHits = R.qStatsHost[CNT_SHADED]; stats.texFetches = R.qStatsHost[CNT_TEXELS];
	stats.kernelMs = ms; stats.traceKernelMs = ms; stats.traceLaunches = 1;
	stats.wallMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return true;
}

typedef void (*RadianceKernel)(const DSceneView, const SkyRot, const DRadianceParams, const float4*, uint32_t, float4*, float*, unsigned int*, unsigned long long*);
static RadianceKernel RadianceKernelFor(const QueryPlan& p)
{
	if (p.tree == TREE_GRID4) return p.stack <= 32 ? (RadianceKernel)k_radiance<4, 32, false> : (RadianceKernel)k_radiance<4, 64, false>;
	if (p.stack <= 32) return p.prims ? (RadianceKernel)k_radiance<2, 32, true> : (RadianceKernel)k_radiance<2, 32, false>;
	return p.prims ? (RadianceKernel)k_radiance<2, 64, true> : (RadianceKernel)k_radiance<2, 64, false>;
}
static_assert(sizeof(RaylibAMDPathRay) == 32, "radiance records");
static_assert(RL_RADIANCE_STACK_BUDGET / ((uint64_t)RL_RADIANCE_MAX_PATH * 8 * sizeof(float) * RL_BLOCK) >= 1, "one workgroup's path stack fits the budget");

bool DeviceTraceRadiance(Scene& sc, const RaylibAMDRadianceParams& prm, uint64_t seed, const void* rays, int32_t n, float* out, bool hostMem, void* stream,
                         RaylibAMDStats& stats)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	const QueryPlan plan = PlanRadiance(sc, ReadRenderKnobs());
	if (!plan.ok) { Log("RaylibAMD_TraceRadiance: BVH depth %u exceeds the traversal stack (64)", sc.bvh.depth); return false; }
	if (!hostMem && n > 0) {
		if (!OnDevice(rays, R.device) || !OnDevice(out, R.device)) { Log("RaylibAMD_TraceRadianceDevice: a pointer is not device memory of device %d", R.device); return false; }
		// the kernel reads a ray as two 16-byte loads and writes a result as one 16-byte store
		if (((uintptr_t)rays & 15u) != 0) { Log("RaylibAMD_TraceRadianceDevice: the rays are not 16-byte aligned"); return false; }
		if (((uintptr_t)out & 15u) != 0) { Log("RaylibAMD_TraceRadianceDevice: the output is not 16-byte aligned"); return false; }
	}
	if (!UploadScene(sc) || !SyncSky(sc)) return false;
	DeviceSceneCopy* Cp = sc.device->copy[(size_t)R.devSlot];
	if (!EnsureWideTree(Cp, sc, plan.tree)) return false;
	const hipStream_t st = stream ? (hipStream_t)stream : R.stream;
	const bool sync = !stream;
	if (!R.radCounter) HIP_OK(hipMalloc(&R.radCounter, sizeof(unsigned int)));
	if (!R.radEv) HIP_OK(hipEventCreateWithFlags(&R.radEv, hipEventDisableTiming));
	if (sync && !R.qStats) {
		HIP_OK(hipMalloc(&R.qStats, 8 * sizeof(unsigned long long)));
		HIP_OK(hipHostMalloc(&R.qStatsHost, 8 * sizeof(unsigned long long), hipHostMallocDefault));
		HIP_OK(hipEventCreate(&R.qEv[0])); HIP_OK(hipEventCreate(&R.qEv[1]));
	}
	memset(&stats, 0, sizeof(stats));
	stats.treeWidth = plan.treeWidth; stats.nodeBytes = plan.nodeBytes; stats.ranks = 1; stats.devices = 1;
	stats.numNodes = (uint32_t)sc.bvh.nodes.size(); stats.numTriangles = (uint32_t)sc.triangles.size(); stats.bvhDepth = sc.bvh.depth;
	if (n == 0) return true;
	const RadianceKernel kernel = RadianceKernelFor(plan);
	const int blocksPerCU = OccupancyOf(R, (const void*)kernel);
	if (blocksPerCU < 0) return false;
	// enough workgroups to fill the device once; the waves take their jobs from the counter (rl_k_radiance.inl)
	uint64_t blocks64 = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)R.numCUs * (uint64_t)std::max(1, blocksPerCU), ((uint64_t)n + RL_BLOCK - 1) / RL_BLOCK));
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
	if (!Grow(R.radStack, R.radStackBytes, depthSlots * 8 * Q.stackStride * sizeof(float))) return false;
	const float4* dRays = (const float4*)rays; float4* dOut = (float4*)out;
	const size_t outBytes = (size_t)n * sizeof(float4);
	if (hostMem) {
		if (!Grow(R.qRays, R.qRaysBytes, (size_t)n * sizeof(RaylibAMDPathRay)) || !Grow(R.qOut, R.qOutBytes, outBytes)) return false;
		HIP_OK(hipMemcpyAsync(R.qRays, rays, (size_t)n * sizeof(RaylibAMDPathRay), hipMemcpyHostToDevice, st));
		dRays = R.qRays; dOut = (float4*)R.qOut;
	}
	const DSceneView view = Cp->view;
	const SkyRot skyRot = sc.device->skyRot;
	if (R.radEvUsed) HIP_OK(hipStreamWaitEvent(st, R.radEv, 0));
	HIP_OK(hipMemsetAsync(R.radCounter, 0, sizeof(unsigned int), st));
	if (sync) { HIP_OK(hipMemsetAsync(R.qStats, 0, 8 * sizeof(unsigned long long), st)); HIP_OK(hipEventRecord(R.qEv[0], st)); }
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RL_BLOCK), 0, st, view, skyRot, Q, dRays, (uint32_t)n, dOut, R.radStack, R.radCounter, sync ? R.qStats : nullptr);
	HIP_OK(hipGetLastError());
	HIP_OK(hipEventRecord(R.radEv, st));
	R.radEvUsed = true;
	if (!sync) return true;
	HIP_OK(hipEventRecord(R.qEv[1], st));
	HIP_OK(hipMemcpyAsync(R.qStatsHost, R.qStats, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	if (hostMem) HIP_OK(hipMemcpyAsync(out, dOut, outBytes, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	float ms = 0.0f;
	HIP_OK(hipEventElapsedTime(&ms, R.qEv[0], R.qEv[1]));
	stats.rays = R.qStatsHost[CNT_RAYS]; stats.nodesVisited = R.qStatsHost[CNT_NODES]; stats.trisTested = R.qStatsHost[CNT_TRIS];
	stats.shadedHits = R.qStatsHost[CNT_SHADED]; stats.texFetches = R.qStatsHost[CNT_TEXELS]; stats.cameraSamples = R.qStatsHost[CNT_SAMPLES];
	stats.waveTrips = R.qStatsHost[CNT_TRIPS];
	stats.kernelMs = ms; stats.traceKernelMs = ms; stats.traceLaunches = 1;
	stats.wallMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return true;
}

// kind 0: scatter (in 16 / out 16 floats per record, a = material), 1: camera rays (in 2 / out 7), 2: texture (in 2 / out 4, a = texture, b = sRGB)
bool DeviceEvalHook(int kind, Scene* sc, const DCamera* cam, int a, int b, const float* in, int n, uint64_t seed, float* out)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (sc && !UploadScene(*sc)) return false;
	if (n <= 0) return true;
	const int inW = kind == 0 ? 16 : 2, outW = kind == 0 ? 16 : (kind == 1 ? 7 : 4);
	float *din = nullptr, *dout = nullptr;
	HIP_OK(hipMalloc(&din, (size_t)n * inW * 4));
	if (hipMalloc(&dout, (size_t)n * outW * 4) != hipSuccess) { (void)hipFree(din); return false; }
	bool ok = hipMemcpy(din, in, (size_t)n * inW * 4, hipMemcpyHostToDevice) == hipSuccess;
	if (ok) {
		const dim3 grid(((uint32_t)n + RL_BLOCK - 1) / RL_BLOCK), block(RL_BLOCK);
		if (kind == 0) hipLaunchKernelGGL(k_eval_scatter, grid, block, 0, R.stream, sc->device->copy[(size_t)R.devSlot]->view, a, din, n, (unsigned long long)seed, dout);
		else if (kind == 1) hipLaunchKernelGGL(k_eval_camera, grid, block, 0, R.stream, *cam, din, n, (unsigned long long)seed, dout);
		else hipLaunchKernelGGL(k_eval_texture, grid, block, 0, R.stream, sc->device->copy[(size_t)R.devSlot]->view, a, b, din, n, dout);
		ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(R.stream) == hipSuccess;
		ok = ok && hipMemcpy(out, dout, (size_t)n * outW * 4, hipMemcpyDeviceToHost) == hipSuccess;
	}
	(void)hipFree(din); (void)hipFree(dout);
	return ok;
}

bool DeviceEvalMath(int fn, const float* x, const float* y, int n, float* out)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (n <= 0) return true;
	float *dx = nullptr, *dy = nullptr, *dout = nullptr;
	bool ok = hipMalloc(&dx, (size_t)n * 4) == hipSuccess && hipMalloc(&dout, (size_t)n * 4) == hipSuccess;
	ok = ok && hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess;
	if (ok && y) ok = hipMalloc(&dy, (size_t)n * 4) == hipSuccess && hipMemcpy(dy, y, (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess;
	if (ok) {
		hipLaunchKernelGGL(k_eval_math, dim3(((uint32_t)n + RL_BLOCK - 1) / RL_BLOCK), dim3(RL_BLOCK), 0, R.stream, fn, dx, dy, n, dout);
		ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(R.stream) == hipSuccess;
		ok = ok && hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess;
	}
	if (dx) (void)hipFree(dx); if (dout) (void)hipFree(dout); if (dy) (void)hipFree(dy);
	return ok;
}

bool DeviceVerifyExactMath(int which, uint64_t* outMismatches, uint64_t* outFirst)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	unsigned long long* d = nullptr;
	HIP_OK(hipMalloc(&d, 2 * sizeof(unsigned long long)));
	unsigned long long h[2] = { 0ull, ~0ull };
	bool ok = hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) == hipSuccess;
	if (ok) {
		hipLaunchKernelGGL(k_verify_exact_math, dim3(4096), dim3(RL_BLOCK), 0, R.stream, which, d);
		ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(R.stream) == hipSuccess && hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess;
	}
	(void)hipFree(d);
	if (outMismatches) *outMismatches = h[0];
	if (outFirst) *outFirst = h[1];
	return ok;
}

// Images live on rank 0's device.
void* DeviceImagePixels(Image& img)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!EnsureRuntime()) return nullptr;
	const size_t need = (size_t)img.width * img.height * sizeof(float4);
	if (need == 0) return nullptr;
	if (img.devPixels && img.devBytes >= need) return img.devPixels;
	(void)DrainLocked();   // a frame in flight may be writing the buffer that is about to be freed
	if (hipSetDevice(Rank0().device) != hipSuccess) return nullptr;
	if (img.devPixels) { (void)hipFree(img.devPixels); img.devPixels = nullptr; img.devBytes = 0; }
	if (hipMalloc(&img.devPixels, need) != hipSuccess) { img.devPixels = nullptr; return nullptr; }
	img.devBytes = need;
	img.devValid = false;
	return img.devPixels;
}

bool DeviceReadback(Image& img)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	return ReadbackLocked(img);
}
namespace {
bool ReadbackLocked(Image& img)
{
	const size_t n = (size_t)img.width * img.height;
	if (n == 0) return true;
	if (!g_rt.ok || !img.devPixels || !img.devValid || img.devBytes < n * sizeof(float4)) return false;
	if (!DrainLocked()) Log("Image read-back: a frame in flight did not complete");
	HIP_OK(hipSetDevice(Rank0().device));
	img.rgba.resize(n * 4);
	HIP_OK(hipMemcpyAsync(img.rgba.data(), img.devPixels, n * sizeof(float4), hipMemcpyDeviceToHost, Rank0().stream));
	HIP_OK(hipStreamSynchronize(Rank0().stream));
	return true;
}
} // namespace

// Raylib_DumpImageData for a frame that lives on the device (reference raylib.h:90-93: the caller's buffer of 3 * 4 * w * h bytes; in the reference the pixels
// are in host memory when Raylib_Render returns, renderer.cc:292-296, so this copy is part of what a front-end sees of a render).  k_pack_rgb packs RGB on
// the device; the packed frame crosses the bus in chunks into PINNED staging memory (a pageable destination makes the runtime stage the copy through its own
// small buffers: 12 GB/s measured in round 3); helper threads copy every chunk on to the caller's memory as soon as its event has fired, so the host copies
// run beside the rest of the transfer.  img.rgba stays stale: another reader fetches its own copy (Image::SyncHost).
namespace {
struct DumpStage {
	float* packed = nullptr; size_t packedBytes = 0;     // device: RGB, 12 bytes per pixel
	float* pinned = nullptr; size_t pinnedBytes = 0;     // host, page-locked
	hipEvent_t ev[16] = {};
	bool evReady = false;
	std::vector<Worker*> helpers;
};
DumpStage g_dump;
}
bool DeviceDumpRGB(Image& img, float* outDest)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	const size_t n = (size_t)img.width * img.height;
	if (n == 0) return true;
	if (!g_rt.ok || !img.devPixels || !img.devValid || img.devBytes < n * sizeof(float4)) return false;
	if (const char* e = getenv("RAYLIB_FAST_DUMP")) if (atoi(e) == 0) return false;   // the plain path: read RGBA back, pack on the host
	if (!DrainLocked()) Log("Raylib_DumpImageData: a frame in flight did not complete");
	RankCtx& R = Rank0();
	DumpStage& D = g_dump;
	HIP_OK(hipSetDevice(R.device));
	const size_t bytes = n * 3 * sizeof(float);
	if (!Grow(D.packed, D.packedBytes, (bytes + 15) & ~(size_t)15)) return false;
	if (D.pinnedBytes < bytes) {
		if (D.pinned) { (void)hipHostFree(D.pinned); D.pinned = nullptr; D.pinnedBytes = 0; }
		HIP_OK(hipHostMalloc((void**)&D.pinned, bytes, hipHostMallocDefault));
		D.pinnedBytes = bytes;
	}
	if (!D.evReady) { for (hipEvent_t& e : D.ev) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); D.evReady = true; }
	const uint32_t blocks = (uint32_t)(((n + 3) / 4 + RL_BLOCK - 1) / RL_BLOCK);
	hipLaunchKernelGGL(k_pack_rgb, dim3(blocks), dim3(RL_BLOCK), 0, R.stream, (const float4*)img.devPixels, (float4*)D.packed, D.packed, n);
	HIP_OK(hipGetLastError());
	// chunks of ~2 MB (at most 16): the first host copy starts after 1/chunks of the transfer, the last one is all that is left when the transfer ends
	const size_t chunks = std::max<size_t>(1, std::min<size_t>(16, bytes / (2u << 20)));
	const size_t per = ((bytes / chunks) + 63) & ~(size_t)63;
	size_t nChunks = 0;
	for (size_t off = 0; off < bytes; off += per, ++nChunks) {
		const size_t len = std::min(per, bytes - off);
		HIP_OK(hipMemcpyAsync((char*)D.pinned + off, (const char*)D.packed + off, len, hipMemcpyDeviceToHost, R.stream));
		HIP_OK(hipEventRecord(D.ev[nChunks], R.stream));
	}
	// helper threads: chunk c is copied by helper c % (helpers + 1), the calling thread takes its share too
	const size_t wantHelpers = nChunks > 1 ? std::min<size_t>(3, std::max(1u, std::thread::hardware_concurrency()) - 1) : 0;
	while (D.helpers.size() < wantHelpers) { Worker* w = new Worker; w->Start(R.device); D.helpers.push_back(w); }
	const size_t lanes = wantHelpers + 1;
	auto copyLane = [&D, outDest, per, bytes, nChunks, lanes](size_t lane) -> bool {
		bool ok = true;
		for (size_t c = lane; c < nChunks; c += lanes) {
			if (hipEventSynchronize(D.ev[c]) != hipSuccess) { ok = false; break; }
			const size_t off = c * per;
			memcpy((char*)outDest + off, (const char*)D.pinned + off, std::min(per, bytes - off));
		}
		return ok;
	};
	for (size_t h = 0; h < wantHelpers; ++h) D.helpers[h]->Post([&copyLane, h]() { return copyLane(h + 1); });
	bool ok = copyLane(0);
	for (size_t h = 0; h < wantHelpers; ++h) ok = D.helpers[h]->Wait() && ok;
	if (!ok) { Log("Raylib_DumpImageData: the device copy failed"); (void)hipStreamSynchronize(R.stream); return false; }
	return true;
}

void DeviceFreePixels(void* p)
{
	if (!p) return;
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (g_rt.ok) { (void)DrainLocked(); (void)hipSetDevice(Rank0().device); (void)hipFree(p); }
}

// Image2D::PostProcess (reference render/image.cc:44-103) on the device: k_pp_max finds the white point
// (max is exact in any order), k_pp_map applies extended Reinhard on luminance, the clamp and gamma 1/2.2
// with glibc's exact powf.  Bit-identical to the host statement of the same function.
bool DevicePostProcess(Image& img)
{
	const size_t n = (size_t)img.width * img.height;
	if (n == 0) return true;
	float4* px = (float4*)DeviceImagePixels(img);
	if (!px) return false;
	std::lock_guard<std::mutex> lk(g_rt.lock);
	(void)DrainLocked();   // the frame this works on may still be in flight on the gather stream
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (!img.devValid) HIP_OK(hipMemcpyAsync(px, img.rgba.data(), n * sizeof(float4), hipMemcpyHostToDevice, R.stream));   // (never stale here: stale implies devValid)
	unsigned int one; { float f = 1.0f; memcpy(&one, &f, 4); }
	HIP_OK(hipMemcpyAsync(R.jobCounter, &one, sizeof(one), hipMemcpyHostToDevice, R.stream));
	const uint32_t blocks = (uint32_t)std::min<size_t>((n + RL_BLOCK - 1) / RL_BLOCK, 2048);
	hipLaunchKernelGGL(k_pp_max, dim3(blocks), dim3(RL_BLOCK), 0, R.stream, px, n, R.jobCounter);
	HIP_OK(hipGetLastError());
	hipLaunchKernelGGL(k_pp_map, dim3((uint32_t)((n + RL_BLOCK - 1) / RL_BLOCK)), dim3(RL_BLOCK), 0, R.stream, px, n, R.jobCounter);
	HIP_OK(hipGetLastError());
	float white = 1.0f;
	HIP_OK(hipMemcpyAsync(&white, R.jobCounter, 4, hipMemcpyDeviceToHost, R.stream));
	HIP_OK(hipStreamSynchronize(R.stream));
	img.devValid = true;
	img.hostStale = true;   // read back when the pixels are asked for (Image::SyncHost)
	img.Touch();
	Log("Max white luminance: %f", white);
	return true;
}

// ---- progressive sessions: rank 0's device and stream, whatever RAYLIB_NUM_GPUS says (a pass is one EnqueueRender of the whole frame) ----
namespace {
void FreeProgressive(ProgressiveSession* S)
{
	(void)hipFree(S->st.sum); (void)hipFree(S->st.s1); (void)hipFree(S->st.s2); (void)hipFree(S->st.cellSamples); (void)hipFree(S->st.stopped);
	(void)hipFree(S->live); (void)hipFree(S->trace); (void)hipFree(S->empty); (void)hipFree(S->counts);
	if (S->countsHost) (void)hipHostFree(S->countsHost);
	delete S;
}
bool AllocProgressive(ProgressiveSession& S)
{
	const size_t slots = (size_t)S.numCells * 64u, cells = S.numCells;
	HIP_OK(hipMalloc((void**)&S.st.sum, slots * sizeof(float4)));
	HIP_OK(hipMalloc((void**)&S.st.s1, slots * sizeof(float)));
	HIP_OK(hipMalloc((void**)&S.st.s2, slots * sizeof(float)));
	HIP_OK(hipMalloc((void**)&S.st.cellSamples, cells * sizeof(uint32_t)));
	HIP_OK(hipMalloc((void**)&S.st.stopped, cells));
	HIP_OK(hipMalloc((void**)&S.live, cells * sizeof(uint32_t)));
	HIP_OK(hipMalloc((void**)&S.trace, cells * sizeof(uint32_t)));
	HIP_OK(hipMalloc((void**)&S.empty, cells));
	HIP_OK(hipMalloc((void**)&S.counts, 4 * sizeof(uint32_t)));
	HIP_OK(hipHostMalloc((void**)&S.countsHost, 4 * sizeof(uint32_t), hipHostMallocDefault));
	HIP_OK(hipMemset(S.st.sum, 0, slots * sizeof(float4)));
	HIP_OK(hipMemset(S.st.s1, 0, slots * sizeof(float)));
	HIP_OK(hipMemset(S.st.s2, 0, slots * sizeof(float)));
	HIP_OK(hipMemset(S.st.cellSamples, 0, cells * sizeof(uint32_t)));
	HIP_OK(hipMemset(S.st.stopped, 0, cells));
	HIP_OK(hipMemset(S.empty, 0, cells));
	std::vector<uint32_t> all(cells);
	for (size_t c = 0; c < cells; ++c) all[c] = (uint32_t)c;
	HIP_OK(hipMemcpy(S.live, all.data(), cells * sizeof(uint32_t), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(S.trace, all.data(), cells * sizeof(uint32_t), hipMemcpyHostToDevice));
	return true;
}
} // namespace

ProgressiveSession* DeviceProgressiveBegin(Scene& sc, const RenderRequest& req, float threshold, uint32_t minSamples)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!EnsureRuntime()) return nullptr;
	if (hipSetDevice(Rank0().device) != hipSuccess) return nullptr;
	if (!UploadScene(sc) || !SyncSky(sc)) return nullptr;
	(void)DrainLocked();
	ProgressiveSession* S = new ProgressiveSession;
	S->scene = &sc; S->sceneSerial = sc.device->serial;
	S->sky = sc.sky; S->skyVersion = sc.sky ? sc.sky->version : 0;
	S->accelT0 = sc.accelT0; S->accelT1 = sc.accelT1;
	S->req = req; S->req.cellFirst = 0; S->req.cellStride = 1; S->req.cellMajor = false; S->req.slot = 0;
	S->req.outDevice = nullptr; S->req.outHostRGBA = nullptr; S->req.callerOwnsOut = false;
	S->width = req.settings.viewportWidth; S->height = req.settings.viewportHeight;
	S->numCells = ((S->width + 7) / 8) * ((S->height + 7) / 8);
	S->cap = (uint32_t)(req.settings.samplesPerPixel > 1 ? req.settings.samplesPerPixel : 1);
	S->st.threshold = threshold; S->st.minSamples = minSamples;
	S->numLive = S->numTrace = S->numCells;
	if (!AllocProgressive(*S)) { Log("RaylibAMD_BeginProgressive: the session's buffers could not be allocated"); FreeProgressive(S); return nullptr; }
	return S;
}

int32_t DeviceProgressiveStep(ProgressiveSession& S, uint32_t samples, void* outDevice, RaylibAMDStats& stats, bool& rendered)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	const auto t0 = std::chrono::steady_clock::now();
	rendered = false;
	if (!g_rt.ok) return -1;
	Scene& sc = *S.scene;
	// what the frame depends on must be what the session began on: anything else would make a mosaic of two scenes
	if (!sc.device || sc.device->serial != S.sceneSerial || sc.accelT0 != S.accelT0 || sc.accelT1 != S.accelT1) {
		Log("RaylibAMD_ProgressiveStep: the scene changed since the session began (finalized, sun or shutter); the image is unchanged");
		return -1;
	}
	if (sc.sky != S.sky || (sc.sky && sc.sky->version != S.skyVersion)) {
		Log("RaylibAMD_ProgressiveStep: the scene's sky panorama changed since the session began; the image is unchanged");
		return -1;
	}
	if (S.samples >= S.cap || S.numLive == 0) return 0;
	const uint32_t cnt = std::min(samples, S.cap - S.samples);
	(void)DrainLocked();
	g_deferredUnreported = false;   // (the numbers the caller reads next are this pass's)
	if (hipSetDevice(Rank0().device) != hipSuccess || !SyncSky(sc)) return -1;
	S.passEnd = S.samples + cnt;
	RenderRequest req = S.req;
	req.outDevice = outDevice;
	PendingRender pend;
	bool ok = EnqueueRender(Rank0(), sc, req, pend, &S);
	ok = FinishRender(Rank0(), pend, stats) && ok;
	if (!ok) return -1;
	rendered = true;
	S.samples += cnt; ++S.passes;
	S.numLive = S.countsHost[0]; S.numTrace = S.countsHost[1];
	S.emptyLivePixels = (uint64_t)S.countsHost[2] | ((uint64_t)S.countsHost[3] << 32);
	stats.ranks = 1; stats.devices = 1;
	stats.numNodes = (uint32_t)sc.bvh.nodes.size(); stats.numTriangles = (uint32_t)sc.triangles.size(); stats.bvhDepth = sc.bvh.depth;
	stats.wallMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return S.samples >= S.cap ? 0 : (int32_t)S.numLive;
}

// The session's per-cell samples and stop flags, and the moments of y per pixel in row-major order (the device keeps them cell-major).
bool DeviceProgressiveExport(ProgressiveSession& S, uint32_t* cellSamples, uint8_t* cellStopped, float* sumY, float* sumY2)
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!g_rt.ok) return false;
	HIP_OK(hipSetDevice(Rank0().device));
	if (cellSamples) HIP_OK(hipMemcpy(cellSamples, S.st.cellSamples, (size_t)S.numCells * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (cellStopped) HIP_OK(hipMemcpy(cellStopped, S.st.stopped, S.numCells, hipMemcpyDeviceToHost));
	const uint32_t cellsX = (S.width + 7) / 8;
	std::vector<float> slots((size_t)S.numCells * 64u);
	for (int m = 0; m < 2; ++m) {
		float* dst = m ? sumY2 : sumY;
		if (!dst) continue;
		HIP_OK(hipMemcpy(slots.data(), m ? S.st.s2 : S.st.s1, slots.size() * sizeof(float), hipMemcpyDeviceToHost));
		for (uint32_t y = 0; y < S.height; ++y)
			for (uint32_t x = 0; x < S.width; ++x) dst[(size_t)y * S.width + x] = slots[((size_t)(y / 8) * cellsX + x / 8) * 64u + (y % 8) * 8u + x % 8];
	}
	return true;
}

void DeviceProgressiveEnd(ProgressiveSession* S)
{
	if (!S) return;
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (g_rt.ok) (void)hipSetDevice(Rank0().device);
	FreeProgressive(S);
}

// Test hook: the lists of a session after a pass, from arrays of the caller's.  The launch is EnqueueFrame's (one workgroup of RL_COMPACT_BLOCK threads on rank 0's
// stream); the kernel writes live and trace in place, entries at indices <= their own, so numLive entries of each suffice.
bool DeviceProgressiveCompactTest(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const uint8_t* emptyOrNull, uint32_t numCells,
                                  uint32_t width, uint32_t height, uint32_t* outLive, uint32_t* outTrace, uint32_t outCounts[4])
{
	std::lock_guard<std::mutex> lk(g_rt.lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	// one allocation: live | trace | counts | stopped | empty, each from a multiple of 256 bytes
	const size_t listBytes = (((size_t)numLive * sizeof(uint32_t)) + 255) & ~(size_t)255, cellBytes = ((size_t)numCells + 255) & ~(size_t)255;
	char* d = nullptr;
	if (hipMalloc((void**)&d, 2 * listBytes + 256 + 2 * cellBytes) != hipSuccess) return false;
	uint32_t *dLive = (uint32_t*)d, *dTrace = (uint32_t*)(d + listBytes), *dCounts = (uint32_t*)(d + 2 * listBytes);
	uint8_t *dStopped = (uint8_t*)(d + 2 * listBytes + 256), *dEmpty = emptyOrNull ? dStopped + cellBytes : nullptr;
	uint32_t counts[4] = { 0, 0, 0, 0 };
	bool ok = numLive == 0 || hipMemcpy(dLive, live, (size_t)numLive * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
	ok = ok && hipMemcpy(dStopped, stopped, numCells, hipMemcpyHostToDevice) == hipSuccess;
	ok = ok && (!emptyOrNull || hipMemcpy(dEmpty, emptyOrNull, numCells, hipMemcpyHostToDevice) == hipSuccess);
	if (ok) {
		hipLaunchKernelGGL(k_progressive_compact, dim3(1), dim3(RL_COMPACT_BLOCK), 0, R.stream,
		                   dLive, dTrace, (const uint8_t*)dStopped, (const uint8_t*)dEmpty, numLive, width, height, (width + 7) / 8, dCounts);
		ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(R.stream) == hipSuccess;
		ok = ok && hipMemcpy(counts, dCounts, sizeof(counts), hipMemcpyDeviceToHost) == hipSuccess;
		ok = ok && counts[1] <= counts[0] && counts[0] <= numLive;   // (nothing is copied past the caller's arrays, whatever the kernel says)
		ok = ok && (counts[0] == 0 || hipMemcpy(outLive, dLive, (size_t)counts[0] * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess);
		ok = ok && (counts[1] == 0 || hipMemcpy(outTrace, dTrace, (size_t)counts[1] * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess);
		if (ok) memcpy(outCounts, counts, sizeof(counts));
	}
	(void)hipFree(d);
	return ok;
}

void DeviceReleaseScene(DeviceScene* D)
{
	if (!D) return;
	std::lock_guard<std::mutex> lk(g_rt.lock);
	(void)DrainLocked();   // frames in flight read this scene
	FreeScene(D);
}

} // namespace rl
