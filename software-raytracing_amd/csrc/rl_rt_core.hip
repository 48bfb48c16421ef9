// Host runtime: the one Runtime of the process, the device probe, the RCCL binding, and what a front-end asks about them (rl_rt.h).
#include "rl_rt.h"

#include <dlfcn.h>

namespace rl {

Runtime& Rt()
{
	static Runtime* const rt = new Runtime;
	return *rt;
}

bool EnsureRuntime()
{
	Runtime& R = Rt();
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
			if (!C->cntHost[q].Grow((CNT_COUNT + 24 + 2) * sizeof(unsigned long long))) return false;   // (+ the RL_CNT_LIT pair)
		}
		if (!C->counters.Grow(RL_CNT_BLOCK * sizeof(unsigned long long))) return false;
		if (!C->jobCounter.Grow(RL_MAX_HEADS * RL_HEAD_STRIDE * sizeof(unsigned int))) return false;   // the heads of the job list, one per XCD, 128 B apart
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
	Runtime& R = Rt();
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

// workgroups of `kernel` a CU holds, asked once per kernel and rank; -1: the query failed (logged).  RAYLIB_PRINT_OCCUPANCY: a megakernel's first answer is logged.
int OccupancyOf(RankCtx& R, const void* kernel, const TracePlan* megakernel)
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

bool DeviceAvailable()
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	return EnsureRuntime();
}

int DeviceNumRanks()
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	return EnsureRuntime() ? (int)Rt().ranks.size() : 0;
}

// Waits for whatever Raylib_Render left in flight.  True with `out` filled when that completed the LAST render call's numbers (counters, times)
// that the call itself could not report yet.
bool DeviceDrain(RaylibAMDStats* out)
{
	Runtime& R = Rt();
	std::lock_guard<std::mutex> lk(R.lock);
	if (!R.ok) return false;
	(void)DrainLocked();
	if (!R.deferredUnreported) return false;
	R.deferredUnreported = false;
	if (out) *out = R.deferredStats;
	return true;
}

// A synchronous call on rank 0's stream that does not drain (the ray queries, radiance, gathers, lightmap bakes) has returned its own numbers, which the caller
// stores as the last call's: a frame still in flight behind it is no longer the last call (FinishInflight compares the serial), and neither is one that a drain
// inside the call (SyncSky) completed.
void DeviceOwnStats()
{
	Runtime& R = Rt();
	std::lock_guard<std::mutex> lk(R.lock);
	++R.statsSerial;
	R.deferredUnreported = false;
}

} // namespace rl
