// Host runtime: a finalized scene's triangles moved (RaylibAMD_SceneMoveTriangles / ...Device, include/raylib_amd.h) -- the moved records and the refit of every
// tree the device holds (rl_refit.hip's kernels), the status a move leaves behind, the read-back that brings the host's copies up to date, and the two test
// hooks: the builder's validity checks on what the device holds, and the device's wide formats against the host's rule on the device's binary boxes (rl_rt.h).
//
// Schedule of a move on stream st: k_move_scan, k_move_records; k_refit_level once per level of the binary tree, deepest first, each launch reading what the one
// before wrote; then k_refit_wide4 / k_refit_wide8 for the wide formats that are on the device; the status block and the root node to pinned memory; the event.
// The binary tree's own array is the one set of exact float boxes all formats are re-derived from: a wide record's child came from one of its child boxes, and
// the builder recorded which (BVH::boxOf*).
// The next call on the scene waits for the event (SettleMove: UploadScene, which opens every device call) and takes from the status what the host keeps of a scene:
// the fastBary flag of the views and the root's boxes, from which the silhouette cull takes the scene's bounds (rl_plan.cc SceneCullScene).
#include "rl_rt.h"

namespace rl {

using Move = DeviceSceneCopy::Move;
static uint32_t BlocksFor(uint64_t n) { return (uint32_t)((n + RL_BLOCK - 1) / RL_BLOCK); }
constexpr size_t kStatusHostWords = RL_MOVE_WORDS + sizeof(DNode) / sizeof(uint32_t);

// the tables of a copy's first move, made with the copy's device current; the host's trees are current (no move has happened)
static bool EnsureMoveTables(DeviceSceneCopy* C, const Scene& sc, hipStream_t st)
{
	if (C->move) return true;
	const BVH& B = sc.bvh;
	const size_t n = sc.triangles.size(), nn = B.nodes.size();
	std::vector<int32_t> slotOf(n, -1);
	if (B.triOrder.size() != n) { Log("RaylibAMD_SceneMoveTriangles: the scene's leaf order does not list its triangles"); return false; }
	for (size_t k = 0; k < n; ++k) { if (B.triOrder[k] >= n) return false; slotOf[B.triOrder[k]] = (int32_t)k; }
	// levels: children follow their parent in `nodes` (rl_bvh.cc EmitBinary numbers them in pre-order), so one forward sweep sees a parent first
	std::vector<uint32_t> depth(nn, 0u); uint32_t levels = 1;
	for (size_t i = 0; i < nn; ++i) for (const int32_t ref : { B.nodes[i].left, B.nodes[i].right }) {
		if (ref < 0) continue;
		if ((size_t)ref <= i || (size_t)ref >= nn) { Log("RaylibAMD_SceneMoveTriangles: the binary tree is not in pre-order"); return false; }
		depth[(size_t)ref] = depth[i] + 1u; levels = std::max(levels, depth[(size_t)ref] + 1u);
	}
	std::unique_ptr<Move> M(new Move);
	M->levelStart.assign((size_t)levels + 1, 0u);
	for (size_t i = 0; i < nn; ++i) M->levelStart[depth[i] + 1u]++;
	for (uint32_t d = 0; d < levels; ++d) M->levelStart[d + 1u] += M->levelStart[d];
	std::vector<uint32_t> levelNodes(nn), at(M->levelStart.begin(), M->levelStart.end() - 1);
	for (size_t i = 0; i < nn; ++i) levelNodes[at[depth[i]]++] = (uint32_t)i;
	if (!M->slotOf.Upload(slotOf.data(), n) || !M->levelNodes.Upload(levelNodes.data(), nn) || !M->boxOf4.Upload(B.boxOf4.data(), B.boxOf4.size())
	    || !M->boxOf8.Upload(B.boxOf8.data(), B.boxOf8.size()) || !M->boxOfLeafList.Upload(B.boxOfLeafList.data(), B.boxOfLeafList.size())
	    || !M->status.Grow(RL_MOVE_WORDS * sizeof(uint32_t)) || !M->statusHost.Grow(kStatusHostWords * sizeof(uint32_t))) return false;
	HIP_OK(hipEventCreateWithFlags(&M->ev, hipEventDisableTiming));
	HIP_OK(hipEventCreateWithFlags(&M->inEv, hipEventDisableTiming)); HIP_OK(hipEventCreateWithFlags(&M->copiedEv, hipEventDisableTiming));
	if (const char* e = getenv("RAYLIB_FAST_BARY")) M->fastBaryBase = atoi(e) != 0 ? 1 : 0;   // (as rl_scene.cc FlattenScene reads it)
	HIP_OK(hipMemsetAsync(M->status.ptr, 0, RL_MOVE_WORDS * sizeof(uint32_t), st));
	hipLaunchKernelGGL(k_move_count, dim3(BlocksFor(n)), dim3(RL_BLOCK), 0, st, (const DTriIsect*)C->isect.ptr, (uint32_t)n, M->status.ptr);
	HIP_OK(hipGetLastError());
	C->move = M.release();
	return true;
}

// A move in flight is complete on every copy, and what the host keeps of the scene agrees with it.  The runtime lock is held; the scene is on the device.
// The status (the same on every copy: the same kernels on the same values) is read from rank 0's.
bool SettleMove(Scene& sc)
{
	const size_t slot0 = (size_t)Rank0().devSlot;
	for (size_t slot = 0; slot < sc.device->copy.size(); ++slot) {
		DeviceSceneCopy* C = sc.device->copy[slot];
		Move* M = C->move;
		if (!M || !M->pending) continue;
		HIP_OK(hipEventSynchronize(M->ev));
		M->pending = false;
		const uint32_t* S = M->statusHost.ptr;
		C->view.fastBary = (M->fastBaryBase && S[RL_MOVE_BAD_DENOM] == 0u) ? 1 : 0;
		if (slot != slot0) continue;
		if (S[RL_MOVE_NONFINITE]) Log("RaylibAMD_SceneMoveTrianglesDevice: a position or normal of the last move was not finite; that move was NOT applied");
		if (!sc.bvh.nodes.empty()) memcpy(&sc.bvh.nodes[0], S + RL_MOVE_WORDS, sizeof(DNode));   // the root's two boxes: the cull's bounds
	}
	return true;
}

// positions / normals: device memory, ready on st.  Everything is enqueued on st; nothing is waited for.
static bool EnqueueMove(DeviceSceneCopy* C, const Scene& sc, uint32_t first, uint32_t count, const float* positions, const float* normals, hipStream_t st)
{
	Move& M = *C->move;
	const uint32_t numTris = (uint32_t)sc.triangles.size(), numNodes = (uint32_t)sc.bvh.nodes.size();
	HIP_OK(hipMemsetAsync(M.status.ptr + RL_MOVE_NONFINITE, 0, sizeof(uint32_t), st));
	hipLaunchKernelGGL(k_move_scan, dim3(BlocksFor((uint64_t)count * 9)), dim3(RL_BLOCK), 0, st, positions, normals, count * 9u, M.status.ptr);
	HIP_OK(hipGetLastError());
	hipLaunchKernelGGL(k_move_records, dim3(BlocksFor(count)), dim3(RL_BLOCK), 0, st, C->isect.ptr, C->shade.ptr, (const int32_t*)M.slotOf.ptr, first, count, numTris,
	                   positions, normals, M.status.ptr);
	HIP_OK(hipGetLastError());
	for (size_t d = M.levelStart.size() - 1; d-- > 0;) {
		const uint32_t b = M.levelStart[d], n = M.levelStart[d + 1] - b;
		if (!n) continue;
		hipLaunchKernelGGL(k_refit_level, dim3(BlocksFor(n)), dim3(RL_BLOCK), 0, st, C->nodes.ptr, (const DTriIsect*)C->isect.ptr, (const uint32_t*)M.levelNodes.ptr + b, n, numNodes, numTris);
		HIP_OK(hipGetLastError());
	}
	const uint32_t n4 = (uint32_t)sc.bvh.nodes4.size(), n8 = (uint32_t)sc.bvh.nodes8.size(), nL = (uint32_t)sc.bvh.leafList.size();
	if (n4 && (C->nodes4f.ptr || C->nodes4.ptr)) {
		hipLaunchKernelGGL(k_refit_wide4, dim3(BlocksFor(n4)), dim3(RL_BLOCK), 0, st, (const DNode*)C->nodes.ptr, numNodes, (const int32_t*)M.boxOf4.ptr, C->nodes4f.ptr, C->nodes4.ptr, n4);
		HIP_OK(hipGetLastError());
	}
	if (nL && C->leafList.ptr) {
		hipLaunchKernelGGL(k_refit_wide4, dim3(BlocksFor(nL)), dim3(RL_BLOCK), 0, st, (const DNode*)C->nodes.ptr, numNodes, (const int32_t*)M.boxOfLeafList.ptr, C->leafList.ptr, (DNode4Q*)nullptr, nL);
		HIP_OK(hipGetLastError());
	}
	if (n8 && C->nodes8.ptr) {
		hipLaunchKernelGGL(k_refit_wide8, dim3(BlocksFor(n8)), dim3(RL_BLOCK), 0, st, (const DNode*)C->nodes.ptr, numNodes, (const int32_t*)M.boxOf8.ptr, C->nodes8.ptr, n8);
		HIP_OK(hipGetLastError());
	}
	HIP_OK(hipMemcpyAsync(M.statusHost.ptr, M.status.ptr, RL_MOVE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	HIP_OK(hipMemcpyAsync(M.statusHost.ptr + RL_MOVE_WORDS, C->nodes.ptr, sizeof(DNode), hipMemcpyDeviceToHost, st));
	HIP_OK(hipEventRecord(M.ev, st));
	M.pending = true;
	return true;
}

// the stream a copy's move runs on: rank 0's copy on the call's stream, another device's copy on the stream of the first rank that renders on it
static hipStream_t CopyStream(size_t slot, hipStream_t st)
{
	if (slot == (size_t)Rank0().devSlot) return st;
	for (RankCtx* R : Rt().ranks) if ((size_t)R->devSlot == slot) return R->stream;
	return nullptr;
}

bool DeviceMoveTriangles(Scene& sc, int32_t first, int32_t count, const float* positions, const float* normals, bool hostMem, void* stream)
{
	const char* who = hostMem ? "RaylibAMD_SceneMoveTriangles" : "RaylibAMD_SceneMoveTrianglesDevice";
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (!hostMem) {
		if (!OnDevice(positions, R.device) || (normals && !OnDevice(normals, R.device))) { Log("%s: a pointer is not device memory of device %d", who, R.device); return false; }
		if (((uintptr_t)positions & 3u) != 0 || ((uintptr_t)normals & 3u) != 0) { Log("%s: the values are not 4-byte aligned", who); return false; }
	}
	if (!UploadScene(sc)) return false;   // (settles a move in flight)
	(void)DrainLocked();                  // a multi-rank frame in flight reads the records and trees that are about to change
	const hipStream_t st = stream ? (hipStream_t)stream : R.stream;
	// the library's work in flight on other streams of the caller's reads the scene too: the move goes behind the ray queries' ring and the path calls' chain
	// (both run on rank 0's device alone)
	for (int k = 0; k < RL_QUERY_RING; ++k) if (R.qRingUsed[k]) HIP_OK(hipStreamWaitEvent(st, R.qRingEv[k], 0));
	if (R.radEvUsed) HIP_OK(hipStreamWaitEvent(st, R.radEv, 0));
	const size_t floats = (size_t)count * 9, slot0 = (size_t)R.devSlot;
	bool ok = true;
	// Every device's copy is moved, rank 0's first: the same kernels on the same values, each on a stream of its own device.  A host call's values are
	// uploaded to each device; a device call's live on rank 0's device, and a copy on another device takes them by a peer copy into its staging buffer, behind an
	// event on the call's stream (the values are ready there) -- and the call's stream waits for those copies, so that the caller may overwrite the values behind the call.
	for (size_t k = 0; k < sc.device->copy.size() && ok; ++k) {
		const size_t slot = k == 0 ? slot0 : (k <= slot0 ? k - 1 : k);
		DeviceSceneCopy* C = sc.device->copy[slot];
		const hipStream_t cs = CopyStream(slot, st);
		if (!cs) { Log("%s: no rank renders on device %d", who, C->device); ok = false; break; }
		HIP_TRY(hipSetDevice(C->device));
		if (!ok || !EnsureMoveTables(C, sc, cs)) { ok = false; break; }
		Move& M = *C->move;
		const float* dPos = positions; const float* dNrm = normals;
		if (hostMem || slot != slot0) {
			if (!M.staging.Grow(2 * floats * sizeof(float))) { ok = false; break; }
			dPos = M.staging.ptr; dNrm = normals ? M.staging.ptr + floats : nullptr;
			if (hostMem) {
				HIP_TRY(hipMemcpyAsync(M.staging.ptr, positions, floats * sizeof(float), hipMemcpyHostToDevice, cs));
				if (normals) HIP_TRY(hipMemcpyAsync(M.staging.ptr + floats, normals, floats * sizeof(float), hipMemcpyHostToDevice, cs));
			} else {
				Move& M0 = *sc.device->copy[slot0]->move;   // (rank 0's copy came first: its events exist)
				HIP_TRY(hipStreamWaitEvent(cs, M0.inEv, 0));
				HIP_TRY(hipMemcpyPeerAsync(M.staging.ptr, C->device, positions, R.device, floats * sizeof(float), cs));
				if (normals) HIP_TRY(hipMemcpyPeerAsync(M.staging.ptr + floats, C->device, normals, R.device, floats * sizeof(float), cs));
				HIP_TRY(hipEventRecord(M.copiedEv, cs));
				HIP_TRY(hipStreamWaitEvent(st, M.copiedEv, 0));
			}
		} else if (sc.device->copy.size() > 1) HIP_TRY(hipEventRecord(M.inEv, st));   // rank 0's copy of a device call: the values are ready on st from here on
		ok = ok && EnqueueMove(C, sc, (uint32_t)first, (uint32_t)count, dPos, dNrm, cs);
		C->lmTrisStale = true;
	}
	(void)hipSetDevice(R.device);
	sc.hostTreesStale = true;
	if (!ok) {   // what was enqueued completes; the scene's copies may disagree from here on, and the host's copies are read back from rank 0's
		for (DeviceSceneCopy* C : sc.device->copy) if (C->move && C->move->pending) (void)hipEventSynchronize(C->move->ev);
		(void)hipStreamSynchronize(st);
		sc.hostTrisStale = true;
		Log("%s: the move could not be enqueued on every device", who);
		return false;
	}
	if (hostMem) {
		// the host's triangles follow at once (the ABI found every value finite); where an earlier device move left them behind, the read-back brings both
		if (!sc.hostTrisStale) for (int32_t k = 0; k < count; ++k) {
			HostTriangle& t = sc.triangles[(size_t)first + (size_t)k];
			memcpy(&t.v0, positions + (size_t)k * 9, 9 * sizeof(float));
			if (normals) memcpy(&t.n0, normals + (size_t)k * 9, 9 * sizeof(float));
		}
	} else sc.hostTrisStale = true;
	if (stream) return true;
	if (!SettleMove(sc)) return false;
	return sc.device->copy[slot0]->move->statusHost.ptr[RL_MOVE_NONFINITE] == 0u;
}

// The host's copies of a moved scene: the triangles' positions and shading normals from the device's records, bvh.nodes from the device's, the wide formats and
// the SAH cost from those (rl_bvh.cc RefitWideFromBinary: the device's rule, so the host's wide trees are the device's).
bool SyncMovedLocked(Scene& sc)
{
	if (!sc.hostTrisStale && !sc.hostTreesStale) return true;
	if (!sc.device || !SettleMove(sc)) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	DeviceSceneCopy* C = sc.device->copy[(size_t)R.devSlot];
	const size_t n = sc.triangles.size();
	if (sc.hostTrisStale) {
		std::vector<DTriIsect> isect(n); std::vector<DTriShade> shade(n);
		HIP_OK(hipMemcpy(isect.data(), C->isect.ptr, n * sizeof(DTriIsect), hipMemcpyDeviceToHost));
		HIP_OK(hipMemcpy(shade.data(), C->shade.ptr, n * sizeof(DTriShade), hipMemcpyDeviceToHost));
		for (size_t k = 0; k < n; ++k) {
			HostTriangle& t = sc.triangles[sc.bvh.triOrder[k]];
			memcpy(&t.v0, isect[k].v0, 12); memcpy(&t.v1, isect[k].v1, 12); memcpy(&t.v2, isect[k].v2, 12);
			memcpy(&t.n0, shade[k].n0, 36);
		}
		sc.hostTrisStale = false;
	}
	if (sc.hostTreesStale) {
		HIP_OK(hipMemcpy(sc.bvh.nodes.data(), C->nodes.ptr, sc.bvh.nodes.size() * sizeof(DNode), hipMemcpyDeviceToHost));
		RefitWideFromBinary(sc.bvh);
		sc.hostTreesStale = false;
	}
	return true;
}
bool DeviceSyncMovedScene(Scene& sc)
{
	if (!sc.device) return true;   // never uploaded, or released: the host's copies are the scene
	std::lock_guard<std::mutex> lk(Rt().lock);
	return SyncMovedLocked(sc);
}

// rl_bvh.cc's checks on the trees and records as the device holds them: a copy of the host's topology with every array the device has read back over it
bool DeviceCheckTrees(Scene& sc, uint32_t* outFailedTree)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (!UploadScene(sc) || !SyncMovedLocked(sc)) return false;
	uint32_t failed = 0;
	for (DeviceSceneCopy* C : sc.device->copy) {   // every device's copy
		HIP_OK(hipSetDevice(C->device));
		BVH B = sc.bvh;
		std::vector<HostTriangle> tris = sc.triangles;
		const size_t n = tris.size();
		std::vector<DTriIsect> isect(n);
		if (n) HIP_OK(hipMemcpy(isect.data(), C->isect.ptr, n * sizeof(DTriIsect), hipMemcpyDeviceToHost));
		for (size_t k = 0; k < n; ++k) { HostTriangle& t = tris[B.triOrder[k]]; memcpy(&t.v0, isect[k].v0, 12); memcpy(&t.v1, isect[k].v1, 12); memcpy(&t.v2, isect[k].v2, 12); }
		HIP_OK(hipMemcpy(B.nodes.data(), C->nodes.ptr, B.nodes.size() * sizeof(DNode), hipMemcpyDeviceToHost));
		if (C->nodes4f.ptr) HIP_OK(hipMemcpy(B.nodes4.data(), C->nodes4f.ptr, B.nodes4.size() * sizeof(DNode4), hipMemcpyDeviceToHost));
		if (C->nodes4.ptr) HIP_OK(hipMemcpy(B.nodes4q.data(), C->nodes4.ptr, B.nodes4q.size() * sizeof(DNode4Q), hipMemcpyDeviceToHost));
		if (C->nodes8.ptr) HIP_OK(hipMemcpy(B.nodes8.data(), C->nodes8.ptr, B.nodes8.size() * sizeof(DNode8), hipMemcpyDeviceToHost));
		if (C->leafList.ptr) HIP_OK(hipMemcpy(B.leafList.data(), C->leafList.ptr, B.leafList.size() * sizeof(DNode4), hipMemcpyDeviceToHost));
		if (memcmp(tris.data(), sc.triangles.data(), n * sizeof(HostTriangle)) != 0 || !ValidateBVH(B, tris)) failed = 2;   // (the host's triangles are current: every copy holds them)
		else if (!B.nodes4.empty() && !ValidateBVH4(B, tris)) failed = 4;
		else if (!ValidateBVH8(B, tris)) failed = 8;
		if (failed) break;
	}
	HIP_OK(hipSetDevice(R.device));
	if (outFailedTree) *outFailedTree = failed;
	return failed == 0;
}

// whether n records on the device are, byte for byte, the host's; false: the read-back failed
template <typename T> static bool SameOnDevice(const T* dev, const T* host, size_t n, bool& same)
{
	std::vector<T> got(n);
	if (n) HIP_OK(hipMemcpy(got.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost));
	same = n == 0 || memcmp(got.data(), host, n * sizeof(T)) == 0;
	return true;
}

// The wide formats as the device holds them against the host's rule on the device's own binary boxes: per copy, its binary nodes read back into a copy of the
// host's BVH (whose topology a move keeps; a stale box of it is overwritten or, under an unused child, the builder's on both sides), RefitWideFromBinary on that
// copy, and the bytes of every wide array the copy holds beside it.  The host's copies and their staleness flags are neither read for their boxes nor touched.
bool DeviceCompareTrees(Scene& sc, uint32_t* outDiffMask)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (!UploadScene(sc)) return false;   // (settles a move in flight)
	uint32_t diff = 0;
	const size_t n = sc.triangles.size();
	std::vector<DTriIsect> isect0(n);
	if (n) HIP_OK(hipMemcpy(isect0.data(), sc.device->copy[(size_t)R.devSlot]->isect.ptr, n * sizeof(DTriIsect), hipMemcpyDeviceToHost));
	for (DeviceSceneCopy* C : sc.device->copy) {   // every device's copy
		HIP_OK(hipSetDevice(C->device));
		BVH B = sc.bvh;
		HIP_OK(hipMemcpy(B.nodes.data(), C->nodes.ptr, B.nodes.size() * sizeof(DNode), hipMemcpyDeviceToHost));
		RefitWideFromBinary(B);
		bool same = true;
		if (C->nodes4f.ptr) { if (!SameOnDevice(C->nodes4f.ptr, B.nodes4.data(), B.nodes4.size(), same)) return false; if (!same) diff |= 1u; }
		if (C->nodes4.ptr) { if (!SameOnDevice(C->nodes4.ptr, B.nodes4q.data(), B.nodes4q.size(), same)) return false; if (!same) diff |= 2u; }
		if (C->leafList.ptr) { if (!SameOnDevice(C->leafList.ptr, B.leafList.data(), B.leafList.size(), same)) return false; if (!same) diff |= 4u; }
		if (C->nodes8.ptr) { if (!SameOnDevice(C->nodes8.ptr, B.nodes8.data(), B.nodes8.size(), same)) return false; if (!same) diff |= 8u; }
		if (!SameOnDevice(C->isect.ptr, isect0.data(), n, same)) return false;
		if (!same) diff |= 16u;
	}
	HIP_OK(hipSetDevice(R.device));
	if (outDiffMask) *outDiffMask = diff;
	return diff == 0;
}

} // namespace rl
