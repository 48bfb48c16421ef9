// Host runtime: whole frames over N ranks, DeviceRender, and progressive sessions -- what is built on a rank's EnqueueRender / FinishRender (rl_rt.h).
#include "rl_rt.h"

namespace rl {

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
	uint64_t serial = 0;                  // Runtime::statsSerial when the frame was enqueued
	bool ok = true, timed = false;
	std::chrono::steady_clock::time_point t0;
};

static bool FinishInflight(int slot)
{
	Runtime& R = Rt();
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
	F->stats.wallMs = MsSince(F->t0);
	// the last call's numbers, to be reported late -- unless a synchronous query, gather or bake has reported its own since the frame was enqueued
	// (they do not drain: RaylibAMD_GetLastStats is theirs then, and this frame's numbers go unreported as an overwritten frame's do)
	if (F->serial == R.statsSerial) { R.deferredStats = F->stats; R.deferredUnreported = true; }
	delete F;
	return ok;
}
// waits for every frame in flight (oldest first); the runtime lock is held by the caller
bool DrainLocked()
{
	Runtime& R = Rt();
	if (!R.ok) return true;
	const int older = (int)(R.frameNo & 1);   // the slot the NEXT frame would take holds the older of two frames in flight
	bool ok = FinishInflight(older);
	return FinishInflight(older ^ 1) && ok;
}

static bool RenderMulti(Scene& sc, const RenderRequest& req, RaylibAMDStats& stats, bool& deferred)
{
	Runtime& R = Rt();
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
	if (!R.gather[b].Grow(std::max<size_t>(16, (size_t)total * 64 * sizeof(float4)))) return false;
	float4* out = (float4*)req.outDevice;
	const size_t frameBytes = (size_t)W * H * sizeof(float4);
	if (!out) {
		if (frameBytes > R0.image.bytes) ok = FinishInflight(b ^ 1) && ok;   // the frame in flight may be writing the library's own image: not while it is re-allocated
		if (!R0.image.Grow(frameBytes)) return false;
		out = R0.image.ptr;
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
	F->serial = ++R.statsSerial;
	memset(&F->stats, 0, sizeof(F->stats));
	std::vector<PendingRender>& pend = F->pend;
	float4* gather = R.gather[b].ptr;
	auto run = [&](int r) -> bool {
		RankCtx& C = *R.ranks[(size_t)r];
		HIP_OK(hipSetDevice(C.device));
		RenderRequest q = req;
		q.cellFirst = (uint32_t)r; q.cellStride = (uint32_t)N; q.cellMajor = true; q.outHostRGBA = nullptr; q.slot = b;
		const size_t bytes = (size_t)local[(size_t)r] * 64 * sizeof(float4);
		float4* dst = gather + plan.offset[r];
		if (remote[(size_t)r]) { if (!C.cells.Grow(std::max<size_t>(16, bytes))) return false; q.outDevice = C.cells.ptr; }
		else q.outDevice = dst;   // same device as rank 0: rendered in place, nothing to move
		if (!EnqueueRender(C, sc, q, pend[(size_t)r])) return false;
		if (remote[(size_t)r] && !useRccl && bytes) HIP_OK(hipMemcpyPeerAsync(dst, R0.device, C.cells.ptr, C.device, bytes, C.stream));
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
			if (rc == 0) rc = A.Send(C.cells.ptr, floats, kRcclFloat, R0.devSlot, A.comms[(size_t)C.devSlot], sendStream(C));
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
	SceneStats(F->stats, sc);
	R.inflight[b] = F;
	++R.frameNo;
	if (!ok || !R.pipeline || req.outHostRGBA || req.callerOwnsOut) {
		// synchronous after all: a failure (every stream is drained whatever happened), the switch, pixels wanted in host memory now, or a frame
		// into device memory of the caller's (RaylibAMD_RenderDevice: "the library's stream has been synchronised when it returns" -- nothing the
		// library owns would keep a reader or a free of that buffer behind the gather stream's scatter)
		ok = DrainLocked() && ok;
		stats = R.deferredStats; R.deferredUnreported = false;
		return ok;
	}
	stats = F->stats;   // counters and times follow when the frame is waited for (RaylibAMD_GetLastStats, any reader of the pixels, the call after next)
	deferred = true;
	return ok;
}

bool DeviceRender(Scene& sc, const RenderRequest& req, RaylibAMDStats& stats)
{
	Runtime& RT = Rt();
	std::lock_guard<std::mutex> lk(RT.lock);
	const auto t0 = std::chrono::steady_clock::now();
	if (!EnsureRuntime()) return false;
	HIP_OK(hipSetDevice(Rank0().device));
	if (!UploadScene(sc)) return false;
	if (!SyncSky(sc)) return false;
	bool ok;
	const bool whole = req.cellFirst == 0 && (req.cellStride == 0 || req.cellStride == 1);
	if (whole && (RT.ranks.size() > 1 || RT.gatherSelf)) {
		bool deferred = false;
		ok = RenderMulti(sc, req, stats, deferred);
		if (deferred) return ok;    // scene numbers are in; counters, times and wallMs follow at the drain
	} else {
		(void)DrainLocked();        // this path uses rank 0's slot-0 events and counter block
		RT.deferredUnreported = false;   // ... and its numbers are the ones the caller reads next
		PendingRender pend;
		ok = EnqueueRender(Rank0(), sc, req, pend);
		if (ok && req.outHostRGBA) HIP_OK(hipMemcpyAsync(req.outHostRGBA, pend.out, pend.outBytes, hipMemcpyDeviceToHost, Rank0().stream));
		ok = FinishRender(Rank0(), pend, stats) && ok;
		stats.ranks = 1; stats.devices = 1;
	}
	SceneStats(stats, sc);
	if (!(whole && (RT.ranks.size() > 1 || RT.gatherSelf))) stats.wallMs = MsSince(t0);
	return ok;
}

// ---- progressive sessions: rank 0's device and stream, whatever RAYLIB_NUM_GPUS says (a pass is one EnqueueRender of the whole frame) ----
static bool AllocProgressive(ProgressiveSession& S)
{
	const size_t slots = (size_t)S.numCells * 64u, cells = S.numCells;
	if (!S.sum.Grow(slots * sizeof(float4)) || !S.s1.Grow(slots * sizeof(float)) || !S.s2.Grow(slots * sizeof(float))) return false;
	if (!S.cellSamples.Grow(cells * sizeof(uint32_t)) || !S.stopped.Grow(cells)) return false;
	if (!S.live.Grow(cells * sizeof(uint32_t)) || !S.trace.Grow(cells * sizeof(uint32_t)) || !S.empty.Grow(cells)) return false;
	if (!S.counts.Grow(4 * sizeof(uint32_t)) || !S.countsHost.Grow(4 * sizeof(uint32_t))) return false;
	S.st.sum = S.sum.ptr; S.st.s1 = S.s1.ptr; S.st.s2 = S.s2.ptr; S.st.cellSamples = S.cellSamples.ptr; S.st.stopped = S.stopped.ptr;
	HIP_OK(hipMemset(S.st.sum, 0, slots * sizeof(float4)));
	HIP_OK(hipMemset(S.st.s1, 0, slots * sizeof(float)));
	HIP_OK(hipMemset(S.st.s2, 0, slots * sizeof(float)));
	HIP_OK(hipMemset(S.st.cellSamples, 0, cells * sizeof(uint32_t)));
	HIP_OK(hipMemset(S.st.stopped, 0, cells));
	HIP_OK(hipMemset(S.empty.ptr, 0, cells));
	std::vector<uint32_t> all(cells);
	for (size_t c = 0; c < cells; ++c) all[c] = (uint32_t)c;
	HIP_OK(hipMemcpy(S.live.ptr, all.data(), cells * sizeof(uint32_t), hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(S.trace.ptr, all.data(), cells * sizeof(uint32_t), hipMemcpyHostToDevice));
	return true;
}

ProgressiveSession* DeviceProgressiveBegin(Scene& sc, const RenderRequest& req, float threshold, uint32_t minSamples)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
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
	if (!AllocProgressive(*S)) { Log("RaylibAMD_BeginProgressive: the session's buffers could not be allocated"); delete S; return nullptr; }
	return S;
}

int32_t DeviceProgressiveStep(ProgressiveSession& S, uint32_t samples, void* outDevice, RaylibAMDStats& stats, bool& rendered)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	const auto t0 = std::chrono::steady_clock::now();
	rendered = false;
	if (!Rt().ok) return -1;
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
	Rt().deferredUnreported = false;   // (the numbers the caller reads next are this pass's)
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
	S.numLive = S.countsHost.ptr[0]; S.numTrace = S.countsHost.ptr[1];
	S.emptyLivePixels = (uint64_t)S.countsHost.ptr[2] | ((uint64_t)S.countsHost.ptr[3] << 32);
	OneRankStats(stats, sc);
	stats.wallMs = MsSince(t0);
	return S.samples >= S.cap ? 0 : (int32_t)S.numLive;
}

// The session's per-cell samples and stop flags, and the moments of y per pixel in row-major order (the device keeps them cell-major).
bool DeviceProgressiveExport(ProgressiveSession& S, uint32_t* cellSamples, uint8_t* cellStopped, float* sumY, float* sumY2)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!Rt().ok) return false;
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
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (Rt().ok) (void)hipSetDevice(Rank0().device);
	delete S;   // (its buffers go with it, on rank 0's device)
}

} // namespace rl
