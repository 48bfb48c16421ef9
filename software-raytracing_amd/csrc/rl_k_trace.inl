// k_trace, the megakernel of one path per lane, and its views twin (RaylibAMD_RenderViews), one source for both: a translation unit includes this file with RL_VIEWS_TWIN 0 for the
// one-view kernel (rl_render.hip) or 1 for the twin (rl_render_views.hip); prototypes and default template arguments: rl_kernels.h.  The twin takes the view table (DViews) as one more
// trailing argument; everything under RL_VIEWS_TWIN is the twin's alone, so that the
// one-view kernel is the token sequence it always was (a template flag would add an inlining level, which reorders the one-view kernel's code:
// tools/isa_equivalence.py).
// RL_LAZY_REFL 1 (rl_render_lazy.hip): k_trace_lazy, the leaf-list kernel's PLAIN instance with the reflectance evaluated on lit paths only
// (rl_dev_shade.h "lazy-reflectance instance"); it takes the lit list (DLitList) as one more trailing argument.  Everything under RL_LAZY_REFL is that instance's alone.
#ifndef RL_LAZY_REFL
#define RL_LAZY_REFL 0
#endif

template <int STACK, bool PRIMS, bool FULL, int LDS, bool PLAIN>
__global__ void __launch_bounds__(RL_BLOCK, (STACK <= 32 ? RL_TRACE_MIN_WAVES : 2))
#if RL_VIEWS_TWIN
k_trace_views(const DRenderParams Pk, const DSceneView Sk, const SkyRot Rk, SampleRGB* __restrict__ samplesK,
              float* __restrict__ pathStackK, unsigned long long* __restrict__ countersK, unsigned int* __restrict__ jobCounterK, const DViews Vk)
#elif RL_LAZY_REFL
k_trace_lazy(const DRenderParams Pk, const DSceneView Sk, const SkyRot Rk, SampleRGB* __restrict__ samplesK,
             float* __restrict__ pathStackK, unsigned long long* __restrict__ countersK, unsigned int* __restrict__ jobCounterK, const DLitList LLk)
#else
k_trace(const DRenderParams Pk, const DSceneView Sk, const SkyRot Rk, SampleRGB* __restrict__ samplesK,
        float* __restrict__ pathStackK, unsigned long long* __restrict__ countersK, unsigned int* __restrict__ jobCounterK)
#endif
{
#if RL_LAZY_REFL
	static_assert(LDS == 2 && PLAIN && !PRIMS, "the lazy instance is the leaf-list kernel's PLAIN instance");
	(void)LLk;
#endif
	(void)Pk; (void)Sk; (void)Rk; (void)samplesK; (void)pathStackK; (void)countersK; (void)jobCounterK;
	RL_TEX_PROLOGUE(Sk);
	RL_MATH_PROLOGUE();
	__shared__ int s_stack[STACK * RL_BLOCK];
	__shared__ float4 s_scene[LDS ? LdsAt<LDS>::TOTAL : 1];
	const float4* sm = s_scene;
#if RL_QUEUE_SHARED_CHUNK
	// LDS == 2: the workgroup's four waves draw their batches of 64 jobs from ONE chunk (low word: next job, high word: end of the chunk)
	__shared__ unsigned long long s_jobs;
	__shared__ unsigned int s_lock, s_done;
	if (LDS == 2 && threadIdx.x == 0) { s_jobs = 0ull; s_lock = 0u; s_done = 0u; }   // empty: the first wave to ask draws the workgroup's first chunk from its XCD's head
#endif
	if (LDS) {
		RL_ARGS();
		const uint32_t nN = (uint32_t)(LDS == 2 ? S.numLeafRecords : S.numNodes4) * 8u, nT = (uint32_t)S.numTriangles * 4u, nM = (uint32_t)S.numMaterials * RL_LDS_MSTRIDE(PLAIN);
		for (uint32_t i = threadIdx.x; i < 4u; i += RL_BLOCK) s_scene[RL_LDS_ROOT + i] = ((const float4*)S.nodes)[i];
		for (uint32_t i = threadIdx.x; i < nN; i += RL_BLOCK) s_scene[RL_LDS_NODES + (i >> 3) * RL_LDS_NSTRIDE + (i & 7u)] = ((const float4*)(LDS == 2 ? S.leafList : S.nodes4f))[i];
		if (LDS == 2) {
			for (uint32_t i = threadIdx.x; i < nT; i += RL_BLOCK) s_scene[LdsAt<LDS>::SHADE + i] = ((const float4*)S.shade)[i];
			for (uint32_t t = threadIdx.x; t < (uint32_t)S.numTriangles; t += RL_BLOCK) {   // the six-float4 record (LdsAt): edges and own box worked out here, once
				const Tri T = LoadTri(S, (int)t);
				const V3 mn = v3(fminf(fminf(T.v0.x, T.v1.x), T.v2.x), fminf(fminf(T.v0.y, T.v1.y), T.v2.y), fminf(fminf(T.v0.z, T.v1.z), T.v2.z));
				const V3 mx = v3(fmaxf(fmaxf(T.v0.x, T.v1.x), T.v2.x), fmaxf(fmaxf(T.v0.y, T.v1.y), T.v2.y), fmaxf(fmaxf(T.v0.z, T.v1.z), T.v2.z));
				float4* r = s_scene + LdsAt<LDS>::ISECT + t * 6u;
				r[0] = make_float4(T.v0.x, T.v0.y, T.v0.z, T.n.x); r[1] = make_float4(T.n.y, T.n.z, T.u.x, T.u.y); r[2] = make_float4(T.u.z, T.v.x, T.v.y, T.v.z);
				r[3] = make_float4(T.uv, T.uu, T.vv, T.denom); r[4] = make_float4(mn.x, mn.y, mn.z, mx.x); r[5] = make_float4(mx.y, mx.z, T.rden, 0.0f);
			}
		} else {
			for (uint32_t i = threadIdx.x; i < nT; i += RL_BLOCK) { const uint32_t at = (i >> 2) * RL_LDS_TSTRIDE + (i & 3u); s_scene[LdsAt<LDS>::ISECT + at] = ((const float4*)S.isect)[i]; s_scene[LdsAt<LDS>::SHADE + at] = ((const float4*)S.shade)[i]; }
		}
		for (uint32_t i = threadIdx.x; i < nM; i += RL_BLOCK) s_scene[LdsAt<LDS>::MATS + i] = ((const float4*)S.materials)[PLAIN ? (i >> 2) * 5u + (i & 3u) : i];
		__syncthreads();
	}
	int* stk = s_stack + threadIdx.x;
	const uint32_t gtid = blockIdx.x * RL_BLOCK + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t numSlots;
	JobSource js;
	{ RL_ARGS(); numSlots = P.numLocalCells * 64u; js = JobSourceInit(P); }

	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	Rng g; g.s.state = 0;
	V3 o = v3s(0.0f), d = v3s(0.0f);
	float rayTime = 0.0f;
	int depth = 0;
	uint32_t outIndex = 0;
	bool active = false;
	bool exhausted = false;
#if RL_LAZY_REFL
	bool lit = false;                          // the path has met light, or a vertex whose reflectance may not be skipped (LazyVertexSafe)
	uint32_t litChunk = ~0u, litFill = RL_LIT_CHUNK;   // wave-uniform: the wave's chunk of the lit list and the entries filled in it (none yet: "full")
	bool litFull = false;                      // wave-uniform: the list has no chunk left
	uint32_t nLit = 0, nInPlace = 0;
#endif

	// Wave-local job range: the wave takes P.jobChunk (64..1024) consecutive jobs from the global counter
	// with ONE atomic and deals them to its lanes itself.  (A returning atomic on one address
	// saturates near 88 dequeues/us chip-wide -- MI355X_MICROARCH.md "dequeue" -- and one atomic
	// per wave and bounce was exactly that rate: the kernel ran at the atomic's speed.)
	// (Round 2 gave every wave its first chunk without an atomic, because 4096 waves asking ONE counter at the same instant stood in line for ~45 us; with a
	// head per XCD the line is an eighth as long and the first chunk comes from the wave's own band like every other.)
	uint32_t chunkNext = 0, chunkEnd = 0;
	bool globalDone = false;
	uint32_t qCount = 0;   // LDS == 2: camera rays waiting in the wave's queue
	RL_TIMELINE(0);
#ifdef RL_DIAG_STAMPS
	// diagnostic build only: shader-clock time per phase (refill | traverse | shade | fold), summed per wave
	unsigned long long stampAcc[4] = { 0, 0, 0, 0 }, subAcc[4] = { 0, 0, 0, 0 }, laneAcc[4] = { 0, 0, 0, 0 }, laneT[4] = { 0, 0, 0, 0 };
	{ RL_ARGS(); c.diag = counters; }
	unsigned long long stampLast = __builtin_amdgcn_s_memtime();
	#define RL_SUBSTAMP(k) { __builtin_amdgcn_sched_barrier(0); const unsigned long long now_ = __builtin_amdgcn_s_memtime(); subAcc[k] += now_ - subLast; subLast = now_; __builtin_amdgcn_sched_barrier(0); }
	unsigned long long subLast = 0;
	#define RL_STAMP(k) { __builtin_amdgcn_sched_barrier(0); const unsigned long long now_ = __builtin_amdgcn_s_memtime(); stampAcc[k] += now_ - stampLast; stampLast = now_; __builtin_amdgcn_sched_barrier(0); }
	// lane-weighted: clock x lanes that took part in the phase (k: 0 traverse, 1 shade a hit, 2 miss shader, 3 fold)
	#define RL_LANESTAMP(k, cond) { __builtin_amdgcn_sched_barrier(0); const unsigned long long now_ = __builtin_amdgcn_s_memtime(); laneAcc[k] += (now_ - laneLast) * (unsigned long long)__popcll(Ballot(cond)); laneT[k] += now_ - laneLast; __builtin_amdgcn_sched_barrier(0); }
	#define RL_LANEBEGIN() { __builtin_amdgcn_sched_barrier(0); laneLast = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
	unsigned long long laneLast = 0;
#else
	#define RL_STAMP(k)
	#define RL_SUBSTAMP(k)
	#define RL_LANESTAMP(k, cond)
	#define RL_LANEBEGIN()
#endif

#ifdef RL_WATCHDOG
	unsigned guardMain = 0;
#endif
	for (;;) {
#ifdef RL_WATCHDOG
		if (++guardMain > 200000u) { if (lane == 0) printf("k_trace main loop stuck: block %u wave %u active %llx exhausted %llx qCount %u globalDone %d chunk %u %u depth %d\n", blockIdx.x, threadIdx.x >> 6, (unsigned long long)Ballot(active), (unsigned long long)Ballot(exhausted), qCount, (int)globalDone, chunkNext, chunkEnd, depth); break; }
#endif
		// ---- refill idle lanes: wave64 ballot + prefix rank ----
		// Up to RL_REFILL_ROUNDS rounds: a fresh camera ray that misses both boxes of the root node can
		// only run the (sun-less) miss shader, so it is finished here and its lane takes another job at
		// once instead of occupying a lane slot through a whole bounce trip (in a 16:9 Cornell frame
		// more than half of the camera samples never touch the scene).
		if constexpr (LDS == 2) {
			RL_ARGS();
			// Leaf-list scenes need no traversal stack, and its LDS (1024 dwords per wave) is a QUEUE of camera rays instead: rays are
			// generated 64 at a time -- every lane takes a job, the same code for all of them -- the ones that cannot hit anything are finished
			// on the spot as in the rounds below, the others are written to the queue back to back (ballot + prefix rank), and the idle
			// lanes take theirs from its end.  The rounds below generate for the idle lanes only: a third of the wave in the first round, then a half
			// of that (in a 16:9 Cornell frame more than half of the camera samples miss the room), a quarter ... at the cost of a whole wave each time.
			enum { QCAP = 112, QFIELDS = 9 };   // 9 x 112 dwords <= 1024
			int* q = s_stack + (threadIdx.x >> 6) * (STACK * 64);
			const bool need = !active && !exhausted;
			const unsigned long long needMask = Ballot(need);
			const uint32_t n = (uint32_t)__popcll(needMask);
			while (n > 0 && qCount < n && qCount <= QCAP - 64 && !(globalDone && chunkNext >= chunkEnd)) {
#if RL_QUEUE_SHARED_CHUNK
				// The next batch of the workgroup's chunk: one LDS atomic.  The chunk is the granule of the GLOBAL job list (one global atomic per
				// P.jobChunk jobs, as before), the batch the granule of a wave's work: when the list runs dry a wave has at most its batch in
				// front of it, not a chunk -- the launch's tail shrinks from "one chunk per wave" to "a quarter of one".
				// Whoever finds the chunk used up takes the lock, asks the global counter and publishes the new chunk; the others wait for it.
				for (;;) {
					unsigned long long st = 0ull;
					if (lane == 0) st = atomicAdd(&s_jobs, 64ull);
					st = __shfl(st, 0);
					const uint32_t nx = (uint32_t)st, en = (uint32_t)(st >> 32);
					if (nx < en) { chunkNext = nx; chunkEnd = min(nx + 64u, en); break; }
					if (__atomic_load_n(&s_done, __ATOMIC_RELAXED) != 0u) { globalDone = true; chunkNext = chunkEnd = 0; break; }
					uint32_t won = 0;
					if (lane == 0) won = atomicCAS(&s_lock, 0u, 1u) == 0u ? 1u : 0u;
					won = __shfl(won, 0);
					if (won) {
						__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
						const unsigned long long cur = __atomic_load_n(&s_jobs, __ATOMIC_RELAXED);
						if ((uint32_t)cur >= (uint32_t)(cur >> 32) && __atomic_load_n(&s_done, __ATOMIC_RELAXED) == 0u) {   // still used up: nobody refilled it in between
							uint32_t base = 0, bend = 0;
							const bool got = TakeJobs(P, jobCounter, js, P.jobChunk, lane, base, bend);
							if (lane == 0) {
								if (!got) __atomic_store_n(&s_done, 1u, __ATOMIC_RELAXED);
								else __atomic_store_n(&s_jobs, (unsigned long long)base | ((unsigned long long)bend << 32), __ATOMIC_RELAXED);
							}
						}
						__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
						if (lane == 0) __atomic_store_n(&s_lock, 0u, __ATOMIC_RELAXED);
					} else {
						// wait for the wave that is asking the global counter (microseconds).  Not for ever: a wave that has waited ~1 ms stops relying
						// on its neighbours and takes one batch straight from the global counter -- always correct, the counter is the truth
#if RL_QUEUE_SPIN_LIMIT == 0
						while (__atomic_load_n(&s_lock, __ATOMIC_RELAXED) != 0u) __builtin_amdgcn_s_sleep(2);
						if (false) {
#else
						uint32_t spins = 0;
						while (__atomic_load_n(&s_lock, __ATOMIC_RELAXED) != 0u && ++spins < RL_QUEUE_SPIN_LIMIT) __builtin_amdgcn_s_sleep(2);
						if (spins >= RL_QUEUE_SPIN_LIMIT) {
#endif
							uint32_t base = 0, bend = 0;
							if (!TakeJobs(P, jobCounter, js, 64u, lane, base, bend)) { globalDone = true; chunkNext = chunkEnd = 0; }
							else { chunkNext = base; chunkEnd = bend; }
							break;
						}
					}
				}
				if (globalDone) { RL_TIMELINE(1); break; }
#else
				if (chunkNext >= chunkEnd) {
					uint32_t base = 0, bend = 0;
					if (!TakeJobs(P, jobCounter, js, P.jobChunk, lane, base, bend)) { globalDone = true; RL_TIMELINE(1); break; }
					chunkNext = base; chunkEnd = bend;
				}
#endif
				const uint32_t avail = chunkEnd - chunkNext;
				bool survive = false;
				V3 qo = v3s(0.0f), qd = v3s(0.0f); Rng qg; qg.s.state = 0; uint32_t qOut = 0;
				if (lane < avail) {
#if RL_VIEWS_TWIN
					RL_VIEWS();
					uint32_t view;
					const JobPixel j = DecodeJobBatchViews(P, VW, chunkNext, lane, view);   // (one (cell, sample): the view is wave-uniform)
#else
					const JobPixel j = DecodeJobBatch(P, chunkNext, lane);
#endif
					if (j.valid) {
						// GenerateCell body, reference render/renderer.cc:232-239
						const uint32_t sm_ = P.sampleBegin + j.sample;
						qg.s = raylib_rng_begin_mixed(P.seedMixed, j.y * P.width + j.x, sm_);
						float u, v;
						PixelUV(P, j.x, j.y, sm_, qg, u, v);
						float qTime;
#if RL_VIEWS_TWIN
						CameraRay(LoadViewCameraUniform(VW, view), u, v, qg, qo, qd, qTime);
#else
						CameraRay(P.camera, u, v, qg, qo, qd, qTime);
#endif
						qOut = j.sample * numSlots + j.slot;
						c.samples++;
						survive = true;
						if (P.maxPathLength > 0 && RootMiss<LDS>(S, qo, qd, P.rayTMin, sm)) {
							const bool sunQuick = !S.hasSun || RootMiss<LDS>(S, qo, -ld3(S.sunDirection), P.rayTMin, sm);
							if (sunQuick) {
								c.rays++; c.nodes++;   // the closest-hit query this replaces fetches the root node and stops
								DSceneView Sq = S; Sq.hasSun = 0;
								V3 L = MissShader<STACK, PRIMS, FULL, LDS, PLAIN>(Sq, R, qo, qd, qTime, P.rayTMin, stk, c, sm);
								if (S.hasSun) { c.rays++; c.nodes++; L = L + ld3(S.sunIlluminance); }
#if RL_LAZY_REFL
								RL_LIT_ARGS();
								if (!LL.mask) samples[qOut] = make_sample(L.x, L.y, L.z);
								else if (AnyBitSet(L)) {   // the lit-sample mask's rule (rl_lit_mask.h): all zero bits, neither stored nor flagged
									samples[qOut] = make_sample(L.x, L.y, L.z);
									atomicOr(&LL.mask[LitMaskWord(j.sample, numSlots, j.slot)], LitMaskBit(j.sample));
								}
#else
								samples[qOut] = make_sample(L.x, L.y, L.z);
#endif
								survive = false;
							}
						}
					}
				}
				chunkNext += min(64u, avail);
				const unsigned long long sv = Ballot(survive);
				if (survive) {
					const uint32_t at = qCount + (uint32_t)__popcll(sv & ((1ull << lane) - 1ull));
					q[0 * QCAP + at] = __float_as_int(qo.x); q[1 * QCAP + at] = __float_as_int(qo.y); q[2 * QCAP + at] = __float_as_int(qo.z);
					q[3 * QCAP + at] = __float_as_int(qd.x); q[4 * QCAP + at] = __float_as_int(qd.y); q[5 * QCAP + at] = __float_as_int(qd.z);
					q[6 * QCAP + at] = (int)(uint32_t)qg.s.state; q[7 * QCAP + at] = (int)(uint32_t)(qg.s.state >> 32); q[8 * QCAP + at] = (int)qOut;
				}
				qCount += (uint32_t)__popcll(sv);
				WaveLdsSync();
			}
			if (need) {
				const uint32_t rank = (uint32_t)__popcll(needMask & ((1ull << lane) - 1ull));
				if (rank < qCount) {
					const uint32_t at = qCount - 1u - rank;
					o = v3(__int_as_float(q[0 * QCAP + at]), __int_as_float(q[1 * QCAP + at]), __int_as_float(q[2 * QCAP + at]));
					d = v3(__int_as_float(q[3 * QCAP + at]), __int_as_float(q[4 * QCAP + at]), __int_as_float(q[5 * QCAP + at]));
					g.s.state = (uint64_t)(uint32_t)q[6 * QCAP + at] | ((uint64_t)(uint32_t)q[7 * QCAP + at] << 32);
					outIndex = (uint32_t)q[8 * QCAP + at];
					rayTime = 0.0f;   // leaf-list scenes are triangle scenes: nothing moves, the ray's time is not read
					depth = 0;
					active = true;
#if RL_LAZY_REFL
					lit = false;
#endif
				} else if (globalDone && chunkNext >= chunkEnd) exhausted = true;
			}
			qCount -= min(n, qCount);
			WaveLdsSync();
		} else
		for (int round = 0; round < RL_REFILL_ROUNDS; ++round) {
			RL_ARGS();
			const bool need = !active && !exhausted;
			const unsigned long long mask = Ballot(need);
			if (mask == 0ull) break;
			if (chunkNext >= chunkEnd && !globalDone) {
				uint32_t base = 0, bend = 0;
				if (!TakeJobs(P, jobCounter, js, P.jobChunk, lane, base, bend)) { globalDone = true; RL_TIMELINE(1); }
				else { chunkNext = base; chunkEnd = bend; }
			}
			const uint32_t avail = chunkEnd - chunkNext;
			if (need) {
				const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
				if (rank >= avail) {
					if (globalDone) exhausted = true;   // else: served in a later round / trip from the next chunk
				} else {
					const uint32_t job = chunkNext + rank;
#if RL_VIEWS_TWIN
					RL_VIEWS();
					uint32_t view;
					const JobPixel j = DecodeJobViews(P, VW, job, view);
#else
					const JobPixel j = DecodeJob(P, job);
#endif
					if (j.valid) {
						// GenerateCell body, reference render/renderer.cc:232-239
						const uint32_t s = P.sampleBegin + j.sample;
						g.s = raylib_rng_begin_mixed(P.seedMixed, j.y * P.width + j.x, s);
						float u, v;
						PixelUV(P, j.x, j.y, s, g, u, v);
#if RL_VIEWS_TWIN
						CameraRay(LoadViewCamera(VW, view), u, v, g, o, d, rayTime);
#else
						CameraRay(P.camera, u, v, g, o, d, rayTime);
#endif
						depth = 0;
						outIndex = j.sample * numSlots + j.slot;
						active = true;
						c.samples++;
						if (P.maxPathLength > 0 && RootMiss<LDS>(S, o, d, P.rayTMin, sm)) {
							// The camera ray cannot hit anything.  Its miss shader (renderer.cc:155-199) is the sky lookup plus,
							// with a sun, one occlusion query from the ray origin; if that shadow ray misses the root too, the
							// whole sample is decided here.
							const bool sunQuick = !S.hasSun || RootMiss<LDS>(S, o, -ld3(S.sunDirection), P.rayTMin, sm);
							if (sunQuick) {
								c.rays++; c.nodes++;   // the closest-hit query this replaces fetches the root node and stops
								DSceneView Sq = S; Sq.hasSun = 0;
								V3 L = MissShader<STACK, PRIMS, FULL, LDS, PLAIN>(Sq, R, o, d, rayTime, P.rayTMin, stk, c, sm);
								if (S.hasSun) { c.rays++; c.nodes++; L = L + ld3(S.sunIlluminance); }
								samples[outIndex] = make_sample(L.x, L.y, L.z);
								active = false;
							}
						}
					}
				}
			}
			chunkNext += min((uint32_t)__popcll(mask), avail);
		}
		if (Ballot(active) == 0ull) {
			if (Ballot(!exhausted) == 0ull) break;
			continue;
		}

		// ---- one bounce for every active lane (TraceScene, reference render/renderer.cc:114-208) ----
		if (lane == 0) c.trips++;
		RL_STAMP(0);
		RL_LANEBEGIN();
		HitRec h; h.tri = -1;
		bool doTrace, hit = false;
		{
		RL_ARGS();
		doTrace = active && depth < P.maxPathLength;   // renderer.cc:120-123 otherwise
		// the 4-wide tree when the launch carries it (triangle scenes; half the steps: 24.6 -> 22.4 ms on the Cornell frame)
		if (doTrace) {
			if constexpr (LDS != 0) hit = Traverse4<STACK, false, PRIMS, FULL, LDS, PLAIN>(S, o, d, rayTime, P.rayTMin, h, stk, c, sm);   // an LDS-resident scene has its wide tree
			else hit = (!PRIMS && (FULL ? (const void*)S.nodes4f : (const void*)S.nodes4)) ? Traverse4<STACK, false, PRIMS, FULL, LDS>(S, o, d, rayTime, P.rayTMin, h, stk, c, sm) : Traverse<STACK, false, PRIMS>(S, o, d, rayTime, P.rayTMin, h, stk, c);
		}
		}
		RL_LANESTAMP(0, doTrace);
		RL_STAMP(1);
#if RL_LAZY_REFL
		// what a lane whose path ended lit in this trip leaves for the wave-level part behind the block: its terminal L, and a last vertex that is recorded
		// (it failed LazyVertexSafe) in registers, on top of the depth records of the path stack
		bool finLit = false, finTop = false;
		float4 finRec0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), finRec1 = finRec0;
		V3 finL = v3s(0.0f);
#endif
		if (active) {
			bool done = false, store = false;
			float4 rec0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rec1 = rec0;
			V3 L = v3s(0.0f);
			if (!doTrace) {
				done = true;
			} else if (hit) {
				RL_ARGS();
				Surf s;
				RL_LANEBEGIN();
#ifdef RL_DIAG_STAMPS
				subLast = __builtin_amdgcn_s_memtime();
#endif
				const int mi = BuildSurface<PRIMS, LDS>(S, o, d, h, s, true, c, sm);
				const Mat m = LDS ? MatFrom<PLAIN>(sm + LdsAt<LDS>::MATS + mi * RL_LDS_MSTRIDE(PLAIN)) : LoadMat(S, mi);
				RL_SUBSTAMP(0);
#if RL_LAZY_REFL
				V3 Wo = v3s(0.0f), Wh = v3s(0.0f), outD = v3s(0.0f);
				float pdf = 0.0f, sp = 0.0f;
				bool exactSp = false;
				ScatterLazy(S, m, d, s, g, c, Wo, Wh, outD, pdf, sp, exactSp);
				RL_SUBSTAMP(1);
				const V3 E = Emitted(S, m, s, c);
				if (AnyBitSet(E)) lit = true;
				if (pdf > 0.0f) {
					const bool safe = LazyVertexSafe(Wo, Wh, sp);   // (a quick event's sp slot holds wh.z, finite like the sp it stands for: LazyPdfQuick)
					if (!safe) lit = true;
					const bool last = depth + 1 >= P.maxPathLength;
					if (last && safe) {
						// the path's last vertex (the eager instance's comment below): its finite reflectance meets L = 0, the step comes to (0 + +-0) + E
						L = v3s(0.0f) + E;
						done = true;
					} else {
						// the vertex record (Wo, sp or wh.z | Wh, material and which of the two): what ReflFromRecord, sp, the pdf and the emission are functions of
						store = true;
						rec0 = make_float4(Wo.x, Wo.y, Wo.z, sp);
						rec1 = make_float4(Wh.x, Wh.y, Wh.z, __int_as_float(exactSp ? mi | RL_LAZY_REC_EXACT_SP : mi));
						if (last) done = true;   // (L = 0: the record is folded like every other, from the registers)
						else { o = s.p; d = outD; }
					}
				} else {
					L = v3s(0.0f) + E;
					done = true;
				}
#else
				V3 refl = v3s(0.0f), outD = v3s(0.0f);
				float pdf = 0.0f, sp = 0.0f;
				const bool scattered = Scatter<PLAIN>(S, m, d, s, g, c, refl, outD, pdf, sp);
				RL_SUBSTAMP(1);
				const V3 E = Emitted(S, m, s, c);
				if (scattered && pdf > 0.0f) {
					if (depth + 1 >= P.maxPathLength) {
						// the next TraceScene returns 0 at once (renderer.cc:120-123): this vertex is the path's last, and its step of the
						// fold -- radiance = (0 + refl * 0 * sp / pdf) + E, the reference's expression -- is taken from the registers
						V3 radiance = v3s(0.0f);
						radiance = radiance + refl * L * sp / pdf;
						radiance = radiance + E;
						L = radiance;
						done = true;
					} else {
						// the vertex record (refl, sp | pdf, E) goes to the path stack BEHIND this trip's fold (below): a wave counts loads and
						// stores in one in-order counter, and a fold that waits for its loads behind this trip's stores waits for their write
						// acknowledgements too
						store = true;
						rec0 = make_float4(refl.x, refl.y, refl.z, sp);
						rec1 = make_float4(pdf, E.x, E.y, E.z);
						o = s.p; d = outD;
					}
				} else {
					L = v3s(0.0f) + E;                        // radiance(0) += Emitted, renderer.cc:137,151
					done = true;
				}
#endif
				RL_SUBSTAMP(2);
				RL_LANESTAMP(1, true);
			} else {
				RL_ARGS();
				RL_LANEBEGIN();
				L = MissShader<STACK, PRIMS, FULL, LDS, PLAIN>(S, R, o, d, rayTime, P.rayTMin, stk, c, sm);
				done = true;
				RL_LANESTAMP(2, true);
			}
			RL_STAMP(2);
#if RL_LAZY_REFL
			if (done) {
				RL_ARGS();
				if (AnyBitSet(L)) lit = true;
				// an unlit path: every E and the terminal L are +0 and every vertex passed LazyVertexSafe, so every step of the fold is (0 + +-0) + 0 = +0
				// (with a lit-sample mask it is neither stored nor flagged: rl_lit_mask.h)
				if (!lit) { RL_LIT_ARGS(); if (!LL.mask) samples[outIndex] = make_sample(0.0f, 0.0f, 0.0f); }
				else { finLit = true; finTop = store; finRec0 = rec0; finRec1 = rec1; finL = L; }
				active = false;
			} else if (store) {
				RL_ARGS();
				float4* st = (float4*)pathStack + ((size_t)depth * P.stackStride + gtid) * 2u;
				st[0] = rec0; st[1] = rec1;
				depth++;
			}
		}
		if (Ballot(finLit) != 0ull) {
			// ---- the lit paths that ended in this trip, wave-wide (rl_dev_litfold.h): an entry of the lit list each, reserved in the wave's chunk and, when that
			// is full, in one more; the chunk these entries complete is folded here by the whole wave, 64 entries in 64 lanes.  A path with more records than an
			// entry holds, or without an entry because the list is used up, folds in place: slow, rare, the same statements on the same values.
			RL_ARGS();
			RL_LIT_ARGS();
			const int nrec = depth + (finTop ? 1 : 0);
			uint32_t full;
			const uint32_t entry = LitReserve(LL, lane, finLit && nrec <= RL_FOLD_PREFETCH, litChunk, litFill, litFull, full);
			if (finLit) {
				nLit++;
				if (entry != ~0u) {
					float4* e = (float4*)LL.entries + (size_t)entry * RL_LIT_STRIDE;
					e[0] = make_float4(finL.x, finL.y, finL.z, __uint_as_float(outIndex));
					e[1] = make_float4(__int_as_float(nrec), 0.0f, 0.0f, 0.0f);
					#pragma unroll
					for (int k = 0; k < RL_FOLD_PREFETCH; ++k) {
						if (k < depth) {
							const float4* st = (const float4*)pathStack + ((size_t)k * P.stackStride + gtid) * 2u;
							e[2 + 2 * k] = st[0]; e[3 + 2 * k] = st[1];
						} else if (k == depth && finTop) { e[2 + 2 * k] = finRec0; e[3 + 2 * k] = finRec1; }
					}
				} else {
					nInPlace++;
					LitFoldInPlace(LL, sm, samples, numSlots, outIndex, finL, nrec, depth, (const float4*)pathStack + (size_t)gtid * 2u, (size_t)P.stackStride * 2u, finRec0, finRec1);
				}
			}
			if (full != ~0u) LitFoldChunk(LL, sm, samples, numSlots, full, RL_LIT_CHUNK, lane);
		}
		{   // (a bare block: the eager branch below is still inside `if (active)`, and the brace behind #endif closes either)
#else
			if (done) {
				RL_ARGS();
				RL_LANEBEGIN();
				// fold back to the camera: radiance = (0 + refl*Li*sp/pdf) + E at every vertex
#if RL_FOLD_PREFETCH > 0
				if (depth <= RL_FOLD_PREFETCH) {
					// all vertex records of the path are fetched before the dependent chain starts (one memory latency instead of one per vertex)
					float4 q0[RL_FOLD_PREFETCH], q1[RL_FOLD_PREFETCH];
					#pragma unroll
					for (int k = 0; k < RL_FOLD_PREFETCH; ++k) {
						const int kk = k < depth ? k : 0;
						const float4* st = (const float4*)pathStack + ((size_t)kk * P.stackStride + gtid) * 2u;
						q0[k] = st[0]; q1[k] = st[1];
					}
					#pragma unroll
					for (int k = RL_FOLD_PREFETCH - 1; k >= 0; --k) {
						if (k < depth) {
							const V3 refl = v3(q0[k].x, q0[k].y, q0[k].z);
							const float sp = q0[k].w, pdf = q1[k].x;
							const V3 E = v3(q1[k].y, q1[k].z, q1[k].w);
							V3 radiance = v3s(0.0f);
							radiance = radiance + refl * L * sp / pdf;
							radiance = radiance + E;
							L = radiance;
						}
					}
				} else
#endif
				for (int k = depth - 1; k >= 0; --k) {
					const float4* st = (const float4*)pathStack + ((size_t)k * P.stackStride + gtid) * 2u;
					const float4 r0 = st[0], r1 = st[1];
					const V3 refl = v3(r0.x, r0.y, r0.z);
					const float sp = r0.w, pdf = r1.x;
					const V3 E = v3(r1.y, r1.z, r1.w);
					V3 radiance = v3s(0.0f);
					radiance = radiance + refl * L * sp / pdf;
					radiance = radiance + E;
					L = radiance;
				}
				samples[outIndex] = make_sample(L.x, L.y, L.z);
				active = false;
				RL_LANESTAMP(3, true);
			}
			if (store) {
				RL_ARGS();
				// path vertex record: 32 contiguous bytes per lane, two 16-byte stores
				float4* st = (float4*)pathStack + ((size_t)depth * P.stackStride + gtid) * 2u;
				st[0] = rec0; st[1] = rec1;
				depth++;
			}
#endif
		}
		RL_STAMP(3);
	}

	RL_ARGS();
#if RL_LAZY_REFL
	{   // the chunk the wave still holds: its first litFill entries (litChunk is ~0u when the wave had no lit path, or the list ran out at its last reservation)
		RL_LIT_ARGS();
		if (litChunk != ~0u) LitFoldChunk(LL, sm, samples, numSlots, litChunk, litFill, lane);
	}
#endif
#ifdef RL_DIAG_STAMPS
	if (lane == 0) for (int k = 0; k < 4; ++k) { atomicAdd(&counters[CNT_COUNT + k], stampAcc[k]); atomicAdd(&counters[CNT_COUNT + 8 + k], subAcc[k]); atomicAdd(&counters[CNT_COUNT + 12 + k], c.tAcc[k]); atomicAdd(&counters[CNT_COUNT + 20 + k], laneAcc[k]); if (RL_DIAG_STAMPS < 2) atomicAdd(&counters[CNT_COUNT + 4 + k], laneT[k]); }
#endif
	RL_TIMELINE(2);
	// ---- counters: wave reduction, one atomic per wave and counter ----
	uint32_t vals[CNT_COUNT] = { c.rays, c.nodes, c.tris, c.shaded, c.texels, c.samples, c.trips };
	for (int k = 0; k < CNT_COUNT; ++k) {
		unsigned long long v = vals[k];
		for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
		if (lane == 0 && v) atomicAdd(&counters[k], v);
	}
#if RL_LAZY_REFL
	const uint32_t lz[2] = { nLit, nInPlace };
	for (int k = 0; k < 2; ++k) {
		unsigned long long v = lz[k];
		for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
		if (lane == 0 && v) atomicAdd(&counters[RL_CNT_LIT + k], v);
	}
#endif
}

