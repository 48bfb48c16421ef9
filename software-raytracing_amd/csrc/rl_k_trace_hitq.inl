// k_trace_lazy_hitq, the hit-queue instance of the leaf-list kernel's lazy-reflectance instance (rl_k_trace.inl RL_LAZY_REFL; rl_dev_shade.h "lazy-reflectance
// instance"), included by rl_render_lazy.hip alone: LDS == 2, PLAIN, one view.  The same paths, each with the statements and the values k_trace_lazy gives it and
// its own generator carried along; what differs is which lane runs a path, and when.
// k_trace_lazy refills its idle lanes with camera RAYS in front of the traversal, so a lane whose ray leaves the scene (a fifth of them on the Cornell frame: the
// bounce rays that leave the box through its open front) sits idle through the shading part, which the wave pays for whether 51 or 64 lanes are in it.  This
// instance refills behind the traversal, with camera rays that have been traced already: the wave's queue holds HITS.  Per trip:
//   1. stock   while the job list is not used up and the queue has room for a whole batch: 64 jobs, their camera rays, the root test, the walk; a ray that misses
//              is finished in the batch, a hit goes to the queue;
//   2. walk    the lanes that hold a bounce ray trace it; a miss runs the miss shader and ends the path;
//   3. pop     every free lane takes a queued hit;
//   4. shade   all active lanes: every one of them holds a hit;
//   5. the wave-level part that finishes the lit paths that ended in this trip, as in k_trace_lazy (rl_dev_litfold.h has the statements of both): a path of at
//              most RL_FOLD_PREFETCH records becomes an entry of the wave's chunk of the lit list, and the wave that writes a chunk's 64th entry folds the chunk
//              there, entry `lane` in lane `lane`; a path with more records, or without an entry because the list is used up, folds in place, in its lane alone.
//              This instance ends lit paths at two places -- a camera ray that misses into light in a batch (part 1), and the trip's paths -- and reserves, writes
//              and folds the same way at both;
//   6. exit    behind the loop the wave folds the chunk it still holds, up to the entries it filled.  No kernel follows to finish the list.
// No path changes its lane once it has one, the queue is the wave's own 1024 dwords of s_stack, and nothing here waits for another wave but the draw of a chunk.
// maxPathLength >= 1 (the planner keeps k_trace_lazy otherwise: a camera ray is traced before its path has a depth to test).

template <int STACK, bool PRIMS, bool FULL, int LDS, bool PLAIN>
__global__ void __launch_bounds__(RL_BLOCK, (STACK <= 32 ? RL_TRACE_MIN_WAVES : 2))
k_trace_lazy_hitq(const DRenderParams Pk, const DSceneView Sk, const SkyRot Rk, SampleRGB* __restrict__ samplesK,
                  float* __restrict__ pathStackK, unsigned long long* __restrict__ countersK, unsigned int* __restrict__ jobCounterK, const DLitList LLk)
{
	static_assert(LDS == 2 && PLAIN && !PRIMS && RL_QUEUE_SHARED_CHUNK, "the hit-queue instance is the leaf-list kernel's PLAIN instance, its chunk the workgroup's");
	(void)Pk; (void)Sk; (void)Rk; (void)samplesK; (void)pathStackK; (void)countersK; (void)jobCounterK; (void)LLk;
	RL_TEX_PROLOGUE(Sk);
	RL_MATH_PROLOGUE();
	__shared__ int s_stack[STACK * RL_BLOCK];
	__shared__ float4 s_scene[LdsAt<LDS>::TOTAL];
	const float4* sm = s_scene;
	// the workgroup's four waves draw their batches of 64 jobs from ONE chunk (low word: next job, high word: end of the chunk), as in k_trace_lazy
	__shared__ unsigned long long s_jobs;
	__shared__ unsigned int s_lock, s_done;
	if (threadIdx.x == 0) { s_jobs = 0ull; s_lock = 0u; s_done = 0u; }
	{   // the scene into LDS: k_trace's layout (rl_k_trace.inl, LDS == 2)
		RL_ARGS();
		const uint32_t nN = (uint32_t)S.numLeafRecords * 8u, nT = (uint32_t)S.numTriangles * 4u, nM = (uint32_t)S.numMaterials * RL_LDS_MSTRIDE(PLAIN);
		for (uint32_t i = threadIdx.x; i < 4u; i += RL_BLOCK) s_scene[RL_LDS_ROOT + i] = ((const float4*)S.nodes)[i];
		for (uint32_t i = threadIdx.x; i < nN; i += RL_BLOCK) s_scene[RL_LDS_NODES + (i >> 3) * RL_LDS_NSTRIDE + (i & 7u)] = ((const float4*)S.leafList)[i];
		for (uint32_t i = threadIdx.x; i < nT; i += RL_BLOCK) s_scene[LdsAt<LDS>::SHADE + i] = ((const float4*)S.shade)[i];
		for (uint32_t t = threadIdx.x; t < (uint32_t)S.numTriangles; t += RL_BLOCK) {
			const Tri T = LoadTri(S, (int)t);
			const V3 mn = v3(fminf(fminf(T.v0.x, T.v1.x), T.v2.x), fminf(fminf(T.v0.y, T.v1.y), T.v2.y), fminf(fminf(T.v0.z, T.v1.z), T.v2.z));
			const V3 mx = v3(fmaxf(fmaxf(T.v0.x, T.v1.x), T.v2.x), fmaxf(fmaxf(T.v0.y, T.v1.y), T.v2.y), fmaxf(fmaxf(T.v0.z, T.v1.z), T.v2.z));
			float4* r = s_scene + LdsAt<LDS>::ISECT + t * 6u;
			r[0] = make_float4(T.v0.x, T.v0.y, T.v0.z, T.n.x); r[1] = make_float4(T.n.y, T.n.z, T.u.x, T.u.y); r[2] = make_float4(T.u.z, T.v.x, T.v.y, T.v.z);
			r[3] = make_float4(T.uv, T.uu, T.vv, T.denom); r[4] = make_float4(mn.x, mn.y, mn.z, mx.x); r[5] = make_float4(mx.y, mx.z, T.rden, 0.0f);
		}
		for (uint32_t i = threadIdx.x; i < nM; i += RL_BLOCK) s_scene[LdsAt<LDS>::MATS + i] = ((const float4*)S.materials)[(i >> 2) * 5u + (i & 3u)];
		__syncthreads();
	}
	int* stk = s_stack + threadIdx.x;   // (handed to the walks, which do not read it: a leaf-list scene has no traversal stack)
	const uint32_t gtid = blockIdx.x * RL_BLOCK + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t numSlots;
	JobSource js;
	{ RL_ARGS(); numSlots = P.numLocalCells * 64u; js = JobSourceInit(P); }

	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	Rng g; g.s.state = 0;
	V3 o = v3s(0.0f), d = v3s(0.0f);
	int depth = 0;
	uint32_t outIndex = 0;
	bool active = false;
	bool lit = false;                          // the path has met light, or a vertex whose reflectance may not be skipped (LazyVertexSafe)
	uint32_t litChunk = ~0u, litFill = RL_LIT_CHUNK;   // wave-uniform: the wave's chunk of the lit list and the entries filled in it (none yet: "full")
	bool litFull = false;                      // wave-uniform: the list has no chunk left
	uint32_t nLit = 0, nInPlace = 0;

	// The wave's queue of camera-ray hits, struct of arrays in the 1024 dwords a tree walk would have as its stack: ray origin and direction, generator, outIndex
	// and the hit (t, a, b, triangle).  13 fields x 78 entries = 1014 dwords.  A batch adds 64 entries at most, so the wave stocks while 14 or fewer wait.
	enum { QFIELDS = 13, QCAP = (STACK * 64) / QFIELDS, QROOM = QCAP - 64 };
	static_assert(QROOM >= 0, "the queue holds a whole batch");
	int* q = s_stack + (threadIdx.x >> 6) * (STACK * 64);
	uint32_t qCount = 0;       // wave-uniform: hits waiting in the queue
	bool jobsDone = false;     // wave-uniform: the job list is used up -- no batch will follow
	RL_TIMELINE(0);

	for (;;) {
		// ---- 1. stock the hit queue: batches of 64 jobs, at the top of the trip, where the least of the lanes' own paths is live ----
		while (!jobsDone && qCount <= (uint32_t)QROOM) {
			RL_ARGS();
			// The next batch of the workgroup's chunk: one LDS atomic; whoever finds the chunk used up takes the lock, asks the global counter and publishes the new
			// chunk, the others wait for it (k_trace_lazy's draw: rl_k_trace.inl has the reasons).
			uint32_t chunkNext = 0, chunkEnd = 0;
			for (;;) {
				unsigned long long st = 0ull;
				if (lane == 0) st = atomicAdd(&s_jobs, 64ull);
				st = __shfl(st, 0);
				const uint32_t nx = (uint32_t)st, en = (uint32_t)(st >> 32);
				if (nx < en) { chunkNext = nx; chunkEnd = min(nx + 64u, en); break; }
				if (__atomic_load_n(&s_done, __ATOMIC_RELAXED) != 0u) { jobsDone = true; break; }
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
#if RL_QUEUE_SPIN_LIMIT == 0
					while (__atomic_load_n(&s_lock, __ATOMIC_RELAXED) != 0u) __builtin_amdgcn_s_sleep(2);
#else
					// not for ever: a wave that has waited its limit takes one batch straight from the global counter -- always correct, the counter is the truth
					uint32_t spins = 0;
					while (__atomic_load_n(&s_lock, __ATOMIC_RELAXED) != 0u && ++spins < RL_QUEUE_SPIN_LIMIT) __builtin_amdgcn_s_sleep(2);
					if (spins >= RL_QUEUE_SPIN_LIMIT) {
						uint32_t base = 0, bend = 0;
						if (!TakeJobs(P, jobCounter, js, 64u, lane, base, bend)) jobsDone = true;
						else { chunkNext = base; chunkEnd = bend; }
						break;
					}
#endif
				}
			}
			if (jobsDone) { RL_TIMELINE(1); break; }
			const uint32_t avail = chunkEnd - chunkNext;
			bool survive = false;
			V3 qo = v3s(0.0f), qd = v3s(0.0f); Rng qg; qg.s.state = 0; uint32_t qOut = 0;
			RL_LIT_ARGS();
			if (lane < avail) {
				const JobPixel j = DecodeJobBatch(P, chunkNext, lane);
				if (j.valid) {
					// GenerateCell body, reference render/renderer.cc:232-239
					const uint32_t sm_ = P.sampleBegin + j.sample;
					qg.s = raylib_rng_begin_mixed(P.seedMixed, j.y * P.width + j.x, sm_);
					float u, v;
					PixelUV(P, j.x, j.y, sm_, qg, u, v);
					float qTime;
					CameraRay(P.camera, u, v, qg, qo, qd, qTime);
					qOut = j.sample * numSlots + j.slot;
					c.samples++;
					survive = true;
					// a camera ray that misses both boxes of the root node (and whose sun ray does) is decided here, as in k_trace_lazy
					if (RootMiss<LDS>(S, qo, qd, P.rayTMin, sm)) {
						const bool sunQuick = !S.hasSun || RootMiss<LDS>(S, qo, -ld3(S.sunDirection), P.rayTMin, sm);
						if (sunQuick) {
							c.rays++; c.nodes++;   // the closest-hit query this replaces fetches the root node and stops
							DSceneView Sq = S; Sq.hasSun = 0;
							V3 L = MissShader<STACK, PRIMS, FULL, LDS, PLAIN>(Sq, R, qo, qd, qTime, P.rayTMin, stk, c, sm);
							if (S.hasSun) { c.rays++; c.nodes++; L = L + ld3(S.sunIlluminance); }
							if (!LL.mask) samples[qOut] = make_sample(L.x, L.y, L.z);
							else if (AnyBitSet(L)) {   // the lit-sample mask's rule (rl_lit_mask.h): all zero bits, neither stored nor flagged
								samples[qOut] = make_sample(L.x, L.y, L.z);
								atomicOr(&LL.mask[LitMaskWord(j.sample, numSlots, j.slot)], LitMaskBit(j.sample));
							}
							survive = false;
						}
					}
				}
			}
			// the survivors' first bounce (depth 0 < maxPathLength): the trip's walk and, for a miss, the trip's miss shader, on the same ray
			HitRec qh; qh.t = 0.0f; qh.a = 0.0f; qh.b = 0.0f; qh.tri = -1;
			bool qHit = false, qLit = false;
			V3 qL = v3s(0.0f);
			if (survive) {
				qHit = Traverse4<STACK, false, PRIMS, FULL, LDS, PLAIN>(S, qo, qd, 0.0f, P.rayTMin, qh, stk, c, sm);
				if (!qHit) {
					qL = MissShader<STACK, PRIMS, FULL, LDS, PLAIN>(S, R, qo, qd, 0.0f, P.rayTMin, stk, c, sm);
					// the path is done at depth 0 without a record.  Unlit: +0, which a lit-sample mask neither stores nor flags.  Lit: below.
					if (AnyBitSet(qL)) qLit = true;
					else if (!LL.mask) samples[qOut] = make_sample(0.0f, 0.0f, 0.0f);
				}
			}
			if (Ballot(qLit) != 0ull) {
				// A camera ray that missed into light (a sun): k_trace_lazy ends it in the wave-level part of its trip as a lit path of zero records -- an entry of the
				// lit list, whose fold is the identity, or, the list used up, in place -- and counts it in litPaths (and litFoldedInPlace).  The same here.
				uint32_t full;
				const uint32_t entry = LitReserve(LL, lane, qLit, litChunk, litFill, litFull, full);
				if (qLit) {
					nLit++;
					if (entry != ~0u) {
						float4* e = (float4*)LL.entries + (size_t)entry * RL_LIT_STRIDE;
						e[0] = make_float4(qL.x, qL.y, qL.z, __uint_as_float(qOut));
						e[1] = make_float4(__int_as_float(0), 0.0f, 0.0f, 0.0f);
					} else {
						nInPlace++;
						LitStoreSample(LL, samples, numSlots, qOut, qL);   // (any bit of qL is set)
					}
				}
				if (full != ~0u) LitFoldChunk(LL, sm, samples, numSlots, full, RL_LIT_CHUNK, lane);
			}
			const unsigned long long hv = Ballot(qHit);
			if (qHit) {
				const uint32_t at = qCount + (uint32_t)__popcll(hv & ((1ull << lane) - 1ull));
				q[0 * QCAP + at] = __float_as_int(qo.x); q[1 * QCAP + at] = __float_as_int(qo.y); q[2 * QCAP + at] = __float_as_int(qo.z);
				q[3 * QCAP + at] = __float_as_int(qd.x); q[4 * QCAP + at] = __float_as_int(qd.y); q[5 * QCAP + at] = __float_as_int(qd.z);
				q[6 * QCAP + at] = (int)(uint32_t)qg.s.state; q[7 * QCAP + at] = (int)(uint32_t)(qg.s.state >> 32); q[8 * QCAP + at] = (int)qOut;
				q[9 * QCAP + at] = __float_as_int(qh.t); q[10 * QCAP + at] = __float_as_int(qh.a); q[11 * QCAP + at] = __float_as_int(qh.b); q[12 * QCAP + at] = qh.tri;
			}
			qCount += (uint32_t)__popcll(hv);
			WaveLdsSync();
		}
		// ---- 6. exit ----
		// Behind the loop above jobsDone || qCount > QROOM >= 0.  So with no lane active and an empty queue the job list is used up: every job this wave drew has been
		// finished in its batch, or was queued, popped and run to its end, and no batch will follow.
		// Every turn makes progress towards that: a batch takes at least one job from the finite list or sets jobsDone; a trip with an active lane moves each active
		// path one vertex on or ends it (a path has at most maxPathLength vertices); a trip without one has qCount > 0 and 64 free lanes, and pops min(64, qCount) >= 1.
		if (Ballot(active) == 0ull && qCount == 0u) break;

		// ---- 2. one bounce for every lane that holds a ray (TraceScene, reference render/renderer.cc:114-208) ----
		if (lane == 0) c.trips++;
		HitRec h; h.t = 0.0f; h.a = 0.0f; h.b = 0.0f; h.tri = -1;
		// what a lane whose path ended lit in this trip leaves for the wave-level part behind the shading: its terminal L, and a last vertex that is recorded
		// (it failed LazyVertexSafe) in registers, on top of the depth records of the path stack
		bool finLit = false, finTop = false;
		float4 finRec0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), finRec1 = finRec0;
		V3 finL = v3s(0.0f);
		if (active) {
			RL_ARGS();
			bool hit = false;
			const bool doTrace = depth < P.maxPathLength;   // renderer.cc:120-123 otherwise (not reached: a path that continues has depth + 1 < maxPathLength)
			if (doTrace) hit = Traverse4<STACK, false, PRIMS, FULL, LDS, PLAIN>(S, o, d, 0.0f, P.rayTMin, h, stk, c, sm);
			if (!hit) {
				V3 L = v3s(0.0f);
				if (doTrace) L = MissShader<STACK, PRIMS, FULL, LDS, PLAIN>(S, R, o, d, 0.0f, P.rayTMin, stk, c, sm);
				if (AnyBitSet(L)) lit = true;
				// an unlit path: every E and the terminal L are +0 and every vertex passed LazyVertexSafe, so every step of the fold is (0 + +-0) + 0 = +0
				// (with a lit-sample mask it is neither stored nor flagged: rl_lit_mask.h)
				if (!lit) { RL_LIT_ARGS(); if (!LL.mask) samples[outIndex] = make_sample(0.0f, 0.0f, 0.0f); }
				else { finLit = true; finL = L; }
				active = false;
			}
		}

		// ---- 3. pop: every free lane takes a queued hit, by rank from the queue's end ----
		// (A lane whose path ended lit in the walk above is not free yet: its outIndex, its depth and its records of the path stack are read in part 5.  It waits
		// one trip, as do the lanes the queue has nothing for.)
		{
			const bool need = !active && !finLit;
			const unsigned long long needMask = Ballot(need);
			if (need) {
				const uint32_t rank = (uint32_t)__popcll(needMask & ((1ull << lane) - 1ull));
				if (rank < qCount) {
					const uint32_t at = qCount - 1u - rank;
					o = v3(__int_as_float(q[0 * QCAP + at]), __int_as_float(q[1 * QCAP + at]), __int_as_float(q[2 * QCAP + at]));
					d = v3(__int_as_float(q[3 * QCAP + at]), __int_as_float(q[4 * QCAP + at]), __int_as_float(q[5 * QCAP + at]));
					g.s.state = (uint64_t)(uint32_t)q[6 * QCAP + at] | ((uint64_t)(uint32_t)q[7 * QCAP + at] << 32);
					outIndex = (uint32_t)q[8 * QCAP + at];
					h.t = __int_as_float(q[9 * QCAP + at]); h.a = __int_as_float(q[10 * QCAP + at]); h.b = __int_as_float(q[11 * QCAP + at]); h.tri = q[12 * QCAP + at];
					depth = 0;
					lit = false;
					active = true;
				}
			}
			qCount -= min((uint32_t)__popcll(needMask), qCount);
			WaveLdsSync();
		}

		// ---- 4. shade: every active lane holds a hit (k_trace_lazy's statements) ----
		if (active) {
			RL_ARGS();
			bool done = false, store = false;
			float4 rec0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rec1 = rec0;
			V3 L = v3s(0.0f);
			Surf s;
			const int mi = BuildSurface<PRIMS, LDS>(S, o, d, h, s, true, c, sm);
			const Mat m = MatFrom<PLAIN>(sm + LdsAt<LDS>::MATS + mi * RL_LDS_MSTRIDE(PLAIN));
			V3 Wo = v3s(0.0f), Wh = v3s(0.0f), outD = v3s(0.0f);
			float pdf = 0.0f, sp = 0.0f;
			bool exactSp = false;
			ScatterLazy(S, m, d, s, g, c, Wo, Wh, outD, pdf, sp, exactSp);
			const V3 E = Emitted(S, m, s, c);
			if (AnyBitSet(E)) lit = true;
			if (pdf > 0.0f) {
				const bool safe = LazyVertexSafe(Wo, Wh, sp);   // (a quick event's sp slot holds wh.z, finite like the sp it stands for: LazyPdfQuick)
				if (!safe) lit = true;
				const bool last = depth + 1 >= P.maxPathLength;
				if (last && safe) {
					// the path's last vertex: its finite reflectance meets L = 0, the step comes to (0 + +-0) + E
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
			if (done) {
				if (AnyBitSet(L)) lit = true;
				if (!lit) { RL_LIT_ARGS(); if (!LL.mask) samples[outIndex] = make_sample(0.0f, 0.0f, 0.0f); }
				else { finLit = true; finTop = store; finRec0 = rec0; finRec1 = rec1; finL = L; }
				active = false;
			} else if (store) {
				float4* st = (float4*)pathStack + ((size_t)depth * P.stackStride + gtid) * 2u;
				st[0] = rec0; st[1] = rec1;
				depth++;
			}
		}

		// ---- 5. the lit paths that ended in this trip, wave-wide (k_trace_lazy's part): an entry of the lit list each, reserved in the wave's chunk, and the chunk
		// these entries complete folded here by the whole wave; a path with more records than an entry holds, or without an entry because the list is used up,
		// folds in place ----
		if (Ballot(finLit) != 0ull) {
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
	}

	RL_ARGS();
	{   // the chunk the wave still holds: its first litFill entries (litChunk is ~0u when the wave had no lit path, or the list ran out at its last reservation)
		RL_LIT_ARGS();
		if (litChunk != ~0u) LitFoldChunk(LL, sm, samples, numSlots, litChunk, litFill, lane);
	}
	RL_TIMELINE(2);
	// ---- counters: wave reduction, one atomic per wave and counter ----
	uint32_t vals[CNT_COUNT] = { c.rays, c.nodes, c.tris, c.shaded, c.texels, c.samples, c.trips };
	for (int k = 0; k < CNT_COUNT; ++k) {
		unsigned long long v = vals[k];
		for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
		if (lane == 0 && v) atomicAdd(&counters[k], v);
	}
	const uint32_t lz[2] = { nLit, nInPlace };
	for (int k = 0; k < 2; ++k) {
		unsigned long long v = lz[k];
		for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
		if (lane == 0 && v) atomicAdd(&counters[RL_CNT_LIT + k], v);
	}
}
