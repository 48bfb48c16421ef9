// k_trace_pool, the pool megakernel, and its views twin (RaylibAMD_RenderViews), one source for both: rl_render_pool.hip includes this file twice, with RL_VIEWS_TWIN 1
// and 0; prototypes and default template arguments: rl_kernels.h.  The twin takes the view table (DViews) as one more trailing argument; everything under RL_VIEWS_TWIN is the twin's alone, so that the
// one-view kernel is the token sequence it always was (a template flag would add an inlining level, which reorders the one-view kernel's code:
// tools/isa_equivalence.py).

template <int STACK, bool PRIMS, int K, int LSTACK, int WIDE>
__global__ void __launch_bounds__(RL_BLOCK, (PoolOcc<LSTACK, PRIMS, K>::kBlocks))
#if RL_VIEWS_TWIN
k_trace_pool_views(const DRenderParams Pk, const DSceneView Sk, const SkyRot Rk, SampleRGB* __restrict__ samplesK,
                   float* __restrict__ pathStackK, unsigned long long* __restrict__ countersK, unsigned int* __restrict__ jobCounterK, const DViews Vk)
#else
k_trace_pool(const DRenderParams Pk, const DSceneView Sk, const SkyRot Rk, SampleRGB* __restrict__ samplesK,
             float* __restrict__ pathStackK, unsigned long long* __restrict__ countersK, unsigned int* __restrict__ jobCounterK)
#endif
{
	(void)Pk; (void)Sk; (void)Rk; (void)samplesK; (void)pathStackK; (void)countersK; (void)jobCounterK;   // read through RL_ARGS() where a part of the loop needs them (k_trace)
	RL_TEX_PROLOGUE(Sk);
	RL_MATH_PROLOGUE();
	constexpr int PP = 64 * K;
	static_assert(LSTACK <= STACK, "the LDS part cannot exceed the stack");
	__shared__ int s_stack[LSTACK * RL_BLOCK];
	int ovfStore[LSTACK < STACK ? STACK - LSTACK : 1];
	int* ovf = ovfStore;
	__shared__ float s_pool[RL_BLOCK / 64][PoolOcc<LSTACK, PRIMS, K>::kFields][PP];
	__shared__ unsigned char s_free[RL_BLOCK / 64][PP];
	// the 8-wide walk: s_perm[oct * 256 + y] = the byte y with every bit b moved to bit b XOR oct (slot order -> visiting order of a ray of octant oct)
	// ... and the top of that tree: its first RL_TOP8_NODES nodes (rl_device.h), five 16-byte rows each
	__shared__ uint4 s_top[(WIDE == 3 && RL_TOP8_NODES > 0) ? RL_TOP8_NODES * 5 : 1];
	__shared__ unsigned char s_perm[WIDE == 3 ? 8 * 256 : 1];
	if constexpr (WIDE == 3) {
#if RL_TOP8_NODES > 0
		{
			RL_ARGS();
			const uint32_t rows = (uint32_t)(S.numNodes8 < RL_TOP8_NODES ? S.numNodes8 : RL_TOP8_NODES) * 5u;
			for (uint32_t i = threadIdx.x; i < (uint32_t)RL_TOP8_NODES * 5u; i += RL_BLOCK) s_top[i] = i < rows ? GLoadU4(S.nodes8, (int)i) : make_uint4(0u, 0u, 0u, 0u);
		}
#endif
		for (uint32_t i = threadIdx.x; i < 8u * 256u; i += RL_BLOCK) {
			const uint32_t m = i >> 8, y = i & 255u;
			uint32_t r = 0;
			for (uint32_t bb = 0; bb < 8u; ++bb) if ((y >> bb) & 1u) r |= 1u << (bb ^ m);
			s_perm[i] = (unsigned char)r;
		}
		__syncthreads();
	}
	constexpr int G8 = LSTACK / 2, GMAX8 = STACK / 2;   // groups in the LDS part of the stack, groups in all

	int* stk = s_stack + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	float (*pool)[PP] = s_pool[wave];
	unsigned char* freeList = s_free[wave];
	uint32_t numSlots;
	JobSource js;
	{ RL_ARGS(); numSlots = P.numLocalCells * 64u; js = JobSourceInit(P); }
	const unsigned long long laneLt = (1ull << lane) - 1ull;
	// path-stack column of home slot p: consecutive lanes -> consecutive columns
	const uint32_t homeBase = blockIdx.x * (RL_BLOCK * K) + threadIdx.x;

	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	// home-lane registers of slot p*64 + lane
	unsigned long long stRng[K];
	uint32_t stOut[K];
	int stDepth[K];
	bool stActive[K];
	#pragma unroll
	for (int p = 0; p < K; ++p) { stRng[p] = 0; stOut[p] = 0; stDepth[p] = 0; stActive[p] = false; pool[F_TRI][p * 64 + lane] = __int_as_float(Q_EMPTY); }
	// (Round 2 gave every wave its first chunk without an atomic, because 4096 waves asking ONE counter at the same instant stood in line for ~45 us; with a
	// head per XCD the line is an eighth as long and the first chunk comes from the wave's own band like every other.)
	uint32_t chunkNext = 0, chunkEnd = 0;
	bool globalDone = false, exhausted = false;   // wave-uniform
#ifdef RL_DIAG_TIMELINE
	const uint32_t gtid = blockIdx.x * RL_BLOCK + threadIdx.x;
#endif
	RL_TIMELINE(0);
	uint32_t surviveQ8 = 256u;                    // share of freshly generated camera samples that reached a pool slot, x 256 (wave-uniform)
	// traversal state of the ray this lane is tracing; survives trips (a straggler keeps going while the rest of the pool is shaded)
	// A lane without a ray has T.cur == IDLE (no node index, not negative like a leaf reference): "busy", "at an inner node", "at a leaf" are then ONE integer
	// compare each, and a wave vote on a compare is that compare's lane mask.  (A vote on a bool that is not a compare -- `busy && T.cur >= 0` -- makes the
	// compiler write the bool out as 0 / 1 and compare it with zero again: v_cndmask + v_cmp_ne per vote, four votes per traversal step.)
	constexpr int IDLE = 0x7fffffff;
	int mySlot = 0;
	Trav T;
	T.o = T.d = T.inv = v3s(0.0f); T.rayTime = 0.0f; T.nx = T.ny = T.nz = T.anyhit = false;
	T.best.t = INFINITY; T.best.a = T.best.b = 0.0f; T.best.tri = -1; T.cur = IDLE; T.sp = 0; T.leafI = 0;
	T.gx = T.gy = T.tx = T.ty = T.tz = T.oct = 0u; T.m8x = T.m8y = T.m8z = 0u;
#ifdef RL_DIAG_STAMPS
	unsigned long long stampAcc[4] = { 0, 0, 0, 0 };
	{ RL_ARGS(); c.diag = counters; }
	unsigned long long stampLast = __builtin_amdgcn_s_memtime();
	#define RL_PSTAMP(k) { __builtin_amdgcn_sched_barrier(0); const unsigned long long now_ = __builtin_amdgcn_s_memtime(); stampAcc[k] += now_ - stampLast; stampLast = now_; __builtin_amdgcn_sched_barrier(0); }
#else
	#define RL_PSTAMP(k)
#endif

#ifdef RL_POOL_WATCHDOG
	uint32_t wdSteps = 0, wdTrips = 0; bool wdAbort = false;
#endif
	for (;;) {
#ifdef RL_POOL_WATCHDOG
		if (++wdTrips > 20000u || Ballot(wdAbort) != 0ull) {
			uint32_t nAct = 0, nEmpty = 0, nQ = 0, nH = 0, nPend = 0, nRes = 0;
			for (int p = 0; p < K; ++p) {
				const int q = __float_as_int(pool[F_TRI][p * 64 + (int)lane]);
				nAct += (uint32_t)__popcll(Ballot(stActive[p]));
				nEmpty += (uint32_t)__popcll(Ballot(stActive[p] && q == Q_EMPTY));
				nQ += (uint32_t)__popcll(Ballot(stActive[p] && (q == Q_CLOSEST || q == Q_SHADOW)));
				nH += (uint32_t)__popcll(Ballot(stActive[p] && q >= 0));
				nPend += (uint32_t)__popcll(Ballot(stActive[p] && (q == Q_PENDING || q == Q_PENDING_SHADOW)));
				nRes += (uint32_t)__popcll(Ballot(stActive[p] && (q == Q_MISS || q == Q_CLEAR || q == Q_OCCLUDED)));
			}
			if (lane == 0) {
				RL_ARGS();
				atomicAdd(&counters[CNT_COUNT + 21], 1ull);
				atomicAdd(&counters[CNT_COUNT + 4], (unsigned long long)nAct); atomicAdd(&counters[CNT_COUNT + 5], (unsigned long long)nEmpty);
				atomicAdd(&counters[CNT_COUNT + 6], (unsigned long long)nQ); atomicAdd(&counters[CNT_COUNT + 7], (unsigned long long)nH);
				atomicAdd(&counters[CNT_COUNT + 8], (unsigned long long)nPend); atomicAdd(&counters[CNT_COUNT + 9], (unsigned long long)nRes);
				atomicAdd(&counters[CNT_COUNT + 10], (unsigned long long)(exhausted ? 1 : 0)); atomicAdd(&counters[CNT_COUNT + 11], (unsigned long long)__popcll(Ballot(T.cur != IDLE)));
			}
			break;
		}
#endif
		// ---- refill: deal new camera samples to the free slots (wave64 ballot + prefix ranks) ----
		if (!exhausted) {
			RL_ARGS();
			uint32_t pos[K];
			uint32_t nFree = 0;
			#pragma unroll
			for (int p = 0; p < K; ++p) {
				const bool fr = !stActive[p];
				const unsigned long long m = Ballot(fr);
				pos[p] = fr ? nFree + (uint32_t)__popcll(m & laneLt) : 0xffffffffu;
				if (fr) freeList[pos[p]] = (unsigned char)(p * 64 + (int)lane);
				nFree += (uint32_t)__popcll(m);
			}
			WaveLdsSync();
			uint32_t filled = 0;
			for (int round = 0; round < RL_REFILL_ROUNDS && filled < nFree; ++round) {
				RL_WSTEP(6);   // (level-2 diagnostic build: refill rounds, wave level -- tools/dynamic_mix.py)
				if (chunkNext >= chunkEnd && !globalDone) {
					uint32_t base = 0, bend = 0;
					// (a chunk shared by the workgroup's waves in 64-job batches, as in the leaf-list kernel, was measured here too: 44.5 ms against 43.9)
					if (!TakeJobs(P, jobCounter, js, P.jobChunk, lane, base, bend)) { globalDone = true; RL_TIMELINE(1); }
					else { chunkNext = base; chunkEnd = bend; }
				}
				const uint32_t avail = chunkEnd - chunkNext;
				if (avail == 0) { exhausted = true; break; }
				// How many camera samples to generate this round.  A sample that misses the scene's root box is finished right here and
				// fills no slot; where most do (a camera outside the model: 90 % in the configs[2] stand-in) asking for exactly as many
				// samples as there are free slots fills a tenth of them per round.  So the round asks for more -- free slots / the share
				// that survived lately -- and, if more survive than fit, keeps the first `room` survivors and hands the jobs behind the
				// last one kept back to the queue (chunkNext only advances past the lanes that were committed: the same jobs come
				// round again, same pixel, same stream).  Nothing is written or counted for a lane before it is committed.
				const uint32_t room = nFree - filled;
				uint32_t want = room;
				if (surviveQ8 < 230u) want = min(64u, (room * 256u) / max(24u, surviveQ8 + (surviveQ8 >> 3)));   // a little under 1 / survival rate
				const uint32_t take = min(min(64u, max(room, want)), avail);
				bool alive = false, quick = false;   // quick: decided by the root test (sample written at commit)
				V3 o = v3s(0.0f), d = v3s(0.0f);
				float rayTime = 0.0f;
				Rng g; g.s.state = 0;
				uint32_t outIndex = 0;
				if (lane < take) {
#if RL_VIEWS_TWIN
					RL_VIEWS();
					uint32_t view;   // (per lane: the refill's jobs may span two (cell, sample) groups, of two views)
					const JobPixel j = DecodeJobViews(P, VW, chunkNext + lane, view);
#else
					const JobPixel j = DecodeJob(P, chunkNext + lane);
#endif
					if (j.valid) {
						// GenerateCell body, reference render/renderer.cc:232-239
						const uint32_t sidx = P.sampleBegin + j.sample;
						g.s = raylib_rng_begin_mixed(P.seedMixed, j.y * P.width + j.x, sidx);
						float u, v;
						PixelUV(P, j.x, j.y, sidx, g, u, v);
#if RL_VIEWS_TWIN
						CameraRay(LoadViewCamera(VW, view), u, v, g, o, d, rayTime);
#else
						CameraRay(P.camera, u, v, g, o, d, rayTime);
#endif
						outIndex = j.sample * numSlots + j.slot;
						alive = true;
						if (P.maxPathLength <= 0) { alive = false; quick = true; }   // renderer.cc:120-123
						else if (RootMiss(S, o, d, P.rayTMin)) {
							// cannot hit anything: sky lookup plus (with a sun) one occlusion query that may be decided at the root too
							const bool sunQuick = !S.hasSun || RootMiss(S, o, -ld3(S.sunDirection), P.rayTMin);
							if (sunQuick) { alive = false; quick = true; }
						}
					}
				}
				unsigned long long am = Ballot(alive);
				uint32_t n = (uint32_t)__popcll(am);
				uint32_t commit = take;                    // lanes [0, commit) are this round's samples
				if (n > room) {
					// the lane of the (room + 1)-th survivor: everything from there on goes back to the queue
					const unsigned long long over = Ballot(alive && (uint32_t)__popcll(am & laneLt) == room);
					commit = (uint32_t)__ffsll((long long)over) - 1u;
					if (lane >= commit) { alive = false; quick = false; }
					am = Ballot(alive);
					n = room;
				}
				{   // survival rate of the committed samples, 8-bit fixed point, smoothed over the last few rounds
					const uint32_t rate = commit ? (n * 256u) / commit : 256u;
					surviveQ8 = (surviveQ8 * 3u + rate + 2u) >> 2;
				}
				if (lane < commit && (alive || quick)) c.samples++;
				if (quick) {
					if (P.maxPathLength <= 0) samples[outIndex] = make_sample(0.0f, 0.0f, 0.0f);
					else {
						c.rays++; c.nodes++;
						V3 L = MissSky(S, R, d, c);
						if (S.hasSun) { c.rays++; c.nodes++; L = L + ld3(S.sunIlluminance); }
						samples[outIndex] = make_sample(L.x, L.y, L.z);
					}
				}
				chunkNext += commit;
				if (n == 0) continue;
				if (alive) {
					// the r-th surviving ray goes to the (filled + r)-th free slot; the fields a traversal fills in later carry
					// the RNG state and the output index to the slot's home lane
					const int f = (int)freeList[filled + (uint32_t)__popcll(am & laneLt)];
					pool[F_OX][f] = o.x; pool[F_OY][f] = o.y; pool[F_OZ][f] = o.z;
					pool[F_DX][f] = d.x; pool[F_DY][f] = d.y; pool[F_DZ][f] = d.z;
					if (PRIMS) pool[F_TIME][f] = rayTime;
					pool[F_TRI][f] = __int_as_float(Q_CLOSEST);
					pool[F_T][f] = __int_as_float((int)(uint32_t)(g.s.state & 0xffffffffull));
					pool[F_A][f] = __int_as_float((int)(uint32_t)(g.s.state >> 32));
					pool[F_B][f] = __int_as_float((int)outIndex);
				}
				WaveLdsSync();
				#pragma unroll
				for (int p = 0; p < K; ++p) {
					if (pos[p] >= filled && pos[p] < filled + n) {
						const int slot = p * 64 + (int)lane;
						stRng[p] = (unsigned long long)(uint32_t)__float_as_int(pool[F_T][slot]) | ((unsigned long long)(uint32_t)__float_as_int(pool[F_A][slot]) << 32);
						stOut[p] = (uint32_t)__float_as_int(pool[F_B][slot]);
						stDepth[p] = 0;
						stActive[p] = true;
					}
				}
				filled += n;
			}
		}
		bool anyActive = false;
		#pragma unroll
		for (int p = 0; p < K; ++p) anyActive = anyActive || stActive[p];
		if (Ballot(anyActive) == 0ull) {
			if (exhausted) break;
			continue;
		}
		if (lane == 0) c.trips++;
		RL_PSTAMP(0);

		// ---- traversal phase: every waiting query of the pool; a lane takes the next slot whenever its ray is finished ----
		{
			RL_ARGS();
			const float tMinC = __builtin_canonicalizef(P.rayTMin);   // known to be canonical: the box tests' max chains start from it without a v_max x, x per step
#if RL_POOL_NODEPTR_VGPR
			// the wide nodes' base address in a VGPR pair for the phase: as one of the loop's many uniform values it would be spilled to a VGPR's lanes and
			// read back (two v_readlane, 4 issue cycles each) at every traversal step
			DSceneView St = S;
			if constexpr (WIDE == 3) { }   // (the 8-wide node's rows are loaded from an SGPR base plus a 32-bit offset: NodeStep8)
			else { const DNode4Q* pn = S.nodes4; asm volatile("" : "+v"(pn)); St.nodes4 = pn; }
#else
			const DSceneView& St = S;
#endif
			WaveLdsSync();
			uint32_t nextSlot = 0;
			uint32_t finished = 0;      // rays completed in this phase (wave-uniform)
			for (;;) {
				if (nextSlot < (uint32_t)PP) {
					const unsigned long long idle = Ballot(T.cur == IDLE);
					const uint32_t slot = nextSlot + (uint32_t)__popcll(idle & laneLt);
					if (T.cur == IDLE && slot < (uint32_t)PP) {
						const int q = __float_as_int(pool[F_TRI][slot]);
						if (q == Q_CLOSEST || q == Q_SHADOW) {
							T.o = v3(pool[F_OX][slot], pool[F_OY][slot], pool[F_OZ][slot]);
							T.anyhit = (q == Q_SHADOW);
							T.d = T.anyhit ? -ld3(S.sunDirection) : v3(pool[F_DX][slot], pool[F_DY][slot], pool[F_DZ][slot]);
							T.rayTime = PRIMS ? pool[F_TIME][slot] : 0.0f;
							T.inv = v3(FastRcp(T.d.x), FastRcp(T.d.y), FastRcp(T.d.z));
							if (WIDE) T.inv = ClampInv(T.inv);   // only the grid nodes' fused plane arithmetic wants finite reciprocals; Slab() relies on +-inf / NaN
							T.nx = T.inv.x < 0.0f; T.ny = T.inv.y < 0.0f; T.nz = T.inv.z < 0.0f;
							T.best.t = INFINITY; T.best.tri = -1; T.best.a = 0.0f; T.best.b = 0.0f;
							T.cur = 0; T.sp = 0; T.leafI = 0;
							if constexpr (WIDE == 3) {
								// the root as a group of one: base 0, imask 1, its bit at the visiting position of slot 0
								RaySetup8(T);
								T.gx = 0u; T.gy = (1u << (24u + T.oct)) | 1u; T.tx = T.ty = T.tz = 0u;
							}
							mySlot = (int)slot;
							pool[F_TRI][slot] = __int_as_float(T.anyhit ? Q_PENDING_SHADOW : Q_PENDING);
							c.rays++;
						}
					}
					nextSlot += (uint32_t)__popcll(idle);
				}
				const int nBusy = (int)__popcll(Ballot(T.cur != IDLE));
				if (nBusy == 0) {
					if (nextSlot >= (uint32_t)PP) break;
					continue;
				}
				// all queries handed out and only a few long rays left: shade what is there, the stragglers go on next trip
				const int cutAt = exhausted ? RL_POOL_CUT_EXH : RL_POOL_CUT;
				if (nextSlot >= (uint32_t)PP && nBusy <= cutAt && finished > 0) break;
				// one step for the larger (cost-weighted) party, lanes at inner nodes or lanes at leaves, until enough lanes
				// have finished to make a fetch worth it
				int nb;
				do {
					const bool atNode = (uint32_t)T.cur < (uint32_t)IDLE, atLeaf = T.cur < 0;
					const int nN = (int)__popcll(Ballot(atNode)), nL = (int)__popcll(Ballot(atLeaf));
					bool fin = false;
					const bool nodeTurn = nN * (WIDE == 3 ? RL_POOL_WNODE8 : WIDE ? RL_POOL_WNODE4 : RL_POOL_WNODE) >= nL * (WIDE == 3 ? RL_POOL_WLEAF8 : WIDE ? RL_POOL_WLEAF4 : RL_POOL_WLEAF);
					if constexpr (WIDE == 3) {
#if RL_POOL_BOTH8
						// both parties every turn: a lane at a node takes its node step, a lane at a leaf its triangle step (the wave runs either part only if some lane needs it)
						(void)nodeTurn;
						if (atNode) fin = NodeStep8(St, T, tMinC, stk, ovf, c, s_perm, s_top, G8, GMAX8);
						else if (atLeaf) fin = LeafStep8<PRIMS>(S, T, P.rayTMin, stk, ovf, c, G8);
#else
						if (nodeTurn) { if (atNode) fin = NodeStep8(St, T, tMinC, stk, ovf, c, s_perm, s_top, G8, GMAX8); }
						else { if (atLeaf) fin = LeafStep8<PRIMS>(S, T, P.rayTMin, stk, ovf, c, G8); }
#endif
					} else {
						if (nodeTurn) { if (atNode) fin = WIDE ? NodeStep4<LSTACK, STACK>(St, T, tMinC, stk, ovf, c) : NodeStep<LSTACK, STACK>(S, T, tMinC, stk, ovf, c); }
						else { if (atLeaf) fin = LeafStep<LSTACK, STACK, PRIMS>(S, T, P.rayTMin, stk, ovf, c); }
					}
					if (fin) {
						const bool hit = T.best.tri >= 0;
						int q = T.best.tri;
						if (T.anyhit) q = hit ? Q_OCCLUDED : Q_CLEAR;
						else if (!hit) q = Q_MISS;
						pool[F_T][mySlot] = T.best.t; pool[F_TRI][mySlot] = __int_as_float(q);
						pool[F_A][mySlot] = T.best.a; pool[F_B][mySlot] = T.best.b;
						T.cur = IDLE;
					}
#ifdef RL_POOL_WATCHDOG
					if (++wdSteps > 400000u) { if (lane == 0) atomicAdd(&counters[CNT_COUNT + 20], 1ull); T.cur = IDLE; wdAbort = true; }
#endif
					nb = (int)__popcll(Ballot(T.cur != IDLE));
					finished += (uint32_t)(nN + nL - nb);   // whoever was busy and is not any more has finished its ray
				} while (nb > (nextSlot < (uint32_t)PP ? RL_POOL_KEEP : (finished > 0 ? cutAt : 0)));
			}
			WaveLdsSync();
		}
		RL_PSTAMP(1);

		// ---- shading (TraceScene after the accel->Hit call, reference render/renderer.cc:129-208) ----
		// (1) the cheap outcomes are finished by the slot's home lane: a miss runs the sky lookup and (with a sun) turns
		//     into an occlusion query, a returned occlusion query ends the path.  Hits are only LISTED.
		uint32_t nHit = 0;
		uint32_t hitIdx[K];
		{
		RL_ARGS();
		#pragma unroll
		for (int p = 0; p < K; ++p) {
			const int slot = p * 64 + (int)lane;
			const int q = __float_as_int(pool[F_TRI][slot]);
			const bool isHit = stActive[p] && q >= 0;
			if (stActive[p] && (q == Q_MISS || q == Q_CLEAR || q == Q_OCCLUDED)) {
				const V3 d = v3(pool[F_DX][slot], pool[F_DY][slot], pool[F_DZ][slot]);
				bool done = true;
				V3 L;
				if (q == Q_MISS) {
					L = MissSky(S, R, d, c);
					if (S.hasSun) {
						// the sky part waits in the direction fields (the sun query brings its own direction)
						pool[F_DX][slot] = L.x; pool[F_DY][slot] = L.y; pool[F_DZ][slot] = L.z;
						pool[F_TRI][slot] = __int_as_float(Q_SHADOW);
						done = false;
					}
				} else {
					L = d;
					if (q == Q_CLEAR) L = L + ld3(S.sunIlluminance);
				}
				if (done) {
					L = FoldPath(pathStack, P.stackStride, homeBase + (uint32_t)p * RL_BLOCK, stDepth[p], L);
					samples[stOut[p]] = make_sample(L.x, L.y, L.z);
					stActive[p] = false;
					pool[F_TRI][slot] = __int_as_float(Q_EMPTY);
				}
			}
			const unsigned long long hm = Ballot(isHit);
			hitIdx[p] = isHit ? nHit + (uint32_t)__popcll(hm & laneLt) : 0xffffffffu;
			if (isHit) freeList[hitIdx[p]] = (unsigned char)slot;
			nHit += (uint32_t)__popcll(hm);
		}
		}
		WaveLdsSync();
		// (2) hits are shaded 64 at a time by whichever lane: the expensive material code always runs with a full wave.
		//     A remainder below 64 waits in its slots for the next trip's hits (until the job queue is empty).
		//     The path registers come from the home lane by ds_bpermute and return through the slot's hit fields.
		uint32_t shadedEnd = 0;
		for (;;) {
			RL_ARGS();
			if (shadedEnd >= nHit) break;
			if (nHit - shadedEnd < (uint32_t)RL_POOL_SHADE_MIN && !exhausted) break;   // once the job queue is empty no refill will top the list up: waiting only stretches the tail
#ifdef RL_POOL_WATCHDOG
			if (++wdSteps > 400000u) { if (lane == 0) atomicAdd(&counters[CNT_COUNT + 20], 1ull); wdAbort = true; break; }
#endif
			RL_WSTEP(7);   // (level-2 diagnostic build: rounds of hit shading, wave level)
			const uint32_t idx = shadedEnd + lane;
			const bool on = idx < nHit;
			const int slot = on ? (int)freeList[idx] : 0;
			const int h = slot & 63, pp = slot >> 6;
			uint32_t rngLo = 0, rngHi = 0, outIndex = 0; int depth = 0;
			#pragma unroll
			for (int k = 0; k < K; ++k) {
				const uint32_t a0 = (uint32_t)__shfl((int)(uint32_t)(stRng[k] & 0xffffffffull), h);
				const uint32_t a1 = (uint32_t)__shfl((int)(uint32_t)(stRng[k] >> 32), h);
				const uint32_t a2 = (uint32_t)__shfl((int)stOut[k], h);
				const int a3 = __shfl(stDepth[k], h);
				if (pp == k) { rngLo = a0; rngHi = a1; outIndex = a2; depth = a3; }
			}
			if (on) {
				const V3 o = v3(pool[F_OX][slot], pool[F_OY][slot], pool[F_OZ][slot]);
				const V3 d = v3(pool[F_DX][slot], pool[F_DY][slot], pool[F_DZ][slot]);
				HitRec hr; hr.t = pool[F_T][slot]; hr.tri = __float_as_int(pool[F_TRI][slot]); hr.a = pool[F_A][slot]; hr.b = pool[F_B][slot];
				const uint32_t home = blockIdx.x * (RL_BLOCK * K) + (uint32_t)pp * RL_BLOCK + wave * 64u + (uint32_t)h;
				Rng g; g.s.state = (unsigned long long)rngLo | ((unsigned long long)rngHi << 32);
				Surf sf;
				const Mat m = LoadMat(S, BuildSurface<PRIMS>(S, o, d, hr, sf, true, c));
				V3 refl = v3s(0.0f), outD = v3s(0.0f);
				float pdf = 0.0f, sp = 0.0f;
				const bool scattered = Scatter(S, m, d, sf, g, c, refl, outD, pdf, sp);
				const V3 E = Emitted(S, m, sf, c);
				bool done = false;
				V3 L = v3s(0.0f);
				if (scattered && pdf > 0.0f) {
					float4* rec = (float4*)pathStack + ((size_t)depth * P.stackStride + home) * 2u;
					rec[0] = make_float4(refl.x, refl.y, refl.z, sp);
					rec[1] = make_float4(pdf, E.x, E.y, E.z);
					depth++;
					if (depth >= P.maxPathLength) done = true;   // the next TraceScene returns 0 at once (renderer.cc:120-123)
					else {
						pool[F_OX][slot] = sf.p.x; pool[F_OY][slot] = sf.p.y; pool[F_OZ][slot] = sf.p.z;
						pool[F_DX][slot] = outD.x; pool[F_DY][slot] = outD.y; pool[F_DZ][slot] = outD.z;
						pool[F_TRI][slot] = __int_as_float(Q_CLOSEST);
					}
				} else {
					L = v3s(0.0f) + E;                            // radiance(0) += Emitted, renderer.cc:137,151
					done = true;
				}
				if (done) {
					L = FoldPath(pathStack, P.stackStride, home, depth, L);
					samples[outIndex] = make_sample(L.x, L.y, L.z);
					pool[F_TRI][slot] = __int_as_float(Q_EMPTY);
				}
				// back to the home lane: RNG state and depth (negative = the path has ended)
				pool[F_T][slot] = __int_as_float((int)(uint32_t)(g.s.state & 0xffffffffull));
				pool[F_A][slot] = __int_as_float((int)(uint32_t)(g.s.state >> 32));
				pool[F_B][slot] = __int_as_float(done ? -1 : depth);
			}
			shadedEnd += 64u;
		}
		WaveLdsSync();
		// (3) the home lanes take their registers back
		#pragma unroll
		for (int p = 0; p < K; ++p) {
			if (hitIdx[p] < shadedEnd) {
				const int slot = p * 64 + (int)lane;
				stRng[p] = (unsigned long long)(uint32_t)__float_as_int(pool[F_T][slot]) | ((unsigned long long)(uint32_t)__float_as_int(pool[F_A][slot]) << 32);
				const int dd = __float_as_int(pool[F_B][slot]);
				if (dd < 0) stActive[p] = false; else stDepth[p] = dd;
			}
		}
		RL_PSTAMP(2);
	}

	RL_ARGS();
#ifdef RL_DIAG_STAMPS
	if (lane == 0) for (int k = 0; k < 4; ++k) { atomicAdd(&counters[CNT_COUNT + k], stampAcc[k]); atomicAdd(&counters[CNT_COUNT + 12 + k], c.tAcc[k]); }
#endif
	RL_TIMELINE(2);
	uint32_t vals[CNT_COUNT] = { c.rays, c.nodes, c.tris, c.shaded, c.texels, c.samples, c.trips };
	for (int k = 0; k < CNT_COUNT; ++k) {
		unsigned long long v = vals[k];
		for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
		if (lane == 0 && v) atomicAdd(&counters[k], v);
	}
}
