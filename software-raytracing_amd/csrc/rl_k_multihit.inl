// k_query_all: ordered multi-hit ray queries on a finalized scene (include/raylib_amd.h RaylibAMD_TraceRaysAll, statements M1 to M5): the first maxHits
// accepted triangles of each ray in (t, slot) order and, with COUNT, how many the whole interval holds.  rl_multihit.hip includes this file behind
// rl_k_query.inl -- NextUpF, QueryTMin and k_query's schedule are that file's -- and instantiates the kernels; every other unit stays the code it is.
//
// The walks are written here on the shared pieces: Slab, DecodeLeaf and LoadTri for the binary tree (Traverse's while-while loop), NodeStep8 and the stack of
// groups for the 8-wide tree (LeafStep8's triangle pick), one ray per lane, RL_QUERY_CHUNK rays per atomic, per-lane refill between steps on the 8-wide tree.
// The triangle test is RL_TRIANGLE_TEST, unchanged, with a HitRec as the bound:
//   * while the list is not full, and always with COUNT, the bound is {NextUpF(tMax), -1}: every accepted t <= tMax passes, no tie clause can fire;
//   * with the list full and no count wanted, the bound is the list's last entry, so the macro's "t < best.t || (t == best.t && slot < best.tri)" is the
//     lexicographic test against the K-th key, and NodeStep8 / Slab cull against its t as they cull against a closest hit's.
// When the macro fires, the key is inserted, the count bumped and the bound restored.  Every slot sits in exactly one leaf (ValidateBVH, ValidateBVH8): no
// key comes twice.  The cull is safe for ties as it is for CLOSEST's tie rule: an accepted hit has t * RL_CANDIDATE_SLACK >= the entry into its own box, which
// lies inside every box around it, and the boxes are widened by more than that.
//
// The per-lane list lives in LDS, interleaved by lane like the traversal stack -- entry k's t at word (2k) * RL_BLOCK + lane, its slot one row further -- and the
// launch sizes it by maxHits (dynamic LDS: 2 KB per workgroup and entry), so that a runtime maxHits indexes no register array.  The barycentrics are not kept:
// the winners' are rebuilt at store time with the test's own operations on the same operands (one record load per winner), which halves the list.

// the test of one triangle: true when it was accepted, with `best` = {t, b1, b2, slot} of it
__device__ __forceinline__ bool MultiHitTest(const DSceneView& S, const Tri& TT, int slot, V3 o, V3 d, V3 inv /* exact 1/d */, float tMin, HitRec& best, bool alpha, Counters& c)
{
	RL_TRIANGLE_TEST(S, TT, slot, o, d, tMin, best, alpha, OwnBoxPass(TT.v0, TT.v1, TT.v2, o, inv, tMin, t), true, c, RL_NESTED)
	return false;
}

// One lane's list: K = maxHits entries of capacity, n of them held, sorted by (t, slot) ascending.
struct HitList {
	uint32_t* at;        // this lane's column
	uint32_t K, n, total;
	float bound0;        // NextUpF(tMax)
	__device__ __forceinline__ float T(uint32_t k) const { return __uint_as_float(at[(2u * k) * RL_BLOCK]); }
	__device__ __forceinline__ int Slot(uint32_t k) const { return (int)at[(2u * k + 1u) * RL_BLOCK]; }
	__device__ __forceinline__ void Set(uint32_t k, float t, int slot) { at[(2u * k) * RL_BLOCK] = __float_as_uint(t); at[(2u * k + 1u) * RL_BLOCK] = (uint32_t)slot; }
	__device__ __forceinline__ void Begin(float tMax) { n = 0u; total = 0u; bound0 = NextUpF(tMax); }
	template <bool COUNT> __device__ __forceinline__ void Bound(HitRec& best) const
	{
		if (!COUNT && n == K) { best.t = T(K - 1u); best.tri = Slot(K - 1u); }
		else { best.t = bound0; best.tri = -1; }
		best.a = 0.0f; best.b = 0.0f;
	}
	// behind an accepted test: `best` holds the hit.  Without COUNT a full list's bound has let through only what belongs in front of its last entry.
	template <bool COUNT> __device__ __forceinline__ void Accept(HitRec& best)
	{
		const float t = best.t; const int slot = best.tri;
		++total;
		bool take = true;
		if (COUNT && n == K) { const float tl = T(K - 1u); take = t < tl || (t == tl && slot < Slot(K - 1u)); }
		if (take) {
			uint32_t k = n < K ? n : K - 1u;   // the entry that is free, or the last one, which drops out
			while (k > 0u) {
				const float tp = T(k - 1u); const int sp = Slot(k - 1u);
				if (tp < t || (tp == t && sp < slot)) break;
				Set(k, tp, sp);
				--k;
			}
			Set(k, t, slot);
			if (n < K) ++n;
		}
		Bound<COUNT>(best);
	}
};

// the records of one finished ray: the list's entries with their barycentrics rebuilt as the test computed them, then miss records; the count
__device__ __forceinline__ void MultiHitStore(const DSceneView& S, V3 o, V3 d, const HitList& L, uint32_t i, float4* __restrict__ outHits, uint32_t* __restrict__ outCount,
                                              const int32_t* __restrict__ slotIndex)
{
	float4* row = outHits + (size_t)i * L.K;   // (64-bit: n * maxHits may reach 2^31 - 1)
	for (uint32_t k = 0; k < L.K; ++k) {
		float4 r = make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f);
		if (k < L.n) {
			const float t = L.T(k); const int slot = L.Slot(k);
			const Tri TT = LoadTri(S, slot);
			const V3 p_ = o + t * d;
			const V3 w_ = p_ - TT.v0;
			const float wv_ = dot(w_, TT.v), wu_ = dot(w_, TT.u);
			float pa_, pb_;
			(void)Barycentric(S.fastBary != 0, TT.uv * wv_ - TT.vv * wu_, TT.uv * wu_ - TT.uu * wv_, TT.denom, TT.rden, pa_, pb_);
			r = make_float4(t, __int_as_float(slotIndex ? slotIndex[slot] : slot), pa_, pb_);
		}
		row[k] = r;
	}
	if (outCount) outCount[i] = L.total;
}

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int STACK, bool COUNT>
__global__ void __launch_bounds__(RL_BLOCK)
k_query_all(const DSceneView S, const float4* __restrict__ rays, uint32_t n, uint32_t maxHits, float4* __restrict__ outHits, uint32_t* __restrict__ outCount,
            const int32_t* __restrict__ slotIndex, unsigned int* __restrict__ rayCounter, unsigned long long* __restrict__ counters)
{
	static_assert(TREE == 2 || TREE == 8, "tree");
	RL_TEX_PROLOGUE(S);
	RL_MATH_PROLOGUE();
	__shared__ int s_stack[(TREE == 8 ? RL_POOL8_LSTACK : STACK) * RL_BLOCK];
	extern __shared__ uint32_t s_list[];   // 2 * maxHits * RL_BLOCK words (the launch's dynamic LDS)
	int* stk = s_stack + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	HitList L; L.at = s_list + threadIdx.x; L.K = maxHits; L.n = 0u; L.total = 0u; L.bound0 = 0.0f;
	if constexpr (TREE == 2) {
		for (;;) {
			uint32_t base = 0u;
			if (lane == 0u) base = atomicAdd(rayCounter, RL_QUERY_CHUNK);
			base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
			if (base >= n) break;
			for (uint32_t k = 0; k < RL_QUERY_CHUNK; k += 64u) {
				const uint32_t i = base + k + lane;
				if (i >= n) continue;
				const float4* rp = rays + 2u * (size_t)i;
				const float4 r0 = GLoadF4(rp, 0), r1 = GLoadF4(rp, 1);
				const V3 o = v3(r0.x, r0.y, r0.z), d = v3(r1.x, r1.y, r1.z);
				const float tMin = QueryTMin(r0.w);
				// Traverse's walk (rl_dev_walk.h) with the list behind its triangle test
				c.rays++;
				const V3 inv = ExactInv(d);
				const bool nx = inv.x < 0.0f, ny = inv.y < 0.0f, nz = inv.z < 0.0f;
				HitRec best;
				L.Begin(r1.w); L.template Bound<COUNT>(best);
				int sp = 0, cur = 0;
				const int DONE = 0x7fffffff;
				for (;;) {
					while (cur >= 0 && cur != DONE) {
						const float4* np = (const float4*)(S.nodes + cur);
						const float4 q0 = np[0], q1 = np[1], q2 = np[2];
						const int4 kk = ((const int4*)np)[3];
						c.nodes++;
						float tl, tr;
						const float tmx = fminf(best.t, FLT_MAX);
						bool hl = Slab(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, o, inv, nx, ny, nz, tMin, tmx, tl);
						bool hr = Slab(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, o, inv, nx, ny, nz, tMin, tmx, tr);
						hl = hl && (kk.x != DNODE_EMPTY);
						hr = hr && (kk.y != DNODE_EMPTY);
						if (hl && hr) {
							const bool leftFirst = tl <= tr;
							const int nearC = leftFirst ? kk.x : kk.y, farC = leftFirst ? kk.y : kk.x;
							if (sp < STACK) { stk[sp * RL_BLOCK] = farC; ++sp; }
							cur = nearC;
						} else if (hl) cur = kk.x;
						else if (hr) cur = kk.y;
						else if (sp == 0) cur = DONE;
						else { --sp; cur = stk[sp * RL_BLOCK]; }
					}
					if (cur == DONE) break;
					{
						const LeafRef F = DecodeLeaf(cur);
						for (int j = 0; j < F.count; ++j) {
							const Tri TT = LoadTri(S, F.first + j);
							c.tris++;
							if (MultiHitTest(S, TT, F.first + j, o, d, inv, tMin, best, F.alpha, c)) L.template Accept<COUNT>(best);
						}
					}
					if (sp == 0) break;
					--sp;
					cur = stk[sp * RL_BLOCK];
				}
				MultiHitStore(S, o, d, L, i, outHits, outCount, slotIndex);
			}
		}
	} else {
		// the 8-wide walk on k_query's schedule: the octant table, the LDS part of the stack of groups, the private rest
		__shared__ unsigned char s_perm[8 * 256];
		for (uint32_t k = threadIdx.x; k < 8u * 256u; k += RL_BLOCK) {
			const uint32_t m = k >> 8, y = k & 255u;
			uint32_t r = 0;
			for (uint32_t bb = 0; bb < 8u; ++bb) if ((y >> bb) & 1u) r |= 1u << (bb ^ m);
			s_perm[k] = (unsigned char)r;
		}
		__syncthreads();
		constexpr int G8 = RL_POOL8_LSTACK / 2, GMAX8 = STACK / 2;
		int ovfStore[STACK - RL_POOL8_LSTACK];
		int* ovf = ovfStore;
		const unsigned long long laneLt = (1ull << lane) - 1ull;
		constexpr uint32_t NONE = 0xffffffffu;
		uint32_t my = NONE;
		float tMin = 0.0f;
		Trav T;
		T.o = T.d = T.inv = v3s(0.0f); T.rayTime = 0.0f; T.nx = T.ny = T.nz = false; T.anyhit = false;
		T.best.t = INFINITY; T.best.a = T.best.b = 0.0f; T.best.tri = -1; T.cur = 0; T.sp = 0; T.leafI = 0;
		T.gx = T.gy = T.tx = T.ty = T.tz = T.oct = 0u; T.m8x = T.m8y = T.m8z = 0u;
		uint32_t next = 0u, end = 0u;
		bool drained = false;
		for (;;) {
			unsigned long long idle = Ballot(my == NONE);
			if (!drained && idle != 0ull && (__popcll(idle) >= RL_QUERY_REFILL || idle == ~0ull)) {
				while (idle != 0ull) {
					if (next >= end) {
						uint32_t b = 0u;
						if (lane == 0u) b = atomicAdd(rayCounter, RL_QUERY_CHUNK);
						b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
						if (b >= n) { drained = true; break; }
						next = b; end = min(b + RL_QUERY_CHUNK, n);
					}
					const uint32_t take = min((uint32_t)__popcll(idle), end - next);
					const uint32_t rank = (uint32_t)__popcll(idle & laneLt);
					if (my == NONE && rank < take) {
						my = next + rank;
						const float4* rp = rays + 2u * (size_t)my;
						const float4 r0 = GLoadF4(rp, 0), r1 = GLoadF4(rp, 1);
						T.o = v3(r0.x, r0.y, r0.z); T.d = v3(r1.x, r1.y, r1.z); tMin = QueryTMin(r0.w);
						T.inv = ClampInv(v3(FastRcp(T.d.x), FastRcp(T.d.y), FastRcp(T.d.z)));
						T.nx = T.inv.x < 0.0f; T.ny = T.inv.y < 0.0f; T.nz = T.inv.z < 0.0f;
						L.Begin(r1.w); L.template Bound<COUNT>(T.best);
						T.cur = 0; T.sp = 0; T.leafI = 0;
						RaySetup8(T);
						T.gx = 0u; T.gy = (1u << (24u + T.oct)) | 1u; T.tx = T.ty = T.tz = 0u;
						c.rays++;
					}
					next += take;
					idle = Ballot(my == NONE);
				}
			}
			if (Ballot(my != NONE) == 0ull) { if (drained) break; continue; }
			if (my != NONE) {
				bool fin;
				if (T.cur >= 0) fin = NodeStep8(S, T, tMin, stk, ovf, c, s_perm, nullptr, G8, GMAX8);
				else {
					// LeafStep8's pick (rl_dev_pool.h): the lowest hit leaf child, its next triangle
					const uint32_t lc = (uint32_t)__ffs((int)(T.ty & 0xffu)) - 1u;
					const uint32_t k = (T.ty >> 8) & 3u;
					const uint32_t nib = (T.tz >> (4u * lc)) & 15u;
					const int slot = (int)(T.tx + (uint32_t)__popc(T.tz & ((1u << (4u * lc)) - 1u)) + k);
					const bool alpha = ((T.ty >> (16u + lc)) & 1u) != 0u;
					if ((nib >> (k + 1u)) != 0u) T.ty += 0x100u;
					else { T.ty &= ~0x300u; T.ty &= T.ty - 1u; }
					c.tris++;
					const Tri TT = LoadTri(S, slot);
					if (MultiHitTest(S, TT, slot, T.o, T.d, ExactInv(T.d), tMin, T.best, alpha, c)) L.template Accept<COUNT>(T.best);
					fin = Next8(T, stk, ovf, G8);
				}
				if (fin) { MultiHitStore(S, T.o, T.d, L, my, outHits, outCount, slotIndex); my = NONE; }
			}
		}
	}
	if (counters) {   // wave reduction, one atomic per wave and counter
		const uint32_t vals[5] = { c.rays, c.nodes, c.tris, c.shaded, c.texels };
		for (int k = 0; k < 5; ++k) {
			unsigned long long v = vals[k];
			for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
			if (lane == 0u && v) atomicAdd(&counters[k], v);
		}
	}
}
