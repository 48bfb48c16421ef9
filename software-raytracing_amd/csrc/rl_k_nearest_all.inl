// k_nearest_all: the K nearest triangles of each point and the count in range (include/raylib_amd.h RaylibAMD_NearestPointsAll, statements K1 to K5).
// rl_nearest.hip includes this file behind rl_k_nearest.inl -- the RL_NEAREST_DIST32 / 64 settings are that file's -- and instantiates the kernels.
//
// The walk is rl_dev_boxwalk.h's point walk, shaped around it as k_nearest is: one point per lane, RL_QUERY_CHUNK points per atomic, the stack and its
// packed distances as this lane's LDS columns, counters reduced per wave.  What differs is the bound and what stands behind the triangle test:
//   * while the list is not full, and always with COUNT, the bound is R2 = maxDist * maxDist: every triangle with D <= R2 passes (K1) and is counted;
//   * with the list full and no count wanted, the bound is the list's last D; a triangle whose D equals it enters only with a lower export index than the
//     last entry (slotIndex, read on ties only, as NearestLeaf reads it).
// A triangle's D is at least its own box's distance, the own box lies in every box around it and N2 is monotone under nesting (rl_nearest.h), so a node or a
// triangle whose box distance exceeds the bound holds nothing that belongs in the set (bound R2) or in front of the list's last entry (bound the last D).
// Every slot sits in exactly one leaf: no key comes twice.  With maxHits == 1 and no count the bound moves as k_nearest<CLOSEST>'s best does, at the same
// triangles, so the walk visits the same records.
//
// The per-lane list lives in dynamic LDS, interleaved by lane as HitList's (rl_k_multihit.inl): entry k's D at word (2k) * RL_BLOCK + lane, its slot one row
// further; 2 KB per workgroup and entry.  The barycentrics are not kept: the winners' are rebuilt at store time by NearestTriangleE on the same operands (no
// FMA, the same bits), one record load per winner.

// One lane's list: K = maxHits entries of capacity, n of them held, sorted by (D, export index) ascending; total: the triangles the bound has let through.
struct NearestList {
	uint32_t* at;   // this lane's column
	uint32_t K, n, total;
	__device__ __forceinline__ float D(uint32_t k) const { return __uint_as_float(at[(2u * k) * RL_BLOCK]); }
	__device__ __forceinline__ int Slot(uint32_t k) const { return (int)at[(2u * k + 1u) * RL_BLOCK]; }
	__device__ __forceinline__ void Set(uint32_t k, float d, int slot) { at[(2u * k) * RL_BLOCK] = __float_as_uint(d); at[(2u * k + 1u) * RL_BLOCK] = (uint32_t)slot; }
	// A triangle with D <= bound.  Without COUNT a full list's bound has let through only D <= its last D: the tie clause decides the rest.
	template <bool COUNT> __device__ __forceinline__ void Accept(float d, int slot, const int32_t* __restrict__ slotIndex, float& bound)
	{
		++total;
		if (n == K) {
			const float dl = D(K - 1u);
			if (!(d < dl)) {
				if (d != dl) return;
				const int last = Slot(K - 1u);
				if ((slotIndex ? slotIndex[slot] : slot) > (slotIndex ? slotIndex[last] : last)) return;
			}
		}
		uint32_t k = n < K ? n : K - 1u;   // the entry that is free, or the last one, which drops out
		while (k > 0u) {
			const float dp = D(k - 1u); const int sp = Slot(k - 1u);
			if (dp < d || (dp == d && (slotIndex ? slotIndex[sp] : sp) < (slotIndex ? slotIndex[slot] : slot))) break;
			Set(k, dp, sp);
			--k;
		}
		Set(k, d, slot);
		if (n < K) ++n;
		if (!COUNT && n == K) bound = D(K - 1u);
	}
};

// One leaf: `count` triangles from slot `first`, NearestLeaf's tests against the bound.
template <bool COUNT>
__device__ __forceinline__ void NearestLeafAll(const DSceneView& S, const float p[3], int first, int count, float& bound, NearestList& L, const int32_t* __restrict__ slotIndex, uint32_t& tris)
{
	for (int i = 0; i < count; ++i) {
		const int slot = first + i;
		float v0[3], v1[3], v2[3];
		IsectVertices(S, slot, v0, v1, v2);
		++tris;
		const float B = NearestOwnBoxDist2(p, v0, v1, v2);
		if (B > bound) continue;   // D >= B: not in range, and E need not be known
		float b1, b2;
		const float D = NearestTriangleD(NearestTriangleE(p, v0, v1, v2, b1, b2), B);
		if (D > bound) continue;
		L.template Accept<COUNT>(D, slot, slotIndex, bound);
	}
}

// the records of one finished point: the list's entries with their barycentrics rebuilt as the test computed them, then miss records; the count
__device__ __forceinline__ void NearestStoreAll(const DSceneView& S, const float p[3], const NearestList& L, uint32_t i, float4* __restrict__ outHits, uint32_t* __restrict__ outCount,
                                                const int32_t* __restrict__ slotIndex)
{
	float4* row = outHits + (size_t)i * L.K;   // (64-bit: n * maxHits may reach 2^31 - 1)
	for (uint32_t k = 0; k < L.K; ++k) {
		float4 r = make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f);
		if (k < L.n) {
			const int slot = L.Slot(k);
			float v0[3], v1[3], v2[3];
			IsectVertices(S, slot, v0, v1, v2);
			float b1, b2;
			(void)NearestTriangleE(p, v0, v1, v2, b1, b2);
			r = make_float4(L.D(k), __int_as_float(slotIndex ? slotIndex[slot] : slot), b1, b2);
		}
		row[k] = r;   // (the 16-byte record as one store)
	}
	if (outCount) outCount[i] = L.total;
}

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int STACK, bool COUNT>
__global__ void __launch_bounds__(RL_BLOCK)
k_nearest_all(const DSceneView S, const float4* __restrict__ points, uint32_t n, uint32_t maxHits, float4* __restrict__ outHits, uint32_t* __restrict__ outCount,
              const int32_t* __restrict__ slotIndex, unsigned int* __restrict__ pointCounter, unsigned long long* __restrict__ counters)
{
	__shared__ int s_stack[STACK * RL_BLOCK];
	extern __shared__ uint32_t s_list[];   // 2 * maxHits * RL_BLOCK words (the launch's dynamic LDS)
	int* stk = s_stack + threadIdx.x;
	constexpr int DBYTES = STACK <= 32 ? RL_NEAREST_DIST32 : RL_NEAREST_DIST64;
	typedef NearestDist<DBYTES> Dist;
	__shared__ typename Dist::T s_dist[DBYTES != 0 ? STACK * RL_BLOCK : 1];
	typename Dist::T* dstk = s_dist + (DBYTES != 0 ? threadIdx.x : 0u);
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t cPoints = 0u, cNodes = 0u, cTris = 0u;
	NearestList L; L.at = s_list + threadIdx.x; L.K = maxHits; L.n = 0u; L.total = 0u;
	for (;;) {
		const uint32_t base = ClaimChunk(pointCounter, RL_QUERY_CHUNK, lane);
		if (base >= n) break;
		for (uint32_t k = 0; k < RL_QUERY_CHUNK; k += 64u) {
			const uint32_t i = base + k + lane;
			if (i >= n) continue;
			++cPoints;
			const float4 q = GLoadF4(points + (size_t)i, 0);   // (64-bit offset: n may reach 2^31 - 1)
			const float p[3] = { q.x, q.y, q.z };
			float bound = q.w * q.w;   // R2
			L.n = 0u; L.total = 0u;
			// a point that does not take part has the empty set, without a walk (a NaN bound would cull nothing)
			if (NearestTakesPart(q.x, q.y, q.z, q.w) && S.numTriangles > 0)
				PointWalk<TREE, STACK, DBYTES>(S, p, bound, stk, dstk, cNodes,
				                               [&](int first, int count) { NearestLeafAll<COUNT>(S, p, first, count, bound, L, slotIndex, cTris); return false; });
			NearestStoreAll(S, p, L, i, outHits, outCount, slotIndex);
		}
	}
	FoldWaveCounters(counters, cPoints, cNodes, cTris, lane);
}
