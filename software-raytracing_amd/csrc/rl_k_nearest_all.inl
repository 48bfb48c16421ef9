// k_nearest_all: the K nearest triangles of each point and the count in range (include/raylib_amd.h RaylibAMD_NearestPointsAll, statements K1 to K5).
// rl_nearest.hip includes this file behind rl_k_nearest.inl -- NearestDist and the RL_NEAREST_DIST32 / 64 settings are that file's -- and instantiates the
// kernels; k_nearest's instances stay the code they are (tools/isa_equivalence.py), so the walk is written here again and rl_k_nearest.inl is left alone.
//
// The walk is k_nearest's: one point per lane, RL_QUERY_CHUNK points per atomic, the stack and its packed distances as this lane's LDS columns, children
// ordered and culled by NearestBoxDist2 unwidened -- dropped when the box distance is > the bound, kept when it is == -- counters reduced per wave.  What
// differs is the bound and what stands behind the triangle test:
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
		const float4* tp = (const float4*)(S.isect + slot);
		const float4 q0 = GLoadF4(tp, 0), q1 = GLoadF4(tp, 1), q2 = GLoadF4(tp, 2);
		const float v0[3] = { q0.x, q0.y, q0.z }, v1[3] = { q1.z, q1.w, q2.x }, v2[3] = { q2.y, q2.z, q2.w };
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
			const float4* tp = (const float4*)(S.isect + slot);
			const float4 q0 = GLoadF4(tp, 0), q1 = GLoadF4(tp, 1), q2 = GLoadF4(tp, 2);
			const float v0[3] = { q0.x, q0.y, q0.z }, v1[3] = { q1.z, q1.w, q2.x }, v2[3] = { q2.y, q2.z, q2.w };
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
	static_assert(TREE == 2 || TREE == 4, "tree");
	__shared__ int s_stack[STACK * RL_BLOCK];
	extern __shared__ uint32_t s_list[];   // 2 * maxHits * RL_BLOCK words (the launch's dynamic LDS)
	int* stk = s_stack + threadIdx.x;
	typedef NearestDist<(STACK <= 32 ? RL_NEAREST_DIST32 : RL_NEAREST_DIST64)> Dist;
	constexpr bool POPD = (STACK <= 32 ? RL_NEAREST_DIST32 : RL_NEAREST_DIST64) != 0;
	__shared__ typename Dist::T s_dist[POPD ? STACK * RL_BLOCK : 1];
	typename Dist::T* dstk = s_dist + (POPD ? threadIdx.x : 0u);
#define RL_NEAREST_PUSH(ref_, d_) { if (sp < STACK) { stk[sp * RL_BLOCK] = (ref_); if constexpr (POPD) dstk[sp * RL_BLOCK] = Dist::Pack(d_); ++sp; } }
// the stack's next entry that the bound has not passed since it was pushed
#define RL_NEAREST_POP() while (cur == DONE && sp > 0) { --sp; if constexpr (POPD) if (Dist::Unpack(dstk[sp * RL_BLOCK]) > bound) continue; cur = stk[sp * RL_BLOCK]; }
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t cPoints = 0u, cNodes = 0u, cTris = 0u;
	NearestList L; L.at = s_list + threadIdx.x; L.K = maxHits; L.n = 0u; L.total = 0u;
	const int DONE = 0x7fffffff;   // not a node index, not negative
	for (;;) {
		uint32_t base = 0u;
		if (lane == 0u) base = atomicAdd(pointCounter, RL_QUERY_CHUNK);
		base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
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
			if (NearestTakesPart(q.x, q.y, q.z, q.w) && S.numTriangles > 0) {
				int sp = 0, cur = 0;   // the root is an inner node
				for (;;) {
					// ---- descend: inner nodes until this lane holds a leaf or has nothing left ----
					while (cur >= 0 && cur != DONE) {
						++cNodes;
						if constexpr (TREE == 2) {
							const float4* np = (const float4*)(S.nodes + cur);
							const float4 q0 = GLoadF4(np, 0), q1 = GLoadF4(np, 1), q2 = GLoadF4(np, 2);
							const uint4 ku = GLoadU4(np, 3);
							const int kl = (int)ku.x, kr = (int)ku.y;
							const float dl = NearestBoxDist2(p[0], p[1], p[2], q0.x, q0.y, q0.z, q0.w, q1.x, q1.y);
							const float dr = NearestBoxDist2(p[0], p[1], p[2], q1.z, q1.w, q2.x, q2.y, q2.z, q2.w);
							const bool hl = kl != DNODE_EMPTY && !(dl > bound), hr = kr != DNODE_EMPTY && !(dr > bound);
							if (hl && hr) {
								const bool leftFirst = dl <= dr;
								RL_NEAREST_PUSH(leftFirst ? kr : kl, leftFirst ? dr : dl)
								cur = leftFirst ? kl : kr;
							} else if (hl) cur = kl;
							else if (hr) cur = kr;
							else cur = DONE;
						} else {
							// the 64-byte grid node, decoded as k_nearest decodes it: origin + (float)q * step, a box that contains the float box it was quantised from
							const DNode4Q* np = S.nodes4 + cur;
							const float4 h0 = GLoadF4(np, 0); const uint4 l = GLoadU4(np, 1), u = GLoadU4(np, 2), chu = GLoadU4(np, 3);
							const float sx = h0.w, sy = __uint_as_float(l.w), sz = __uint_as_float(u.w);
							float t0, t1, t2, t3;
							int r0 = (int)chu.x, r1 = (int)chu.y, r2 = (int)chu.z, r3 = (int)chu.w;
#define RL_NEAREST_QBOX(sh, tk, rk) { \
	const float lox = h0.x + (float)((l.x >> sh) & 0xffu) * sx, hix = h0.x + (float)((u.x >> sh) & 0xffu) * sx; \
	const float loy = h0.y + (float)((l.y >> sh) & 0xffu) * sy, hiy = h0.y + (float)((u.y >> sh) & 0xffu) * sy; \
	const float loz = h0.z + (float)((l.z >> sh) & 0xffu) * sz, hiz = h0.z + (float)((u.z >> sh) & 0xffu) * sz; \
	tk = NearestBoxDist2(p[0], p[1], p[2], lox, loy, loz, hix, hiy, hiz); \
	/* a dropped child: no reference, behind every kept one (a kept child's distance may be +inf too: the reference tells them apart) */ \
	if (rk == DNODE_EMPTY || tk > bound) { rk = DNODE_EMPTY; tk = INFINITY; } }
							RL_NEAREST_QBOX(0, t0, r0) RL_NEAREST_QBOX(8, t1, r1) RL_NEAREST_QBOX(16, t2, r2) RL_NEAREST_QBOX(24, t3, r3)
#undef RL_NEAREST_QBOX
							RL_SORT4(t0, r0, t1, r1, t2, r2, t3, r3)
							// from the farthest to the nearest: the nearest kept child is walked next, the others are pushed farthest first
							int nr = r3; float nt = t3;
#define RL_NEAREST_TAKE(tk, rk) if (rk != DNODE_EMPTY) { if (nr != DNODE_EMPTY) RL_NEAREST_PUSH(nr, nt) nr = rk; nt = tk; }
							RL_NEAREST_TAKE(t2, r2) RL_NEAREST_TAKE(t1, r1) RL_NEAREST_TAKE(t0, r0)
#undef RL_NEAREST_TAKE
							cur = nr != DNODE_EMPTY ? nr : DONE;
						}
						RL_NEAREST_POP()
					}
					if (cur == DONE) break;
					// ---- leaf: <= 4 triangles stored back to back ----
					const LeafRef F = DecodeLeaf(cur);
					NearestLeafAll<COUNT>(S, p, F.first, F.count, bound, L, slotIndex, cTris);
					cur = DONE;
					RL_NEAREST_POP()
					if (cur == DONE) break;
				}
			}
			NearestStoreAll(S, p, L, i, outHits, outCount, slotIndex);
		}
	}
#undef RL_NEAREST_POP
#undef RL_NEAREST_PUSH
	if (counters) {   // wave reduction, one atomic per wave and counter
		const uint32_t vals[3] = { cPoints, cNodes, cTris };
		for (int k = 0; k < 3; ++k) {
			unsigned long long v = vals[k];
			for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
			if (lane == 0u && v) atomicAdd(&counters[CNT_RAYS + k], v);
		}
	}
}
