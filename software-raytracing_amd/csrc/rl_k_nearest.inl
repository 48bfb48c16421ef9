// k_nearest: batched nearest-point queries on a finalized scene (include/raylib_amd.h RaylibAMD_NearestPoints, statements N1 to N5).  rl_nearest.hip includes
// this file and instantiates the kernels; the other units see the declaration, the records and the instance list of rl_kernels.h.
//
// The walk is not a ray walk: children are ordered and culled by the distance from the point to their box (rl_nearest.h NearestBoxDist2), not by a parametric
// distance, and nothing is widened -- a child is dropped when its box distance is > best, kept when it is == best (a tie may still win on the export index).
// "best" starts at R2 = maxDist * maxDist; a triangle replaces the best when its D is smaller, or equal with a lower export index (slotIndex, read on a tie and
// for the final record only).  Every triangle's D is a property of the point and the triangle alone, and the box rule never drops a triangle that could win, so
// the tree, the order of the walk and the cut into waves change no result.
//
// Shaped like k_query: one point per lane, a wave takes RL_QUERY_CHUNK points per atomic from the launch's counter, the stack is this lane's column of an LDS
// array (entry k at stk[k * RL_BLOCK]), counters are reduced per wave.  Both walks push at most (children - 1) references per level, as the ray walks do, so
// the planner's bounds hold: the binary tree's depth and the 4-wide tree's BVH::stackNeed4.
// A popped reference is re-tested against the current best when the stack keeps its box distance beside it; otherwise the popped node's children's tests (a
// leaf's own-box tests) do the culling, one fetch later.  RL_NEAREST_DIST32 / RL_NEAREST_DIST64: bytes of distance per entry of the 32- and the 64-deep
// instances' stacks -- 0 none, 4 the float, 2 its upper half (a distance is >= +0, so dropping mantissa bits rounds it down: the re-test then culls a
// little less, never more).  No setting changes a result; what each costs in LDS and buys in node fetches was measured on the 298 k-triangle room (DESIGN.md
// section 2, profiles/nearest_stack_ab.log): the half distance visits the nodes the float does (19.8 per surface-near point for 35.9 without, binary tree;
// 10.9 for 34.8, grid tree) and leaves 3 waves per SIMD (32-deep, 48 KB) where the float leaves 2.
#ifndef RL_NEAREST_DIST32
#define RL_NEAREST_DIST32 2
#endif
#ifndef RL_NEAREST_DIST64
#define RL_NEAREST_DIST64 2
#endif
template <int BYTES> struct NearestDist;
template <> struct NearestDist<0> { typedef float T; static __device__ __forceinline__ T Pack(float) { return 0.0f; } static __device__ __forceinline__ float Unpack(T) { return 0.0f; } };
template <> struct NearestDist<4> { typedef float T; static __device__ __forceinline__ T Pack(float d) { return d; } static __device__ __forceinline__ float Unpack(T v) { return v; } };
template <> struct NearestDist<2> {
	typedef unsigned short T;
	static __device__ __forceinline__ T Pack(float d) { return (T)(__float_as_uint(d) >> 16); }
	static __device__ __forceinline__ float Unpack(T v) { return __uint_as_float((uint32_t)v << 16); }
};

// the walk's state of one point
struct NearestBest { float d; int slot; float b1, b2; };

// One leaf: `count` triangles from slot `first`.  True: a WITHIN query has found its candidate.
template <int KIND>
__device__ __forceinline__ bool NearestLeaf(const DSceneView& S, const float p[3], int first, int count, NearestBest& best, const int32_t* __restrict__ slotIndex, uint32_t& tris)
{
	for (int i = 0; i < count; ++i) {
		const int slot = first + i;
		const float4* tp = (const float4*)(S.isect + slot);
		const float4 q0 = GLoadF4(tp, 0), q1 = GLoadF4(tp, 1), q2 = GLoadF4(tp, 2);
		const float v0[3] = { q0.x, q0.y, q0.z }, v1[3] = { q1.z, q1.w, q2.x }, v2[3] = { q2.y, q2.z, q2.w };
		++tris;
		const float B = NearestOwnBoxDist2(p, v0, v1, v2);
		if (B > best.d) continue;   // D >= B: not a candidate, and E need not be known
		float b1, b2;
		const float D = NearestTriangleD(NearestTriangleE(p, v0, v1, v2, b1, b2), B);
		if (D > best.d) continue;
		if (KIND == RL_NK_WITHIN) return true;   // D <= R2 (best.d never moves)
		if (D == best.d && best.slot >= 0) {
			const int mine = slotIndex ? slotIndex[slot] : slot, theirs = slotIndex ? slotIndex[best.slot] : best.slot;
			if (mine > theirs) continue;
		}
		best.d = D; best.slot = slot; best.b1 = b1; best.b2 = b2;
	}
	return false;
}

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int KIND, int STACK>
__global__ void __launch_bounds__(RL_BLOCK)
k_nearest(const DSceneView S, const float4* __restrict__ points, uint32_t n, void* __restrict__ out, const int32_t* __restrict__ slotIndex,
          unsigned int* __restrict__ pointCounter, unsigned long long* __restrict__ counters)
{
	static_assert(TREE == 2 || TREE == 4, "tree");
	static_assert(KIND == RL_NK_WITHIN || KIND == RL_NK_CLOSEST, "kind");
	__shared__ int s_stack[STACK * RL_BLOCK];
	int* stk = s_stack + threadIdx.x;
	typedef NearestDist<(STACK <= 32 ? RL_NEAREST_DIST32 : RL_NEAREST_DIST64)> Dist;
	constexpr bool POPD = (STACK <= 32 ? RL_NEAREST_DIST32 : RL_NEAREST_DIST64) != 0;
	__shared__ typename Dist::T s_dist[POPD ? STACK * RL_BLOCK : 1];
	typename Dist::T* dstk = s_dist + (POPD ? threadIdx.x : 0u);
#define RL_NEAREST_PUSH(ref_, d_) { if (sp < STACK) { stk[sp * RL_BLOCK] = (ref_); if constexpr (POPD) dstk[sp * RL_BLOCK] = Dist::Pack(d_); ++sp; } }
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t cPoints = 0u, cNodes = 0u, cTris = 0u;
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
			NearestBest best; best.d = q.w * q.w; best.slot = -1; best.b1 = best.b2 = 0.0f;
			bool found = false;
			// a point that does not take part is answered without a walk (a NaN bound would cull nothing)
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
							const bool hl = kl != DNODE_EMPTY && !(dl > best.d), hr = kr != DNODE_EMPTY && !(dr > best.d);
							if (hl && hr) {
								const bool leftFirst = dl <= dr;
								RL_NEAREST_PUSH(leftFirst ? kr : kl, leftFirst ? dr : dl)
								cur = leftFirst ? kl : kr;
							} else if (hl) cur = kl;
							else if (hr) cur = kr;
							else cur = DONE;
						} else {
							// the 64-byte grid node: child c's planes decoded as origin + (float)q * step -- the product is exact (q <= 255, step a power of two), the
							// sum rounds once, monotonically, so the decoded box still contains the float box the planes were rounded outwards from (rl_grid.h)
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
	if (rk == DNODE_EMPTY || tk > best.d) { rk = DNODE_EMPTY; tk = INFINITY; } }
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
						// nothing kept: the stack's next entry that the best has not passed since it was pushed
						while (cur == DONE && sp > 0) {
							--sp;
							if constexpr (POPD) if (Dist::Unpack(dstk[sp * RL_BLOCK]) > best.d) continue;
							cur = stk[sp * RL_BLOCK];
						}
					}
					if (cur == DONE) break;
					// ---- leaf: <= 4 triangles stored back to back ----
					const LeafRef L = DecodeLeaf(cur);
					if (NearestLeaf<KIND>(S, p, L.first, L.count, best, slotIndex, cTris)) { found = true; break; }
					cur = DONE;
					while (cur == DONE && sp > 0) {
						--sp;
						if constexpr (POPD) if (Dist::Unpack(dstk[sp * RL_BLOCK]) > best.d) continue;
						cur = stk[sp * RL_BLOCK];
					}
					if (cur == DONE) break;
				}
			}
			if (KIND == RL_NK_WITHIN) ((uint32_t*)out)[i] = found ? 1u : 0u;
			else {
				// (the 16-byte record as one store)
				const int32_t prim = best.slot < 0 ? -1 : slotIndex ? slotIndex[best.slot] : best.slot;
				((float4*)out)[i] = best.slot < 0 ? make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f) : make_float4(best.d, __int_as_float(prim), best.b1, best.b2);
			}
		}
	}
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
