// k_overlap_box: batched oriented-box range queries on a finalized scene (include/raylib_amd.h RaylibAMD_OverlapBoxes, statements B1 to B6).  rl_overlap_box.hip
// includes this file and instantiates the kernels; the other units see the declaration and the instance list of rl_kernels.h.
//
// The walk is k_overlap's (rl_k_overlap.inl), driven by the same predicate: the box B2 makes of the query meets the child's box under O2's closed comparison
// (rl_overlap.h OverlapBoxesMeet).  B2's box is part of the verdict (rl_box.h), so nothing is widened: a child that does not meet holds no triangle that B2
// would let through, and the tree, the order of the walk and the cut into waves change no result.
// The walk's text is written here a second time, not shared with k_overlap: that kernel's header records that hoisting its walk into a function changed all
// twelve of its schedules and cost 1 %; this unit takes from rl_dev_boxwalk.h what leaves the old objects alone -- the isect record's vertices, the chunk
// claim, the grid node's decode and the counter fold.
//
// Shaped like k_overlap: one query per lane (four 16-byte loads), a wave takes RL_QUERY_CHUNK queries per atomic from the launch's counter, the stack is this
// lane's column of an LDS array (entry k at stk[k * RL_BLOCK]), at most (children - 1) pushes per level, so the planner's bounds hold.
// ANY leaves the walk at its first accepted triangle.  LIST keeps the lane's ascending list of export indices in the launch's dynamic LDS, maxHits * RL_BLOCK
// words, entry k of lane l at word k * RL_BLOCK + l, as k_overlap's, and always walks to the end.  MARK has no list and no dynamic LDS: an accepted triangle's
// bit (export index k: bit k % 32 of word k / 32) is ORed into the call's mask with a vector atomic, skipped when a plain load shows the bit set already -- a
// stale load costs an atomic, never a bit -- and the walk always runs to the end.  The host clears the mask on the launch's stream before the launch.

// One leaf: `count` triangles from slot `first`.  True: an ANY query has found its triangle.
template <int KIND>
__device__ __forceinline__ bool BoxLeaf(const DSceneView& S, const BoxQ& Q, int first, int count, const int32_t* __restrict__ slotIndex, uint32_t* __restrict__ list, uint32_t K,
                                        uint32_t& held, uint32_t& total, uint32_t* __restrict__ mask, uint32_t& tris)
{
	for (int i = 0; i < count; ++i) {
		const int slot = first + i;
		float v0[3], v1[3], v2[3];
		IsectVertices(S, slot, v0, v1, v2);
		++tris;
		if (!BoxAccepts(Q, v0, v1, v2)) continue;
		if (KIND == RL_BK_ANY) return true;
		const int32_t mine = slotIndex ? slotIndex[slot] : slot;
		if (KIND == RL_BK_MARK) {
			if ((uint32_t)mine >= (uint32_t)S.numTriangles) continue;   // (the mask ends there; a slot table names no such triangle)
			uint32_t* word = mask + ((uint32_t)mine >> 5);
			const uint32_t bit = 1u << ((uint32_t)mine & 31u);
			if (!(*word & bit)) atomicOr(word, bit);
			continue;
		}
		++total;
		if (held == K && mine > (int32_t)list[(K - 1u) * RL_BLOCK]) continue;
		uint32_t k = held < K ? held : K - 1u;   // the entry that is free, or the last one, which drops out
		while (k > 0u) {
			const int32_t prev = (int32_t)list[(k - 1u) * RL_BLOCK];
			if (prev < mine) break;
			list[k * RL_BLOCK] = (uint32_t)prev;
			--k;
		}
		list[k * RL_BLOCK] = (uint32_t)mine;
		if (held < K) ++held;
	}
	return false;
}

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int KIND, int STACK>
__global__ void __launch_bounds__(RL_BLOCK)
k_overlap_box(const DSceneView S, const float4* __restrict__ queries, uint32_t n, uint32_t maxHits, void* __restrict__ out, uint32_t* __restrict__ outCount,
              const int32_t* __restrict__ slotIndex, unsigned int* __restrict__ queryCounter, unsigned long long* __restrict__ counters)
{
	static_assert(TREE == 2 || TREE == 4, "tree");
	static_assert(KIND == RL_BK_ANY || KIND == RL_BK_LIST || KIND == RL_BK_MARK, "kind");
	__shared__ int s_stack[STACK * RL_BLOCK];
	extern __shared__ uint32_t s_box_list[];   // LIST: maxHits * RL_BLOCK words (the launch's dynamic LDS); ANY, MARK: none, never touched
	int* stk = s_stack + threadIdx.x;
	uint32_t* list = s_box_list + threadIdx.x;
	const uint32_t K = KIND == RL_BK_LIST ? maxHits : 0u;
#define RL_BOX_PUSH(ref_) { if (sp < STACK) { stk[sp * RL_BLOCK] = (ref_); ++sp; } }
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t cQueries = 0u, cNodes = 0u, cTris = 0u;
	const int DONE = RL_WALK_DONE;
	for (;;) {
		const uint32_t base = ClaimChunk(queryCounter, RL_QUERY_CHUNK, lane);
		if (base >= n) break;
		for (uint32_t k = 0; k < RL_QUERY_CHUNK; k += 64u) {
			const uint32_t i = base + k + lane;
			if (i >= n) continue;
			++cQueries;
			const float4* qp = queries + 4u * (size_t)i;   // (64-bit offset: n may reach 2^31 - 1)
			const float4 a0 = GLoadF4(qp, 0), a1 = GLoadF4(qp, 1), a2 = GLoadF4(qp, 2), a3 = GLoadF4(qp, 3);   // (the reserved word is not read)
			BoxQ Q;
			Q.c[0] = a0.x; Q.c[1] = a0.y; Q.c[2] = a0.z;
			Q.a[0][0] = a1.x; Q.a[0][1] = a1.y; Q.a[0][2] = a1.z; Q.h[0] = a1.w;
			Q.a[1][0] = a2.x; Q.a[1][1] = a2.y; Q.a[1][2] = a2.z; Q.h[1] = a2.w;
			Q.a[2][0] = a3.x; Q.a[2][1] = a3.y; Q.a[2][2] = a3.z; Q.h[2] = a3.w;
			uint32_t held = 0u, total = 0u;
			bool found = false;
			// a query that does not take part is answered without a walk
			if (BoxTakesPart(Q) && S.numTriangles > 0) {
				BoxEnclosing(Q);   // B2, once per query
				int sp = 0, cur = 0;   // the root is an inner node
				for (;;) {
					// ---- descend: inner nodes until this lane holds a leaf or has nothing left ----
					while (cur >= 0 && cur != DONE) {
						++cNodes;
						if constexpr (TREE == 2) {
							const float4* np = (const float4*)(S.nodes + cur);
							const float4 b0 = GLoadF4(np, 0), b1 = GLoadF4(np, 1), b2 = GLoadF4(np, 2);
							const uint4 ku = GLoadU4(np, 3);
							const int kl = (int)ku.x, kr = (int)ku.y;
							const bool hl = kl != DNODE_EMPTY && OverlapBoxesMeet(Q.lo, Q.hi, b0.x, b0.y, b0.z, b0.w, b1.x, b1.y);
							const bool hr = kr != DNODE_EMPTY && OverlapBoxesMeet(Q.lo, Q.hi, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w);
							if (hl && hr) { RL_BOX_PUSH(kr) cur = kl; }
							else if (hl) cur = kl;
							else if (hr) cur = kr;
							else cur = DONE;
						} else {
							const GridNode N = LoadGridNode(S.nodes4 + cur);
							int nr = DNODE_EMPTY;   // the kept child walked next; every other kept child is pushed
#pragma unroll
							for (int c = 3; c >= 0; --c) {
								float lo[3], hi[3];
								const int r = GridChild(N, c, lo, hi);
								if (r != DNODE_EMPTY && OverlapBoxesMeet(Q.lo, Q.hi, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2])) { if (nr != DNODE_EMPTY) RL_BOX_PUSH(nr) nr = r; }
							}
							cur = nr != DNODE_EMPTY ? nr : DONE;
						}
						if (cur == DONE && sp > 0) { --sp; cur = stk[sp * RL_BLOCK]; }
					}
					if (cur == DONE) break;
					// ---- leaf: <= 4 triangles stored back to back ----
					const LeafRef L = DecodeLeaf(cur);
					if (BoxLeaf<KIND>(S, Q, L.first, L.count, slotIndex, list, K, held, total, (uint32_t*)out, cTris)) { found = true; break; }
					if (sp == 0) break;
					--sp;
					cur = stk[sp * RL_BLOCK];
				}
			}
			if (KIND == RL_BK_ANY) ((uint32_t*)out)[i] = found ? 1u : 0u;
			else if (KIND == RL_BK_LIST) {
				int32_t* row = (int32_t*)out + (size_t)i * K;   // (64-bit: n * maxHits may reach 2^31 - 1)
				for (uint32_t e = 0; e < K; ++e) row[e] = e < held ? (int32_t)list[e * RL_BLOCK] : -1;
				if (outCount) outCount[i] = total;
			}
		}
	}
#undef RL_BOX_PUSH
	FoldWaveCounters(counters, cQueries, cNodes, cTris, lane);
}
