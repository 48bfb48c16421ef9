// k_overlap: batched triangle-overlap queries on a finalized scene (include/raylib_amd.h RaylibAMD_OverlapTriangles, statements O1 to O6).  rl_overlap.hip
// includes this file and instantiates the kernels; the other units see the declaration and the instance list of rl_kernels.h.
//
// The walk is driven by a box predicate, as k_nearest's, but by the simplest one: the query triangle's own box meets the child's box under O2's closed
// comparison (rl_overlap.h OverlapBoxesMeet).  Nothing is ordered, nothing is widened and no distance rides on the stack: every child that meets is walked,
// one at once and the others pushed.  O2 is pure comparisons and the trees' boxes nest exactly (rl_overlap.h), so a child that does not meet holds no triangle
// that O2 would let through; every triangle's verdict is a property of the query and the triangle alone, so the tree, the order of the walk and the cut into
// waves change no result.
//
// Shaped like k_nearest: one query per lane, a wave takes RL_QUERY_CHUNK queries per atomic from the launch's counter, the stack is this lane's column of an
// LDS array (entry k at stk[k * RL_BLOCK]), counters are reduced per wave; the 64-byte isect records and the grid node's decode are used as there.  Both
// walks push at most (children - 1) references per level, so the planner's bounds hold: the binary tree's depth and the 4-wide tree's BVH::stackNeed4.
// ANY leaves the walk at its first accepted triangle.  LIST keeps the lane's ascending list of export indices (slotIndex[slot]) in the launch's dynamic LDS,
// maxHits * RL_BLOCK words, entry k of lane l at word k * RL_BLOCK + l: the lanes of a wave touch consecutive words whatever k each of them is at, so no
// two lanes of a 32-lane half share a bank.  A candidate above a full list's last entry only counts.  Every slot sits in exactly one leaf: no index comes
// twice.  The list orders by export index, which says nothing about where a triangle lies, so a full list prunes nothing and LIST always walks to the end.
// The contacts kind (k_overlap_contacts: RaylibAMD_OverlapContacts) is LIST up to write-out; there every held entry gets its record (rl_contact.h, statements C1
// to C6).  It carries two more arguments, so it is a kernel of its own name, and it is this file's text a second time: rl_overlap.hip includes the file once
// plainly, which gives k_overlap, and once under RL_OVERLAP_CONTACTS_PASS, which gives k_overlap_contacts.
// The walk stays written here, and so do the grid node's decode in it and the counter fold; only the isect record's vertices and the chunk claim come from
// rl_dev_boxwalk.h.  Measured (profiles/box_walk_ab.log): with the walk as a function of that header which both kernels called -- one
// inclusion, no pass macro -- every instance compiled to another schedule, and k_overlap<4, ANY> ran 1.004 to 1.012 of the parent's time in every job, over
// the run-to-run spread; one body for both kernels with the walk inside it brought that to 1.003 - 1.007, still over it in two rows of four.  Even the fold as
// a function changes all twelve schedules.  With what is shared now the twelve instances are the parent's, instruction for instruction
// (profiles/box_walk_isa_equivalence.log).
// The list is keyed by export index and the record needs the triangle's slot: a table, export index -> slot, beside slotIndex (4 bytes per
// triangle) gives it, so the dynamic LDS and with it the occupancy stay LIST's.

#ifndef RL_OVERLAP_CONTACTS_PASS
// One leaf: `count` triangles from slot `first`.  True: an ANY query has found its triangle.
template <int KIND>
__device__ __forceinline__ bool OverlapLeaf(const DSceneView& S, const float q0[3], const float q1[3], const float q2[3], const float loQ[3], const float hiQ[3], bool skipShared,
                                            int first, int count, const int32_t* __restrict__ slotIndex, uint32_t* __restrict__ list, uint32_t K, uint32_t& held, uint32_t& total,
                                            uint32_t& tris)
{
	for (int i = 0; i < count; ++i) {
		const int slot = first + i;
		float v0[3], v1[3], v2[3];
		IsectVertices(S, slot, v0, v1, v2);
		++tris;
		if (!OverlapAccepts(q0, q1, q2, loQ, hiQ, v0, v1, v2, skipShared)) continue;
		if (KIND == RL_OK_ANY) return true;
		++total;
		const int32_t mine = slotIndex ? slotIndex[slot] : slot;
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

#endif

// (template and kernel arguments: rl_kernels.h)
#ifndef RL_OVERLAP_CONTACTS_PASS
template <int TREE, int KIND, int STACK>
__global__ void __launch_bounds__(RL_BLOCK)
k_overlap(const DSceneView S, const float4* __restrict__ queries, uint32_t n, uint32_t flags, uint32_t maxHits, void* __restrict__ out, uint32_t* __restrict__ outCount,
          const int32_t* __restrict__ slotIndex, unsigned int* __restrict__ queryCounter, unsigned long long* __restrict__ counters)
{
	static_assert(TREE == 2 || TREE == 4, "tree");
	static_assert(KIND == RL_OK_ANY || KIND == RL_OK_LIST, "kind");
#else
template <int TREE, int STACK>
__global__ void __launch_bounds__(RL_BLOCK)
k_overlap_contacts(const DSceneView S, const float4* __restrict__ queries, uint32_t n, uint32_t flags, uint32_t maxHits, void* __restrict__ out, uint32_t* __restrict__ outCount,
                   const int32_t* __restrict__ slotIndex, unsigned int* __restrict__ queryCounter, unsigned long long* __restrict__ counters,
                   float4* __restrict__ outContact, const int32_t* __restrict__ exportSlot)
{
	static_assert(TREE == 2 || TREE == 4, "tree");
	constexpr int KIND = RL_OK_LIST;   // the walk, the list and the rows are LIST's
#endif
	__shared__ int s_stack[STACK * RL_BLOCK];
	extern __shared__ uint32_t s_overlap_list[];   // LIST: maxHits * RL_BLOCK words (the launch's dynamic LDS); ANY: none, never touched
	int* stk = s_stack + threadIdx.x;
	uint32_t* list = s_overlap_list + threadIdx.x;
	const uint32_t K = KIND == RL_OK_LIST ? maxHits : 0u;
	const bool skipShared = (flags & RL_OVERLAP_SKIP_SHARED) != 0u;
#define RL_OVERLAP_PUSH(ref_) { if (sp < STACK) { stk[sp * RL_BLOCK] = (ref_); ++sp; } }
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t cQueries = 0u, cNodes = 0u, cTris = 0u;
	const int DONE = 0x7fffffff;   // not a node index, not negative
	for (;;) {
		const uint32_t base = ClaimChunk(queryCounter, RL_QUERY_CHUNK, lane);
		if (base >= n) break;
		for (uint32_t k = 0; k < RL_QUERY_CHUNK; k += 64u) {
			const uint32_t i = base + k + lane;
			if (i >= n) continue;
			++cQueries;
			const float4* qp = queries + 3u * (size_t)i;   // (64-bit offset: n may reach 2^31 - 1)
			const float4 a0 = GLoadF4(qp, 0), a1 = GLoadF4(qp, 1), a2 = GLoadF4(qp, 2);   // (the reserved words are not read)
			const float q0[3] = { a0.x, a0.y, a0.z }, q1[3] = { a1.x, a1.y, a1.z }, q2[3] = { a2.x, a2.y, a2.z };
			uint32_t held = 0u, total = 0u;
			bool found = false;
			// a query that does not take part is answered without a walk
			if (OverlapTakesPart(q0, q1, q2) && S.numTriangles > 0) {
				float loQ[3], hiQ[3];
				OverlapOwnBox(q0, q1, q2, loQ, hiQ);
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
							const bool hl = kl != DNODE_EMPTY && OverlapBoxesMeet(loQ, hiQ, b0.x, b0.y, b0.z, b0.w, b1.x, b1.y);
							const bool hr = kr != DNODE_EMPTY && OverlapBoxesMeet(loQ, hiQ, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w);
							if (hl && hr) { RL_OVERLAP_PUSH(kr) cur = kl; }
							else if (hl) cur = kl;
							else if (hr) cur = kr;
							else cur = DONE;
						} else {
							// the 64-byte grid node: child c's planes decoded as origin + (float)q * step -- the product is exact (q <= 255, step a power of two), the
							// sum rounds once, monotonically, so the decoded box still contains the float box the planes were rounded outwards from (rl_grid.h)
							const DNode4Q* np = S.nodes4 + cur;
							const float4 h0 = GLoadF4(np, 0); const uint4 l = GLoadU4(np, 1), u = GLoadU4(np, 2), chu = GLoadU4(np, 3);
							const float sx = h0.w, sy = __uint_as_float(l.w), sz = __uint_as_float(u.w);
							int nr = DNODE_EMPTY;   // the kept child walked next; every other kept child is pushed
#define RL_OVERLAP_QBOX(sh, rk) { \
	const float lox = h0.x + (float)((l.x >> sh) & 0xffu) * sx, hix = h0.x + (float)((u.x >> sh) & 0xffu) * sx; \
	const float loy = h0.y + (float)((l.y >> sh) & 0xffu) * sy, hiy = h0.y + (float)((u.y >> sh) & 0xffu) * sy; \
	const float loz = h0.z + (float)((l.z >> sh) & 0xffu) * sz, hiz = h0.z + (float)((u.z >> sh) & 0xffu) * sz; \
	const int r_ = (int)(rk); \
	if (r_ != DNODE_EMPTY && OverlapBoxesMeet(loQ, hiQ, lox, loy, loz, hix, hiy, hiz)) { if (nr != DNODE_EMPTY) RL_OVERLAP_PUSH(nr) nr = r_; } }
							RL_OVERLAP_QBOX(24, chu.w) RL_OVERLAP_QBOX(16, chu.z) RL_OVERLAP_QBOX(8, chu.y) RL_OVERLAP_QBOX(0, chu.x)
#undef RL_OVERLAP_QBOX
							cur = nr != DNODE_EMPTY ? nr : DONE;
						}
						if (cur == DONE && sp > 0) { --sp; cur = stk[sp * RL_BLOCK]; }
					}
					if (cur == DONE) break;
					// ---- leaf: <= 4 triangles stored back to back ----
					const LeafRef L = DecodeLeaf(cur);
					if (OverlapLeaf<KIND>(S, q0, q1, q2, loQ, hiQ, skipShared, L.first, L.count, slotIndex, list, K, held, total, cTris)) { found = true; break; }
					if (sp == 0) break;
					--sp;
					cur = stk[sp * RL_BLOCK];
				}
			}
			if (KIND == RL_OK_ANY) ((uint32_t*)out)[i] = found ? 1u : 0u;
			else {
				int32_t* row = (int32_t*)out + (size_t)i * K;   // (64-bit: n * maxHits may reach 2^31 - 1)
				for (uint32_t e = 0; e < K; ++e) row[e] = e < held ? (int32_t)list[e * RL_BLOCK] : -1;
				if (outCount) outCount[i] = total;
#ifdef RL_OVERLAP_CONTACTS_PASS
				// a record per row entry: Q is still in registers, T is read again from the entry's 64-byte record; behind the count, 32 zero bytes
				float4* rec = outContact + 2u * ((size_t)i * K);   // (64-bit: the records of n * maxHits entries pass 2^31 bytes long before the rows do)
				for (uint32_t e = 0; e < K; ++e) {
					float4 c0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c1 = c0;
					if (e < held) {
						const int32_t idx = (int32_t)list[e * RL_BLOCK];
						const int slot = exportSlot ? exportSlot[idx] : idx;
						float v0[3], v1[3], v2[3];
						IsectVertices(S, slot, v0, v1, v2);
						const ContactRecord R = ContactOfPair(q0, q1, q2, v0, v1, v2);
						c0 = make_float4(R.p0[0], R.p0[1], R.p0[2], __uint_as_float(R.kind));
						c1 = make_float4(R.p1[0], R.p1[1], R.p1[2], __uint_as_float(R.features));
					}
					rec[2u * e] = c0; rec[2u * e + 1u] = c1;
				}
#endif
			}
		}
	}
#undef RL_OVERLAP_PUSH
	if (counters) {   // wave reduction, one atomic per wave and counter
		const uint32_t vals[3] = { cQueries, cNodes, cTris };
		for (int k = 0; k < 3; ++k) {
			unsigned long long v = vals[k];
			for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
			if (lane == 0u && v) atomicAdd(&counters[CNT_RAYS + k], v);
		}
	}
}
