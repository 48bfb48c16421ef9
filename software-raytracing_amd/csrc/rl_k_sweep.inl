// k_sweep: batched swept-sphere queries on a finalized scene (include/raylib_amd.h RaylibAMD_SweepSpheres, statements W1 to W7 of rl_sweep.h).  rl_sweep.hip
// includes this file and instantiates the kernels; the other units see the declaration, the records and the instance list of rl_kernels.h.
//
// The walk is the point walk's shape (rl_dev_boxwalk.h) with a time in the place of a distance: children are ordered by the time bound of their box (W2,
// SweepBoxTime), nearest first, and culled when it is > bound, bound = the least T found so far, 1 at the start; a child is kept on equality, because a tie may
// still win on the export index.  Nothing is widened.  The bound rides beside a reference on the stack and a popped entry is re-tested against the current
// bound.  In a leaf a triangle's own box is tested against the bound before any of W3 / W4 is computed.  Every triangle's T is a property of the move and the
// triangle alone, and the box rule never drops a triangle that could win (W2, W5), so the tree, the order of the walk and the cut into waves change no result.
// The walk's text is kept here and not routed through PointWalk: a newly shared function changes the schedules of the kernels that call it
// (profiles/box_walk_ab.log).
//
// Shaped like k_nearest: one query per lane, a wave takes RL_QUERY_CHUNK queries per atomic from the launch's counter, the stack is this lane's column of an LDS
// array, counters are reduced per wave.
// RL_SWEEP_TIME32 / RL_SWEEP_TIME64: bytes of box time per entry of the 32- and the 64-deep instances' stacks (rl_dev_boxwalk.h NearestDist: 0, 2 or 4).  A time
// is >= +0 (or +inf), so the upper half rounds it down: the pop's re-test then culls a little less, never more, and no setting changes a result.  The half
// keeps the 32-deep instances at 48 KB of LDS, three workgroups per CU, where the float leaves two (profiles/sweep_resources.log).
#ifndef RL_SWEEP_TIME32
#define RL_SWEEP_TIME32 2
#endif
#ifndef RL_SWEEP_TIME64
#define RL_SWEEP_TIME64 2
#endif

// the walk's state of one CLOSEST query: the winner's slot, feature and point (its T is the walk's bound)
struct SweepBest { int slot; int feature; float p[3]; };

// One leaf: `count` triangles from slot `first`.  True: an ANY query has found its candidate.  A triangle replaces the best when its T is smaller, or equal with
// a lower export index (slotIndex, read on a tie only).
template <int KIND>
__device__ __forceinline__ bool SweepLeaf(const DSceneView& S, const SweepMove& M, int first, int count, float& bound, SweepBest& best, const int32_t* __restrict__ slotIndex,
                                          uint32_t& tris)
{
	for (int i = 0; i < count; ++i) {
		const int slot = first + i;
		float v0[3], v1[3], v2[3];
		IsectVertices(S, slot, v0, v1, v2);
		++tris;
		const float Bt = SweepOwnBoxTime(M, v0, v1, v2);
		if (Bt > bound) continue;   // T >= Bt: not a candidate, and t need not be known
		float t, p[3]; int feature;
		if (!SweepTriangle(M, v0, v1, v2, t, feature, p)) continue;
		const float T = SweepTriangleT(t, Bt);
		if (T > bound) continue;
		if (KIND == RL_SK_ANY) return true;   // T <= 1 (the bound never moves)
		if (T == bound && best.slot >= 0) {
			const int mine = slotIndex ? slotIndex[slot] : slot, theirs = slotIndex ? slotIndex[best.slot] : best.slot;
			if (mine > theirs) continue;
		}
		bound = T; best.slot = slot; best.feature = feature; best.p[0] = p[0]; best.p[1] = p[1]; best.p[2] = p[2];
	}
	return false;
}

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int KIND, int STACK>
__global__ void __launch_bounds__(RL_BLOCK)
k_sweep(const DSceneView S, const float4* __restrict__ queries, uint32_t n, void* __restrict__ out, const int32_t* __restrict__ slotIndex,
        unsigned int* __restrict__ queryCounter, unsigned long long* __restrict__ counters)
{
	static_assert(TREE == 2 || TREE == 4, "tree");
	static_assert(KIND == RL_SK_ANY || KIND == RL_SK_CLOSEST, "kind");
	__shared__ int s_stack[STACK * RL_BLOCK];
	int* stk = s_stack + threadIdx.x;
	constexpr int DBYTES = STACK <= 32 ? RL_SWEEP_TIME32 : RL_SWEEP_TIME64;
	typedef NearestDist<DBYTES> Time;
	__shared__ typename Time::T s_time[DBYTES != 0 ? STACK * RL_BLOCK : 1];
	typename Time::T* tstk = s_time + (DBYTES != 0 ? threadIdx.x : 0u);
	const uint32_t lane = threadIdx.x & 63u;
	const int DONE = RL_WALK_DONE;
	uint32_t cQueries = 0u, cNodes = 0u, cTris = 0u;
	// (push and pop as macros, as the point walk's)
#define RL_SWEEP_PUSH(ref_, t_) { if (sp < STACK) { stk[sp * RL_BLOCK] = (ref_); if constexpr (DBYTES != 0) tstk[sp * RL_BLOCK] = Time::Pack(t_); ++sp; } }
#define RL_SWEEP_POP() while (cur == DONE && sp > 0) { --sp; if constexpr (DBYTES != 0) if (Time::Unpack(tstk[sp * RL_BLOCK]) > bound) continue; cur = stk[sp * RL_BLOCK]; }
	for (;;) {
		const uint32_t base = ClaimChunk(queryCounter, RL_QUERY_CHUNK, lane);
		if (base >= n) break;
		for (uint32_t k = 0; k < RL_QUERY_CHUNK; k += 64u) {
			const uint32_t i = base + k + lane;
			if (i >= n) continue;
			++cQueries;
			const float4 q0 = GLoadF4(queries + 2u * (size_t)i, 0), q1 = GLoadF4(queries + 2u * (size_t)i, 1);   // (64-bit offset: n may reach 2^31 - 1)
			const float o[3] = { q0.x, q0.y, q0.z }, delta[3] = { q1.x, q1.y, q1.z };
			SweepMove M;
			float bound = 1.0f;
			SweepBest best; best.slot = -1; best.feature = 0; best.p[0] = best.p[1] = best.p[2] = 0.0f;
			bool found = false;
			// a query that does not take part is answered without a walk
			if (SweepTakesPart(o, delta, q0.w, M) && S.numTriangles > 0) {
				int sp = 0, cur = 0;
				for (;;) {
					// ---- descend: inner nodes until this lane holds a leaf or has nothing left ----
					while (cur >= 0 && cur != DONE) {
						++cNodes;
						if constexpr (TREE == 2) {
							const float4* np = (const float4*)(S.nodes + cur);
							const float4 b0 = GLoadF4(np, 0), b1 = GLoadF4(np, 1), b2 = GLoadF4(np, 2);
							const uint4 ku = GLoadU4(np, 3);
							const int kl = (int)ku.x, kr = (int)ku.y;
							const float llo[3] = { b0.x, b0.y, b0.z }, lhi[3] = { b0.w, b1.x, b1.y }, rlo[3] = { b1.z, b1.w, b2.x }, rhi[3] = { b2.y, b2.z, b2.w };
							const float tl = SweepBoxTime(M, llo, lhi), tr = SweepBoxTime(M, rlo, rhi);
							const bool hl = kl != DNODE_EMPTY && !(tl > bound), hr = kr != DNODE_EMPTY && !(tr > bound);
							if (hl && hr) {
								const bool leftFirst = tl <= tr;
								RL_SWEEP_PUSH(leftFirst ? kr : kl, leftFirst ? tr : tl)
								cur = leftFirst ? kl : kr;
							} else if (hl) cur = kl;
							else if (hr) cur = kr;
							else cur = DONE;
						} else {
							const GridNode N = LoadGridNode(S.nodes4 + cur);
							float t[4]; int r[4];
#pragma unroll
							for (int c = 0; c < 4; ++c) {
								float lo[3], hi[3];
								r[c] = GridChild(N, c, lo, hi);
								t[c] = SweepBoxTime(M, lo, hi);
								// a dropped child: no reference, behind every kept one
								if (r[c] == DNODE_EMPTY || t[c] > bound) { r[c] = DNODE_EMPTY; t[c] = INFINITY; }
							}
							RL_SORT4(t[0], r[0], t[1], r[1], t[2], r[2], t[3], r[3])
							// from the farthest to the nearest: the nearest kept child is walked next, the others are pushed farthest first
							int nr = r[3]; float nt = t[3];
#pragma unroll
							for (int c = 2; c >= 0; --c) if (r[c] != DNODE_EMPTY) { if (nr != DNODE_EMPTY) RL_SWEEP_PUSH(nr, nt) nr = r[c]; nt = t[c]; }
							cur = nr != DNODE_EMPTY ? nr : DONE;
						}
						RL_SWEEP_POP()   // nothing kept
					}
					if (cur == DONE) break;
					// ---- leaf ----
					const LeafRef L = DecodeLeaf(cur);
					if (SweepLeaf<KIND>(S, M, L.first, L.count, bound, best, slotIndex, cTris)) { found = true; break; }
					cur = DONE;
					RL_SWEEP_POP()
					if (cur == DONE) break;
				}
			}
			if (KIND == RL_SK_ANY) ((uint32_t*)out)[i] = found ? 1u : 0u;
			else {
				// (the 32-byte record as two stores)
				float4* rec = (float4*)out + 2u * (size_t)i;
				if (best.slot < 0) { rec[0] = make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f); rec[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
				else {
					const int32_t prim = slotIndex ? slotIndex[best.slot] : best.slot;
					rec[0] = make_float4(bound, __int_as_float(prim), __int_as_float(best.feature), 0.0f);
					rec[1] = make_float4(best.p[0], best.p[1], best.p[2], 0.0f);
				}
			}
		}
	}
#undef RL_SWEEP_POP
#undef RL_SWEEP_PUSH
	FoldWaveCounters(counters, cQueries, cNodes, cTris, lane);
}
