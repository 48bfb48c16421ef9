// k_nearest: batched nearest-point queries on a finalized scene (include/raylib_amd.h RaylibAMD_NearestPoints, statements N1 to N5).  rl_nearest.hip includes
// this file and instantiates the kernels; the other units see the declaration, the records and the instance list of rl_kernels.h.
//
// The walk is rl_dev_boxwalk.h's point walk, with NearestLeaf of that file at its leaves and the best distance as its bound.  "best" starts at
// R2 = maxDist * maxDist; a triangle replaces the best when its D is smaller, or equal with a lower export index (slotIndex, read on a tie and for the final
// record only).  Every triangle's D is a property of the point and the triangle alone, and the walk's box rule never drops a triangle that could win, so the
// tree, the order of the walk and the cut into waves change no result.
//
// Shaped like k_query: one point per lane, a wave takes RL_QUERY_CHUNK points per atomic from the launch's counter, the stack is this lane's column of an LDS
// array, counters are reduced per wave.
// RL_NEAREST_DIST32 / RL_NEAREST_DIST64: bytes of box distance per entry of the 32- and the 64-deep instances' stacks (rl_dev_boxwalk.h NearestDist: 0, 2
// or 4).  No setting changes a result; what each costs in LDS and buys in node fetches was measured on the 298 k-triangle room (DESIGN.md
// section 2, profiles/nearest_stack_ab.log): the half distance visits the nodes the float does (19.8 per surface-near point for 35.9 without, binary tree;
// 10.9 for 34.8, grid tree) and leaves 3 waves per SIMD (32-deep, 48 KB) where the float leaves 2.
#ifndef RL_NEAREST_DIST32
#define RL_NEAREST_DIST32 2
#endif
#ifndef RL_NEAREST_DIST64
#define RL_NEAREST_DIST64 2
#endif

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int KIND, int STACK>
__global__ void __launch_bounds__(RL_BLOCK)
k_nearest(const DSceneView S, const float4* __restrict__ points, uint32_t n, void* __restrict__ out, const int32_t* __restrict__ slotIndex,
          unsigned int* __restrict__ pointCounter, unsigned long long* __restrict__ counters)
{
	static_assert(KIND == RL_NK_WITHIN || KIND == RL_NK_CLOSEST, "kind");
	__shared__ int s_stack[STACK * RL_BLOCK];
	int* stk = s_stack + threadIdx.x;
	constexpr int DBYTES = STACK <= 32 ? RL_NEAREST_DIST32 : RL_NEAREST_DIST64;
	typedef NearestDist<DBYTES> Dist;
	__shared__ typename Dist::T s_dist[DBYTES != 0 ? STACK * RL_BLOCK : 1];
	typename Dist::T* dstk = s_dist + (DBYTES != 0 ? threadIdx.x : 0u);
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t cPoints = 0u, cNodes = 0u, cTris = 0u;
	for (;;) {
		const uint32_t base = ClaimChunk(pointCounter, RL_QUERY_CHUNK, lane);
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
			if (NearestTakesPart(q.x, q.y, q.z, q.w) && S.numTriangles > 0)
				found = PointWalk<TREE, STACK, DBYTES>(S, p, best.d, stk, dstk, cNodes,
				                                       [&](int first, int count) { return NearestLeaf<KIND>(S, p, first, count, best, slotIndex, cTris); });
			if (KIND == RL_NK_WITHIN) ((uint32_t*)out)[i] = found ? 1u : 0u;
			else {
				// (the 16-byte record as one store)
				const int32_t prim = best.slot < 0 ? -1 : slotIndex ? slotIndex[best.slot] : best.slot;
				((float4*)out)[i] = best.slot < 0 ? make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f) : make_float4(best.d, __int_as_float(prim), best.b1, best.b2);
			}
		}
	}
	FoldWaveCounters(counters, cPoints, cNodes, cTris, lane);
}
