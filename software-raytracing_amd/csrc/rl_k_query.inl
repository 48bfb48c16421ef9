// k_query: batched ray queries on a finalized scene (include/raylib_amd.h RaylibAMD_TraceRays), on the renderer's own walks -- Traverse (the binary
// tree), Traverse4 (the 4-wide grid nodes) and NodeStep8 / LeafStep8 on the pool kernel's Trav state (the 8-wide tree).  rl_query.hip includes this file
// and instantiates the kernels; the other units see the declaration, the records and the instance list of rl_kernels.h, so that the render
// kernels stay the code they were (tools/isa_equivalence.py).
//
// One ray per lane.  A wave takes RL_QUERY_CHUNK rays at a time from a global counter: incoherent rays differ in step counts by orders of magnitude, and a
// static ray-per-thread grid would leave a wave waiting for its slowest lane while other waves have run dry.  On the binary and grid trees a lane walks one
// ray to its end (Traverse / Traverse4 are whole walks); on the 8-wide tree a lane whose ray is done takes the chunk's next ray between two steps.
//
// The interval [tMin, tMax]: the walk starts with "best" at the float above tMax, so the triangle test (t >= tMin, t < best) takes a hit at exactly tMax,
// as Triangle::Hit does, and every box beyond tMax is culled.  A sphere's interval is open (Sphere::Hit: t_min < t < t_max): the walk hands its sphere test
// tMax as that open end (Traverse's OPEN, SphereHitBelow), so a sphere at exactly tMax is never a candidate.  (Accepting it and dropping it after the walk lost
// a cube at that same t, which is in range -- a cube's interval is closed -- but is taken only if nearer than the best so far:
// tests/test_gpu_analytic_edges.py.)  A NaN bound makes every comparison false: a miss.
// tMin < 0 is raised to +0 (QueryTMin).  A triangle at exactly tMin counts: this unit widens the candidate rule's "own box ends before tMin" (RL_OWN_BOX_WIDEN_TMIN, rl_dev_walk.h OwnBoxPassBox).
// (RL_QUERY_CHUNK, the rays a wave takes per atomic on the global counter: rl_kernels.h)
#ifndef RL_QUERY_REFILL
#define RL_QUERY_REFILL 8        /* 8-wide walk: idle lanes of a wave before it hands out new rays between steps */
#endif

__device__ __forceinline__ float NextUpF(float x)
{
	if (!(x < INFINITY)) return x;                  // +inf, NaN
	if (x == 0.0f) return __int_as_float(1);        // +-0 -> the least positive denormal
	const int b = __float_as_int(x);
	return __int_as_float(x > 0.0f ? b + 1 : b - 1);
}

// A query never reports a hit behind the origin: tMin < 0 is read as +0 (include/raylib_amd.h).  The slack of the candidate rule (t * RL_CANDIDATE_SLACK >= the
// entry into the triangle's own box) and of the widened box tests (tf * widen < tn) is a factor above 1, which moves a negative t the wrong way.  A comparison,
// not fmaxf: a NaN stays a NaN and gives a miss; -0.0 compares as 0.
__device__ __forceinline__ float QueryTMin(float tMin) { return tMin < 0.0f ? 0.0f : tMin; }

// the record of one finished ray
template <int KIND, bool PRIMS>
__device__ __forceinline__ void QueryStore(const DSceneView& S, V3 o, V3 d, const HitRec& h, uint32_t i, void* __restrict__ out,
                                           int32_t* __restrict__ outPrim, const int32_t* __restrict__ slotIndex, Counters& c)
{
	const uint32_t kind = PRIMS ? ((uint32_t)h.tri) >> 28 : 0u;
	const bool hit = h.tri >= 0;
	if (KIND == RL_QK_ANY) { ((uint32_t*)out)[i] = hit ? 1u : 0u; return; }
	const int32_t prim = !hit ? -1 : kind != 0u ? h.tri : slotIndex ? slotIndex[h.tri] : h.tri;
	if (KIND == RL_QK_CLOSEST) {
		// (the 16-byte record as one store; the 64-byte shading record is not fetched)
		const float4 r = hit ? make_float4(h.t, __int_as_float(prim), kind == 0u ? h.a : 0.0f, kind == 0u ? h.b : 0.0f) : make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f);
		((float4*)out)[i] = r;
		return;
	}
	DHitOut r; memset(&r, 0, sizeof(r)); r.material = -1;
	if (hit) {   // as k_closest_hit
		Surf s;
		const int material = BuildSurface<PRIMS>(S, o, d, h, s, false, c);
		r.hit = 1; r.t = s.t;
		r.p[0] = s.p.x; r.p[1] = s.p.y; r.p[2] = s.p.z;
		r.n[0] = s.n.x; r.n[1] = s.n.y; r.n[2] = s.n.z;
		r.paramU = s.U; r.paramV = s.V; r.material = material;
	}
	((DHitOut*)out)[i] = r;
	if (outPrim) outPrim[i] = prim;
}

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int KIND, int STACK, bool PRIMS>
__global__ void __launch_bounds__(RL_BLOCK)
k_query(const DSceneView S, const float4* __restrict__ rays, uint32_t n, float rayTime, void* __restrict__ out, int32_t* __restrict__ outPrim,
        const int32_t* __restrict__ slotIndex, unsigned int* __restrict__ rayCounter, unsigned long long* __restrict__ counters)
{
	static_assert(TREE == 2 || TREE == 4 || TREE == 8, "tree");
	static_assert(TREE == 2 || !PRIMS, "spheres and cubes are walked on the binary tree only");
	RL_TEX_PROLOGUE(S);
	RL_MATH_PROLOGUE();
	// ANY stops at the first accepted candidate -- not in the instances with spheres and cubes (RaylibAMDQueryPlan's `early`, csrc/rl_plan.cc)
	constexpr bool EARLY = KIND == RL_QK_ANY && !PRIMS;
	__shared__ int s_stack[(TREE == 8 ? RL_POOL8_LSTACK : STACK) * RL_BLOCK];
	int* stk = s_stack + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	if constexpr (TREE != 8) {
		for (;;) {
			uint32_t base = 0u;
			if (lane == 0u) base = atomicAdd(rayCounter, RL_QUERY_CHUNK);
			base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
			if (base >= n) break;
			for (uint32_t k = 0; k < RL_QUERY_CHUNK; k += 64u) {
				const uint32_t i = base + k + lane;
				if (i < n) {
					const float4* rp = rays + 2u * (size_t)i;   // (64-bit offset: n may reach 2^31 - 1)
					const float4 r0 = GLoadF4(rp, 0), r1 = GLoadF4(rp, 1);
					const V3 o = v3(r0.x, r0.y, r0.z), d = v3(r1.x, r1.y, r1.z);
					const float tMin = QueryTMin(r0.w), tMax = r1.w;
					HitRec h;
					if constexpr (TREE == 2) Traverse<STACK, EARLY, PRIMS, PRIMS>(S, o, d, rayTime, tMin, h, stk, c, NextUpF(tMax), tMax < FLT_MAX ? tMax : FLT_MAX);   // (a NaN tMax: FLT_MAX, and nothing is below the NaN bound)
					else Traverse4<STACK, EARLY, false, false>(S, o, d, rayTime, tMin, h, stk, c, nullptr, NextUpF(tMax));
					QueryStore<KIND, PRIMS>(S, o, d, h, i, out, outPrim, slotIndex, c);
				}
			}
		}
	} else {
		// the 8-wide walk as the pool kernel runs it: its octant table, the LDS part of the stack of groups, the private rest
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
		uint32_t my = NONE;                      // this lane's ray
		float tMin = 0.0f;
		Trav T;
		T.o = T.d = T.inv = v3s(0.0f); T.rayTime = rayTime; T.nx = T.ny = T.nz = false; T.anyhit = EARLY;
		T.best.t = INFINITY; T.best.a = T.best.b = 0.0f; T.best.tri = -1; T.cur = 0; T.sp = 0; T.leafI = 0;
		T.gx = T.gy = T.tx = T.ty = T.tz = T.oct = 0u; T.m8x = T.m8y = T.m8z = 0u;
		uint32_t next = 0u, end = 0u;            // the wave's chunk (wave-uniform)
		bool drained = false;                    // the global counter is past n (wave-uniform)
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
						T.best.t = NextUpF(r1.w); T.best.tri = -1; T.best.a = 0.0f; T.best.b = 0.0f;
						T.cur = 0; T.sp = 0; T.leafI = 0;
						// the root as a group of one: base 0, imask 1, its bit at the visiting position of slot 0
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
				else fin = LeafStep8<false>(S, T, tMin, stk, ovf, c, G8);
				if (fin) { QueryStore<KIND, false>(S, T.o, T.d, T.best, my, out, outPrim, slotIndex, c); my = NONE; }
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
