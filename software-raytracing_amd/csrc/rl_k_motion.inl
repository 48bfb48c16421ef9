// k_motion: the motion plane beside the hit plane (include/raylib_amd.h RaylibAMD_RenderMotion, statements T1 to T6) -- k_gbuffer's pixels, rays, walks and
// drivers with another finish.  rl_motion.hip includes rl_k_gbuffer.inl for GBufferPixel, GBufferRay and RL_QUERY_REFILL, makes no instance of k_gbuffer, then
// includes this file and instantiates the kernels; the other units see the declaration and the instance list of rl_kernels.h.
//
// The lanes are k_gbuffer's: one pixel per lane, slot i is pixel i & 63 of the 8 x 8 cell i >> 6, so both planes are written as rows of eight 16-byte stores.
// The finish, once per pixel: the hit record as k_gbuffer's GBufferHit stores it (T1), then the previous point (T2) -- for a triangle of the moved range its
// nine previous coordinates, 36 bytes gathered by the lane and read this once, not in the walk -- and its projection through the previous camera (T3, T4:
// rl_motion.h, which the host oracle compiles too).  No LDS beyond the walk's stack (and, on the 8-wide tree, its octant table).

// A pixel's end: the planes asked for.  hit: the walk found something (h); else the ray's direction is projected as the point at infinity
template <bool PRIMS>
__device__ __forceinline__ void MotionStore(const DGBuffer& G, const DMotion& M, V3 o, V3 d, bool hit, const HitRec& h, uint32_t pix, const int32_t* __restrict__ slotIndex)
{
	int32_t prim = -1;
	uint32_t kind = 0u;
	if (hit) {
		kind = PRIMS ? ((uint32_t)h.tri) >> 28 : 0u;
		prim = kind != 0u ? h.tri : slotIndex ? slotIndex[h.tri] : h.tri;
	}
	if (G.mask & RL_GB_HIT) {   // k_gbuffer's record
		if (hit) G.hit[pix] = make_float4(h.t, __int_as_float(prim), kind == 0u ? h.a : 0.0f, kind == 0u ? h.b : 0.0f);
		else G.hit[pix] = make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f);
	}
	if (!M.motion) return;
	const float of[3] = { o.x, o.y, o.z }, df[3] = { d.x, d.y, d.z };
	float P[3] = { df[0], df[1], df[2] };
	if (hit) {
		const int32_t k = prim - M.first;   // (a sphere's or a cube's prim is at least 2^28 and `first + count` at most the scene's triangles: outside)
		if (kind == 0u && k >= 0 && k < M.count) {
			const float* __restrict__ src = M.prevPositions + 9u * (size_t)k;
			float pp[9];
			for (int a = 0; a < 9; ++a) pp[a] = src[a];
			MotionTrianglePoint(pp, h.a, h.b, P);
		} else {
			MotionRayPoint(of, df, h.t, P);
		}
	}
	float r[3];
	const uint32_t status = MotionProject(M.prevCamera.origin, M.prevCamera.top_left, M.prevCamera.horizontal, M.prevCamera.vertical, (float)G.width, (float)G.height, hit, P, r);
	M.motion[pix] = make_float4(r[0], r[1], r[2], __uint_as_float(status));
}

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int STACK, bool PRIMS>
__global__ void __launch_bounds__(RL_BLOCK)
k_motion(const DSceneView S, const DGBuffer G, const DMotion M, const int32_t* __restrict__ slotIndex, unsigned int* __restrict__ cellCounter, unsigned long long* __restrict__ counters)
{
	static_assert(TREE == 2 || TREE == 4 || TREE == 8, "tree");
	static_assert(TREE == 2 || !PRIMS, "spheres and cubes are walked on the binary tree only");
	RL_TEX_PROLOGUE(S);
	RL_MATH_PROLOGUE();
	__shared__ int s_stack[(TREE == 8 ? RL_POOL8_LSTACK : STACK) * RL_BLOCK];
	int* stk = s_stack + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	constexpr uint32_t CHUNK_CELLS = RL_QUERY_CHUNK / 64u;
	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	if constexpr (TREE != 8) {
		for (;;) {
			uint32_t cell0 = 0u;
			if (lane == 0u) cell0 = atomicAdd(cellCounter, CHUNK_CELLS);
			cell0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cell0);
			if (cell0 >= G.numCells) break;
			for (uint32_t k = 0; k < RL_QUERY_CHUNK; k += 64u) {
				uint32_t x, y;
				if (!GBufferPixel(G, cell0, k + lane, x, y)) continue;
				const uint32_t pix = y * G.width + x;
				V3 o, d; float rayTime;
				GBufferRay(G, x, y, o, d, rayTime);
				HitRec h;
				bool hit;
				if constexpr (TREE == 2) hit = Traverse<STACK, false, PRIMS>(S, o, d, rayTime, G.rayTMin, h, stk, c);
				else hit = Traverse4<STACK, false, false, false>(S, o, d, rayTime, G.rayTMin, h, stk, c);
				MotionStore<PRIMS>(G, M, o, d, hit, h, pix, slotIndex);
			}
		}
	} else {
		// the 8-wide walk as k_gbuffer runs it: the octant table, the LDS part of the stack of groups, the private rest; a lane whose ray is done takes the
		// chunk's next slot between two steps
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
		uint32_t my = NONE;                      // this lane's pixel, y * width + x
		const float tMin = G.rayTMin;
		Trav T;
		T.o = T.d = T.inv = v3s(0.0f); T.rayTime = 0.0f; T.nx = T.ny = T.nz = false; T.anyhit = false;
		T.best.t = INFINITY; T.best.a = T.best.b = 0.0f; T.best.tri = -1; T.cur = 0; T.sp = 0; T.leafI = 0;
		T.gx = T.gy = T.tx = T.ty = T.tz = T.oct = 0u; T.m8x = T.m8y = T.m8z = 0u;
		// a ray's start, as k_gbuffer's
		auto begin = [&](V3 o, V3 d) {
			T.o = o; T.d = d;
			T.inv = ClampInv(v3(FastRcp(d.x), FastRcp(d.y), FastRcp(d.z)));
			T.nx = T.inv.x < 0.0f; T.ny = T.inv.y < 0.0f; T.nz = T.inv.z < 0.0f;
			T.best.t = INFINITY; T.best.tri = -1; T.best.a = 0.0f; T.best.b = 0.0f;
			T.cur = 0; T.sp = 0; T.leafI = 0;
			RaySetup8(T);
			T.gx = 0u; T.gy = (1u << (24u + T.oct)) | 1u; T.tx = T.ty = T.tz = 0u;
			c.rays++;
		};
		uint32_t cell0 = 0u, next = 0u, end = 0u;   // the wave's chunk: its first cell, the slots of it handed out, its slots (wave-uniform)
		bool drained = false;                       // the global counter is past the frame's cells (wave-uniform)
		for (;;) {
			unsigned long long idle = Ballot(my == NONE);
			if (!drained && idle != 0ull && (__popcll(idle) >= RL_QUERY_REFILL || idle == ~0ull)) {
				while (idle != 0ull) {
					if (next >= end) {
						uint32_t b = 0u;
						if (lane == 0u) b = atomicAdd(cellCounter, CHUNK_CELLS);
						b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
						if (b >= G.numCells) { drained = true; break; }
						cell0 = b; next = 0u; end = min(CHUNK_CELLS, G.numCells - b) * 64u;
					}
					const uint32_t take = min((uint32_t)__popcll(idle), end - next);
					const uint32_t rank = (uint32_t)__popcll(idle & laneLt);
					uint32_t x, y;
					if (my == NONE && rank < take && GBufferPixel(G, cell0, next + rank, x, y)) {
						my = y * G.width + x;
						V3 o, d;
						GBufferRay(G, x, y, o, d, T.rayTime);
						begin(o, d);
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
				if (fin) { MotionStore<false>(G, M, T.o, T.d, T.best.tri >= 0, T.best, my, slotIndex); my = NONE; }
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
