// k_gbuffer: the primary-hit G-buffer (include/raylib_amd.h RaylibAMD_RenderGBuffer, statements G1 to G6) -- k_aov's camera front end and debug-mode
// arithmetic on k_query's driver and walks.  rl_gbuffer.hip includes this file and instantiates the kernels; the other units see the declaration, the
// records and the instance list of rl_kernels.h, so that every other kernel stays the code it was (tools/isa_equivalence.py).
//
// One pixel per lane.  A wave takes RL_QUERY_CHUNK pixel slots at a time from a global counter; slot i is pixel p = i & 63 of the 8 x 8 cell i >> 6, as
// k_aov numbers them, so that the 64 lanes of a wave start on one cell: coherent primary rays, and rows of eight 16-byte stores.  The counter counts CELLS
// (a chunk is RL_QUERY_CHUNK / 64 of them): a frame of 2^31 - 1 pixels one pixel wide has 2^34 slots, and 2^28 cells.  A slot outside the frame takes no
// ray and writes nothing.  On the binary and grid trees a lane walks its ray to the end (Traverse / Traverse4 are whole walks); on the 8-wide tree a lane
// whose ray is done takes the chunk's next slot between two steps, as in k_query.
//
// The hit is the render's (G2): the search starts at INFINITY, rayTMin is the walk's tMin as it stands, and this unit does not widen the own-box rule
// (rl_dev_walk.h RL_OWN_BOX_WIDEN_TMIN) -- k_aov's Traverse call on the binary tree, the pool kernel's steps on the 8-wide one.
//
// The finish, once per hit: BuildSurface and LoadMat once, then the planes asked for; the mask is a kernel argument, so every branch on it is uniform.
// BuildSurface's flag is `basis`: it adds the tangent frame and changes nothing else of the record, so the surface plane (QueryStore passes false: its
// record has no frame) and the colour planes (k_aov passes true) are one record; the frame is built when the micro normal, its one reader, is asked for.
// The albedo plane of a mirror-like surface is the albedo of what the reflection meets (k_aov, reference renderer.cc:66-78): a second walk on the same
// tree from the same lane, and only then.
#ifndef RL_QUERY_REFILL
#define RL_QUERY_REFILL 8        /* 8-wide walk: idle lanes of a wave before it hands out new slots between steps (k_query's) */
#endif
static_assert(RL_QUERY_CHUNK % 64u == 0u && RL_QUERY_CHUNK >= 64u, "a chunk is whole cells");

__device__ __forceinline__ void GBufferStoreColour(float4* __restrict__ plane, uint32_t pix, V3 v) { plane[pix] = make_float4(v.x, v.y, v.z, 1.0f); }

// A pixel that hit nothing: every plane asked for (G3)
__device__ __forceinline__ void GBufferMiss(const DGBuffer& G, uint32_t pix)
{
	if (G.mask & RL_GB_HIT) G.hit[pix] = make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f);
	if (G.mask & RL_GB_SURFACE) { DHitOut r; memset(&r, 0, sizeof(r)); r.material = -1; G.surface[pix] = r; }
	const V3 z = v3s(0.0f);
	if (G.mask & RL_GB_ALBEDO) GBufferStoreColour(G.albedo, pix, z);
	if (G.mask & RL_GB_SURFACE_NORMAL) GBufferStoreColour(G.surfaceNormal, pix, z);
	if (G.mask & RL_GB_MICRO_NORMAL) GBufferStoreColour(G.microNormal, pix, z);
	if (G.mask & RL_GB_TEXCOORD) GBufferStoreColour(G.texcoord, pix, z);
	if (G.mask & RL_GB_EMISSION) GBufferStoreColour(G.emission, pix, z);
}

// A pixel's hit: every plane asked for but, where a follow-up is due, the albedo.  True: the albedo plane was asked for and the surface is mirror-like --
// `albedo` is the surface's own (what the plane gets when the reflection meets nothing) and (p2, d2) the reflected ray.
template <bool PRIMS>
__device__ __forceinline__ bool GBufferHit(const DSceneView& S, const DGBuffer& G, V3 o, V3 d, const HitRec& h, uint32_t pix, const int32_t* __restrict__ slotIndex, Counters& c,
                                           V3& albedo, V3& p2, V3& d2)
{
	const uint32_t kind = PRIMS ? ((uint32_t)h.tri) >> 28 : 0u;
	if (G.mask & RL_GB_HIT) {   // QueryStore's CLOSEST record
		const int32_t prim = kind != 0u ? h.tri : slotIndex ? slotIndex[h.tri] : h.tri;
		G.hit[pix] = make_float4(h.t, __int_as_float(prim), kind == 0u ? h.a : 0.0f, kind == 0u ? h.b : 0.0f);
	}
	if ((G.mask & ~RL_GB_HIT) == 0u) return false;
	Surf s;
	const int material = BuildSurface<PRIMS>(S, o, d, h, s, (G.mask & RL_GB_MICRO_NORMAL) != 0u, c);
	if (G.mask & RL_GB_SURFACE) {   // QueryStore's SURFACE record
		DHitOut r; memset(&r, 0, sizeof(r));
		r.hit = 1; r.t = s.t;
		r.p[0] = s.p.x; r.p[1] = s.p.y; r.p[2] = s.p.z;
		r.n[0] = s.n.x; r.n[1] = s.n.y; r.n[2] = s.n.z;
		r.paramU = s.U; r.paramV = s.V; r.material = material;
		G.surface[pix] = r;
	}
	if ((G.mask & RL_GB_COLOUR) == 0u) return false;
	const Mat m = LoadMat(S, material);
	if (G.mask & RL_GB_SURFACE_NORMAL) GBufferStoreColour(G.surfaceNormal, pix, v3s(0.5f) + 0.5f * s.n);
	if (G.mask & RL_GB_MICRO_NORMAL) {
		V3 N = GetMicrosurfaceNormal(S, m, s, c);
		N = LocalToWorld(s, N);
		GBufferStoreColour(G.microNormal, pix, 0.5f * N + 0.5f);
	}
	if (G.mask & RL_GB_TEXCOORD) GBufferStoreColour(G.texcoord, pix, v3(s.U, s.V, 0.0f));
	if (G.mask & RL_GB_EMISSION) GBufferStoreColour(G.emission, pix, Emitted(S, m, s, c));
	if (G.mask & RL_GB_ALBEDO) {
		albedo = GetAlbedo(S, m, s.U, s.V, c);
		if (IsMirrorLike(S, m, s.U, s.V, c)) { p2 = s.p; d2 = reflect(d, s.n); return true; }
		GBufferStoreColour(G.albedo, pix, albedo);
	}
	return false;
}

// The end of a follow-up: the albedo of what the reflection met, or the surface's own
template <bool PRIMS>
__device__ __forceinline__ void GBufferFollowed(const DSceneView& S, const DGBuffer& G, V3 p2, V3 d2, const HitRec& h2, uint32_t pix, V3 albedo, Counters& c)
{
	if (h2.tri >= 0) {
		Surf s2;
		const Mat m2 = LoadMat(S, BuildSurface<PRIMS>(S, p2, d2, h2, s2, false, c));
		albedo = GetAlbedo(S, m2, s2.U, s2.V, c);
	}
	GBufferStoreColour(G.albedo, pix, albedo);
}

// slot `off` of the chunk that begins at cell `cell0` -> its pixel's (x, y); false: outside the frame
__device__ __forceinline__ bool GBufferPixel(const DGBuffer& G, uint32_t cell0, uint32_t off, uint32_t& x, uint32_t& y)
{
	const uint32_t cell = cell0 + (off >> 6), p = off & 63u;
	if (cell >= G.numCells) return false;
	x = (cell % G.cellsX) * 8u + (p & 7u); y = (cell / G.cellsX) * 8u + (p >> 3);
	return x < G.width && y < G.height;
}
// G1: pixel (x, y)'s sample-0 camera ray, as k_aov generates it
__device__ __forceinline__ void GBufferRay(const DGBuffer& G, uint32_t x, uint32_t y, V3& o, V3& d, float& rayTime)
{
	Rng g; g.s = raylib_rng_begin(G.seed, y * G.width + x, 0);
	CameraRay(G.camera, (float)x / (float)G.width, (float)y / (float)G.height, g, o, d, rayTime);
}

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int STACK, bool PRIMS>
__global__ void __launch_bounds__(RL_BLOCK)
k_gbuffer(const DSceneView S, const DGBuffer G, const int32_t* __restrict__ slotIndex, unsigned int* __restrict__ cellCounter, unsigned long long* __restrict__ counters)
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
				if (!hit) { GBufferMiss(G, pix); continue; }
				V3 albedo, p2, d2;
				if (GBufferHit<PRIMS>(S, G, o, d, h, pix, slotIndex, c, albedo, p2, d2)) {
					HitRec h2;
					if constexpr (TREE == 2) Traverse<STACK, false, PRIMS>(S, p2, d2, rayTime, G.rayTMin, h2, stk, c);
					else Traverse4<STACK, false, false, false>(S, p2, d2, rayTime, G.rayTMin, h2, stk, c);
					GBufferFollowed<PRIMS>(S, G, p2, d2, h2, pix, albedo, c);
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
		uint32_t my = NONE;                      // this lane's pixel, y * width + x
		bool follow = false;                     // ... and its ray is the albedo plane's follow-up, with the surface's own albedo kept here
		V3 albedo = v3s(0.0f);
		const float tMin = G.rayTMin;
		Trav T;
		T.o = T.d = T.inv = v3s(0.0f); T.rayTime = 0.0f; T.nx = T.ny = T.nz = false; T.anyhit = false;
		T.best.t = INFINITY; T.best.a = T.best.b = 0.0f; T.best.tri = -1; T.cur = 0; T.sp = 0; T.leafI = 0;
		T.gx = T.gy = T.tx = T.ty = T.tz = T.oct = 0u; T.m8x = T.m8y = T.m8z = 0u;
		// a ray's start: the reciprocals, the search at INFINITY (the render's), the root as a group of one -- base 0, imask 1, its bit at the visiting position of slot 0
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
						my = y * G.width + x; follow = false;
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
				if (fin) {
					if (follow) { GBufferFollowed<false>(S, G, T.o, T.d, T.best, my, albedo, c); my = NONE; }
					else if (T.best.tri < 0) { GBufferMiss(G, my); my = NONE; }
					else {
						V3 p2, d2;
						if (GBufferHit<false>(S, G, T.o, T.d, T.best, my, slotIndex, c, albedo, p2, d2)) { follow = true; begin(p2, d2); }
						else my = NONE;
					}
				}
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
