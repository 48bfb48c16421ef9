// k_sdf_rows, k_sdf_parity, k_sdf_dist: a signed distance field baked on the device (include/raylib_amd.h RaylibAMD_BakeDistanceField, statements V1 to V7).
// rl_sdf.hip includes this file behind rl_k_query.inl (NextUpF, QueryTMin and k_query's schedule are that file's) and rl_dev_boxwalk.h (the distance kernel's
// walk and its leaf test) and instantiates the kernels.  No point, ray or result record exists: a voxel's point and a row's ray are made from their indices (SdfCentre, V1), a lane
// writes its 4-byte value (and 4 bytes of outPrim), and the only scratch is the bit volumes of the sign axes.
//
//   k_sdf_rows    one row ray per lane (V3), k_query_all's COUNT walks without a list: the bound stays {NextUpF(tMax), -1}, every accepted crossing comes once,
//                 and each toggles, in the row's words, bit m = #{i : t_a(i) < t} -- the voxels it lies ahead of are the prefix i < m (t_a is monotone in i),
//                 so bit m flips the inside bits of that prefix once the parity kernel has run.  m == 0 lies ahead of no voxel and toggles nothing.
//   k_sdf_parity  per row, in place: bit i becomes the XOR of the toggle bits above i (V4), by the shift-XOR suffix within a word and a carry over the words.
//   k_sdf_dist    the point walk with k_nearest's CLOSEST leaves, its LDS stack and half-distance column, one 4 x 4 x 4 brick of voxels per wave (partial bricks masked) so
//                 that a wave's lanes walk the same nodes; a claim is RL_QUERY_CHUNK voxels' worth of bricks from one counter.  V2 and V5 at the store.

// (V1 -- SdfT, SdfCentre -- is rl_sdf.h's, which the host oracle compiles too)
// (an axis picked at run time reads the grid through selects: an indexed kernel argument would be copied to scratch)
#define RL_SDF_SEL(v, a) ((a) == 0 ? (v)[0] : (a) == 1 ? (v)[1] : (v)[2])

// One row of the launch: its ray (V3) and what its crossings need -- the axis' voxel size and count, and the row's first toggle word.
struct SdfRowRef { float spacing; uint32_t n; unsigned long long word; };
__device__ __forceinline__ SdfRowRef SdfRow(const DSdfGrid& G, uint32_t r, V3& o, V3& d)
{
	const int a = r < G.rowEnd[0] ? 0 : r < G.rowEnd[1] ? 1 : 2;
	const uint32_t row = r - (a == 0 ? 0u : a == 1 ? G.rowEnd[0] : G.rowEnd[1]);
	// the other two axes, the lower one first: (y, z), (x, z), (x, y)
	const uint32_t nb = a == 0 ? G.dims[1] : G.dims[0];
	const uint32_t ib = row % nb, ic = row / nb;
	const float cx = SdfCentre(G.origin[0], G.spacing[0], a == 0 ? 0u : ib);
	const float cy = SdfCentre(G.origin[1], G.spacing[1], a == 0 ? ib : a == 1 ? 0u : ic);
	const float cz = SdfCentre(G.origin[2], G.spacing[2], a == 2 ? 0u : ic);
	o = v3(a == 0 ? G.origin[0] : cx, a == 1 ? G.origin[1] : cy, a == 2 ? G.origin[2] : cz);
	d = v3(a == 0 ? 1.0f : 0.0f, a == 1 ? 1.0f : 0.0f, a == 2 ? 1.0f : 0.0f);
	SdfRowRef R;
	R.spacing = RL_SDF_SEL(G.spacing, a); R.n = RL_SDF_SEL(G.dims, a);
	R.word = RL_SDF_SEL(G.wordBase, a) + (unsigned long long)row * RL_SDF_SEL(G.words, a);
	return R;
}

// Behind an accepted crossing at parameter t: its toggle bit m = #{i < n : t_a(i) < t}.  A float guess, then comparisons against the V1 expression itself
// (t_a does not decrease in i, so the count is the first index whose t_a is not below t).  m == 0 lies ahead of no voxel.
__device__ __forceinline__ void SdfToggle(const SdfRowRef& R, uint32_t* __restrict__ bits, float t)
{
	const float f = t / R.spacing;
	uint32_t m = f >= (float)R.n ? R.n : (f > 0.0f ? (uint32_t)f : 0u);
	while (m < R.n && SdfT(R.spacing, m) < t) ++m;
	while (m > 0u && !(SdfT(R.spacing, m - 1u) < t)) --m;
	if (m > 0u) atomicXor(bits + (R.word + (m >> 5)), 1u << (m & 31u));
}

// the test of one triangle, as rl_k_multihit.inl's: true when it was accepted, with `best` = {t, b1, b2, slot} of it
__device__ __forceinline__ bool SdfRowTest(const DSceneView& S, const Tri& TT, int slot, V3 o, V3 d, V3 inv /* exact 1/d */, float tMin, HitRec& best, bool alpha, Counters& c)
{
	RL_TRIANGLE_TEST(S, TT, slot, o, d, tMin, best, alpha, OwnBoxPass(TT.v0, TT.v1, TT.v2, o, inv, tMin, t), true, c, RL_NESTED)
	return false;
}

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int STACK>
__global__ void __launch_bounds__(RL_BLOCK)
k_sdf_rows(const DSceneView S, const DSdfGrid G, uint32_t n, uint32_t* __restrict__ bits, unsigned int* __restrict__ rowCounter, unsigned long long* __restrict__ counters)
{
	static_assert(TREE == 2 || TREE == 8, "tree");
	RL_TEX_PROLOGUE(S);
	RL_MATH_PROLOGUE();
	__shared__ int s_stack[(TREE == 8 ? RL_POOL8_LSTACK : STACK) * RL_BLOCK];
	int* stk = s_stack + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	const float tMin = QueryTMin(0.0f), bound0 = NextUpF(FLT_MAX);
#define RL_SDF_BOUND(best_) { (best_).t = bound0; (best_).tri = -1; (best_).a = 0.0f; (best_).b = 0.0f; }
	if constexpr (TREE == 2) {
		for (;;) {
			uint32_t base = 0u;
			if (lane == 0u) base = atomicAdd(rowCounter, RL_QUERY_CHUNK);
			base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
			if (base >= n) break;
			for (uint32_t k = 0; k < RL_QUERY_CHUNK; k += 64u) {
				const uint32_t i = base + k + lane;
				if (i >= n) continue;
				V3 o, d;
				const SdfRowRef R = SdfRow(G, i, o, d);
				// Traverse's walk (rl_dev_walk.h) with the toggle behind its triangle test
				c.rays++;
				const V3 inv = ExactInv(d);
				const bool nx = inv.x < 0.0f, ny = inv.y < 0.0f, nz = inv.z < 0.0f;
				HitRec best;
				RL_SDF_BOUND(best)
				int sp = 0, cur = 0;
				const int DONE = 0x7fffffff;
				for (;;) {
					while (cur >= 0 && cur != DONE) {
						const float4* np = (const float4*)(S.nodes + cur);
						const float4 q0 = np[0], q1 = np[1], q2 = np[2];
						const int4 kk = ((const int4*)np)[3];
						c.nodes++;
						float tl, tr;
						const float tmx = fminf(best.t, FLT_MAX);
						bool hl = Slab(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, o, inv, nx, ny, nz, tMin, tmx, tl);
						bool hr = Slab(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, o, inv, nx, ny, nz, tMin, tmx, tr);
						hl = hl && (kk.x != DNODE_EMPTY);
						hr = hr && (kk.y != DNODE_EMPTY);
						if (hl && hr) {
							const bool leftFirst = tl <= tr;
							const int nearC = leftFirst ? kk.x : kk.y, farC = leftFirst ? kk.y : kk.x;
							if (sp < STACK) { stk[sp * RL_BLOCK] = farC; ++sp; }
							cur = nearC;
						} else if (hl) cur = kk.x;
						else if (hr) cur = kk.y;
						else if (sp == 0) cur = DONE;
						else { --sp; cur = stk[sp * RL_BLOCK]; }
					}
					if (cur == DONE) break;
					{
						const LeafRef F = DecodeLeaf(cur);
						for (int j = 0; j < F.count; ++j) {
							const Tri TT = LoadTri(S, F.first + j);
							c.tris++;
							if (SdfRowTest(S, TT, F.first + j, o, d, inv, tMin, best, F.alpha, c)) { SdfToggle(R, bits, best.t); RL_SDF_BOUND(best) }
						}
					}
					if (sp == 0) break;
					--sp;
					cur = stk[sp * RL_BLOCK];
				}
			}
		}
	} else {
		// the 8-wide walk on k_query's schedule: the octant table, the stack of groups
		__shared__ unsigned char s_perm[8 * 256];
		for (uint32_t k = threadIdx.x; k < 8u * 256u; k += RL_BLOCK) {
			const uint32_t m = k >> 8, y = k & 255u;
			uint32_t r = 0;
			for (uint32_t bb = 0; bb < 8u; ++bb) if ((y >> bb) & 1u) r |= 1u << (bb ^ m);
			s_perm[k] = (unsigned char)r;
		}
		__syncthreads();
		constexpr int G8 = RL_POOL8_LSTACK / 2, GMAX8 = STACK / 2;
		// (the rest of the stack of groups, which k_query keeps private, in LDS as well: a lane's words back to back, as NodeStep8 indexes them -- no scratch)
		__shared__ int s_ovf[(STACK - RL_POOL8_LSTACK) * RL_BLOCK];
		int* ovf = s_ovf + threadIdx.x * (STACK - RL_POOL8_LSTACK);
		const unsigned long long laneLt = (1ull << lane) - 1ull;
		constexpr uint32_t NONE = 0xffffffffu;
		uint32_t my = NONE;
		SdfRowRef R; R.spacing = 1.0f; R.n = 0u; R.word = 0ull;
		Trav T;
		T.o = T.d = T.inv = v3s(0.0f); T.rayTime = 0.0f; T.nx = T.ny = T.nz = false; T.anyhit = false;
		T.best.t = INFINITY; T.best.a = T.best.b = 0.0f; T.best.tri = -1; T.cur = 0; T.sp = 0; T.leafI = 0;
		T.gx = T.gy = T.tx = T.ty = T.tz = T.oct = 0u; T.m8x = T.m8y = T.m8z = 0u;
		uint32_t next = 0u, end = 0u;
		bool drained = false;
		for (;;) {
			unsigned long long idle = Ballot(my == NONE);
			if (!drained && idle != 0ull && (__popcll(idle) >= RL_QUERY_REFILL || idle == ~0ull)) {
				while (idle != 0ull) {
					if (next >= end) {
						uint32_t b = 0u;
						if (lane == 0u) b = atomicAdd(rowCounter, RL_QUERY_CHUNK);
						b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
						if (b >= n) { drained = true; break; }
						next = b; end = min(b + RL_QUERY_CHUNK, n);
					}
					const uint32_t take = min((uint32_t)__popcll(idle), end - next);
					const uint32_t rank = (uint32_t)__popcll(idle & laneLt);
					if (my == NONE && rank < take) {
						my = next + rank;
						R = SdfRow(G, my, T.o, T.d);
						T.inv = ClampInv(v3(FastRcp(T.d.x), FastRcp(T.d.y), FastRcp(T.d.z)));
						T.nx = T.inv.x < 0.0f; T.ny = T.inv.y < 0.0f; T.nz = T.inv.z < 0.0f;
						RL_SDF_BOUND(T.best)
						T.cur = 0; T.sp = 0; T.leafI = 0;
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
				else {
					// LeafStep8's pick (rl_dev_pool.h): the lowest hit leaf child, its next triangle
					const uint32_t lc = (uint32_t)__ffs((int)(T.ty & 0xffu)) - 1u;
					const uint32_t k = (T.ty >> 8) & 3u;
					const uint32_t nib = (T.tz >> (4u * lc)) & 15u;
					const int slot = (int)(T.tx + (uint32_t)__popc(T.tz & ((1u << (4u * lc)) - 1u)) + k);
					const bool alpha = ((T.ty >> (16u + lc)) & 1u) != 0u;
					if ((nib >> (k + 1u)) != 0u) T.ty += 0x100u;
					else { T.ty &= ~0x300u; T.ty &= T.ty - 1u; }
					c.tris++;
					const Tri TT = LoadTri(S, slot);
					if (SdfRowTest(S, TT, slot, T.o, T.d, ExactInv(T.d), tMin, T.best, alpha, c)) { SdfToggle(R, bits, T.best.t); RL_SDF_BOUND(T.best) }
					fin = Next8(T, stk, ovf, G8);
				}
				if (fin) my = NONE;
			}
		}
	}
#undef RL_SDF_BOUND
	if (counters) {   // wave reduction, one atomic per wave and counter
		const uint32_t vals[5] = { c.rays, c.nodes, c.tris, c.shaded, c.texels };
		for (int k = 0; k < 5; ++k) {
			unsigned long long v = vals[k];
			for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
			if (lane == 0u && v) atomicAdd(&counters[k], v);
		}
	}
}

// Toggle bits into inside bits, in place, one row per thread: inside(i) = XOR of the toggle bits j > i.  From the row's last word down: S = the word's
// inclusive suffix XOR (bit i: the bits i .. 31), flipped when the words above hold an odd number of bits; the word becomes S >> 1 with that carry as bit 31.
__global__ void __launch_bounds__(RL_BLOCK)
k_sdf_parity(const DSdfGrid G, uint32_t n, uint32_t* __restrict__ bits)
{
	const uint32_t r = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (r >= n) return;
	const int a = r < G.rowEnd[0] ? 0 : r < G.rowEnd[1] ? 1 : 2;
	const uint32_t row = r - (a == 0 ? 0u : a == 1 ? G.rowEnd[0] : G.rowEnd[1]);
	const uint32_t words = RL_SDF_SEL(G.words, a);
	uint32_t* w = bits + (RL_SDF_SEL(G.wordBase, a) + (unsigned long long)row * words);
	uint32_t carry = 0u;
	for (uint32_t k = words; k-- > 0u;) {
		const uint32_t x = w[k];
		uint32_t s = x;
		s ^= s >> 1; s ^= s >> 2; s ^= s >> 4; s ^= s >> 8; s ^= s >> 16;
		if (carry) s = ~s;
		w[k] = (s >> 1) | (carry << 31);
		carry ^= (uint32_t)__popc(x) & 1u;
	}
}

// ---- the distance walk: rl_dev_boxwalk.h's, with k_nearest's CLOSEST leaf test (the barycentrics it keeps are never read), on generated points ----
#ifndef RL_SDF_DIST32
#define RL_SDF_DIST32 2   /* bytes of box distance per stack entry, as RL_NEAREST_DIST32 / 64: the upper half of the float */
#endif
#ifndef RL_SDF_DIST64
#define RL_SDF_DIST64 2
#endif

// (template and kernel arguments: rl_kernels.h)
template <int TREE, int STACK, bool SIGNED>
__global__ void __launch_bounds__(RL_BLOCK)
k_sdf_dist(const DSceneView S, const DSdfGrid G, float* __restrict__ outDist, int32_t* __restrict__ outPrim, const uint32_t* __restrict__ bits,
           const int32_t* __restrict__ slotIndex, unsigned int* __restrict__ brickCounter, unsigned long long* __restrict__ counters)
{
	__shared__ int s_stack[STACK * RL_BLOCK];
	int* stk = s_stack + threadIdx.x;
	constexpr int DBYTES = STACK <= 32 ? RL_SDF_DIST32 : RL_SDF_DIST64;
	typedef NearestDist<DBYTES> Dist;
	__shared__ typename Dist::T s_dist[DBYTES != 0 ? STACK * RL_BLOCK : 1];
	typename Dist::T* dstk = s_dist + (DBYTES != 0 ? threadIdx.x : 0u);
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t cPoints = 0u, cNodes = 0u, cTris = 0u;
	const uint32_t bricksX = (G.dims[0] + 3u) >> 2, bricksY = (G.dims[1] + 3u) >> 2, bricksZ = (G.dims[2] + 3u) >> 2;
	const uint32_t numBricks = bricksX * bricksY * bricksZ;   // (<= 2^31 - 1 voxels: at most 2^29 + ... bricks, the ABI checked the product)
	constexpr uint32_t CLAIM = RL_QUERY_CHUNK / 64u;
	const bool takesPart = G.maxDist >= 0.0f && S.numTriangles > 0;   // (V7 refused a centre that is not finite)
	for (;;) {
		const uint32_t base = ClaimChunk(brickCounter, CLAIM, lane);
		if (base >= numBricks) break;
		for (uint32_t kb = 0; kb < CLAIM; ++kb) {
			const uint32_t brick = base + kb;
			if (brick >= numBricks) break;
			const uint32_t bx = brick % bricksX, byz = brick / bricksX, by = byz % bricksY, bz = byz / bricksY;
			const uint32_t vi = 4u * bx + (lane & 3u), vj = 4u * by + ((lane >> 2) & 3u), vk = 4u * bz + (lane >> 4);
			if (vi >= G.dims[0] || vj >= G.dims[1] || vk >= G.dims[2]) continue;   // a partial brick's lanes outside the grid
			++cPoints;
			const float p[3] = { SdfCentre(G.origin[0], G.spacing[0], vi), SdfCentre(G.origin[1], G.spacing[1], vj), SdfCentre(G.origin[2], G.spacing[2], vk) };
			NearestBest best; best.d = G.maxDist * G.maxDist; best.slot = -1; best.b1 = best.b2 = 0.0f;
			if (takesPart)
				PointWalk<TREE, STACK, DBYTES>(S, p, best.d, stk, dstk, cNodes,
				                               [&](int first, int count) { return NearestLeaf<RL_NK_CLOSEST>(S, p, first, count, best, slotIndex, cTris); });
			// V2, V5: the magnitude, then the sign from the inside-bit volumes of the sign axes
			float m = best.slot < 0 ? G.maxDist : rlm::sqrtf_(best.d);
			if constexpr (SIGNED) {
				const uint32_t idx[3] = { vi, vj, vk };
				const uint32_t rows[3] = { vk * G.dims[1] + vj, vk * G.dims[0] + vi, vj * G.dims[0] + vi };
				uint32_t votes = 0u, asked = 0u;
				for (int a = 0; a < 3; ++a) {
					if (!((G.axes >> a) & 1u)) continue;
					++asked;
					votes += (bits[G.wordBase[a] + (unsigned long long)rows[a] * G.words[a] + (idx[a] >> 5)] >> (idx[a] & 31u)) & 1u;
				}
				if (2u * votes > asked) m = -m;   // one axis: its bit; three: at least two of them
			}
			const size_t at = ((size_t)vk * G.dims[1] + vj) * G.dims[0] + vi;
			outDist[at] = m;
			if (outPrim) outPrim[at] = best.slot < 0 ? -1 : slotIndex ? slotIndex[best.slot] : best.slot;
		}
	}
	FoldWaveCounters(counters, cPoints, cNodes, cTris, lane);
}
