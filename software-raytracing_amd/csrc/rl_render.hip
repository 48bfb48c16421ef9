// HIP kernels + device runtime of the MI355X raylib (gfx950, wave64): the main translation unit.
//
// Replaces, on the device, the reference's per-pixel render loop and everything it
// calls (reference render/renderer.cc:62-271, geom/bvh.cc:82-107, geom/aabb.h:14-55,
// geom/triangle.cc:18-58, geom/hit.cc:6-30, render/material.cc, render/brdf.h,
// render/camera.h:44-53, render/texture.cc:30-53, core/random.cc:3-50):
//
//   k_trace    persistent "megakernel": every lane owns one camera sample (a path)
//              at a time and runs one bounce per loop trip; lanes whose path ended
//              are refilled at the top of the loop from a global job counter using a
//              wave64 __ballot + prefix rank (one atomic per wave and trip), so waves
//              stay full while path lengths differ.  Traversal is iterative on ONE
//              flat BVH2 with an LDS stack ([entry][lane], conflict free), ordered
//              near-first with t-shrinking -- it returns the reference's closest hit
//              (min t over all triangles) without the reference's both-children walk.
//   k_resolve  sums a pixel's samples IN SAMPLE ORDER (float addition is not
//              associative; the reference adds s = 0..SPP-1 sequentially,
//              renderer.cc:232-246) and applies the reciprocal-multiply mean.
//   k_aov      the debug render modes (renderer.cc:62-111).
//   k_closest_hit  rays in -> hit records out (tests).
//
// Radiance is folded exactly as the reference's recursion evaluates it
// (renderer.cc:139-151): per bounce the lane stores (reflectance, scatteringPdf,
// pdf, emitted) in a global path stack and, when the path ends, folds from the last
// vertex back to the camera, so every rounding step is the reference's.
//
// The device library is rl_dev_*.h; a kernel's body is an rl_k_*.inl file, and rl_kernels.h says which translation unit owns which kernel.  This
// unit owns the one-view k_trace, k_resolve and k_aov and the small kernels below: kernels only.  The host runtime that launches them is rl_rt_*.hip.

// ---- settings: this unit takes every default ----

// ---- the device library ----
#include "rl_kernels.h"

namespace rl {

// ---- kernel bodies ----
#define RL_VIEWS_TWIN 0
#include "rl_k_trace.inl"
#include "rl_k_resolve.inl"

// ---- progressive rendering (rl_kernels.h ProgressiveState; include/raylib_amd.h RaylibAMD_BeginProgressive) ----
// One pass's batch over EVERY cell of the frame (one wave = one 8x8 cell): a cell still sampled adds the batch's samples to its sums (the megakernel
// traced it: P.activeCells holds the session's list; or it lies outside the silhouette: P.cellEmpty), exactly as k_resolve does.  The pass's last batch
// then decides whether the cell stops (ProgressivePixelError, maximum over the wave) and writes every valid pixel of the row-major frame as its
// cell's sum * (1 / samples): the frame a one-shot render at that sample count would give, whatever touched the image since the last pass.
__global__ void __launch_bounds__(RL_BLOCK)
k_progressive_resolve(const DRenderParams P, const DSceneView S, const SkyRot R, const SampleRGB* __restrict__ samples, const ProgressiveState st,
                      float4* __restrict__ out, int lastBatch)
{
	RL_MATH_PROLOGUE();
	const uint32_t numSlots = P.numLocalCells * 64u;
	const uint32_t slot = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (slot >= numSlots) return;   // (whole waves: numSlots is a multiple of 64)
	const uint32_t p = slot & 63u, cellLocal = slot >> 6;
	const uint32_t x = (cellLocal % P.cellsX) * 8u + (p & 7u), y = (cellLocal / P.cellsX) * 8u + (p >> 3);
	const bool valid = x < P.width && y < P.height;
	float4 a = st.sum[slot];
	uint32_t n;
	if (!st.stopped[cellLocal]) {
		n = P.sampleBegin + P.sampleCount;
		float s1 = 0.0f, s2 = 0.0f;
		if (valid) {
			s1 = st.s1[slot]; s2 = st.s2[slot];
			a = SumSlotBatch(P, S, R, samples, numSlots, slot, cellLocal, x, y, a, [&](float r, float g, float b) __attribute__((always_inline)) {
				const float L = dot(v3(r, g, b), v3(0.2126f, 0.7152f, 0.0722f));   // (k_pp_max's luminance)
				const float yv = L / (1.0f + L);
				s1 += yv; s2 += yv * yv;
			});
			st.sum[slot] = a; st.s1[slot] = s1; st.s2[slot] = s2;
		}
		if (lastBatch) {
			float e = valid ? ProgressivePixelError(s1, s2, n) : 0.0f;
			for (int off = 32; off > 0; off >>= 1) { const float o = __shfl_xor(e, off); e = e < o ? o : e; }   // (no NaN: the error is +inf instead)
			if (p == 0) {
				st.cellSamples[cellLocal] = n;
				if (ProgressiveCellStops(e, n, st.threshold, st.minSamples)) st.stopped[cellLocal] = 1;
			}
		}
	} else n = st.cellSamples[cellLocal];
	if (lastBatch && valid) {
		const float k = rtm::rcp1_((float)n);
		out[(size_t)y * P.width + x] = make_float4(a.x * k, a.y * k, a.z * k, 1.0f);
	}
}

// The session's lists after a pass, in one workgroup: `live` (every cell still sampled, ascending) loses the cells that stopped, in place and in order,
// and `trace` becomes the live cells inside the silhouette, in order -- the megakernel's job list of the next pass, bands of whole cells as before.
// counts: [0] live cells, [1] listed cells, [2..3] valid pixels of the live cells outside the silhouette (64 bits; the next pass's culled samples per sample).
__global__ void __launch_bounds__(RL_COMPACT_BLOCK)
k_progressive_compact(uint32_t* __restrict__ live, uint32_t* __restrict__ trace, const uint8_t* __restrict__ stopped, const uint8_t* __restrict__ empty,
                      uint32_t numLive, uint32_t width, uint32_t height, uint32_t cellsX, uint32_t* __restrict__ counts)
{
	constexpr uint32_t WAVES = RL_COMPACT_BLOCK / 64;
	__shared__ uint32_t sLive[WAVES], sTrace[WAVES];
	__shared__ unsigned long long sPx[WAVES];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	uint32_t doneLive = 0, doneTrace = 0;   // entries written by the chunks before (the same in every thread)
	unsigned long long px = 0;
	for (uint32_t base = 0; base < numLive; base += RL_COMPACT_BLOCK * RL_COMPACT_PER) {
		// a thread's RL_COMPACT_PER consecutive entries: all of the chunk is read before the barrier, and every entry moves to an index <= its own
		uint32_t c[RL_COMPACT_PER], keep = 0, listed = 0;
		#pragma unroll
		for (int k = 0; k < RL_COMPACT_PER; ++k) {
			const uint32_t i = base + t * RL_COMPACT_PER + (uint32_t)k;
			c[k] = i < numLive ? live[i] : 0u;
			if (i < numLive && !stopped[c[k]]) {
				keep |= 1u << k;
				if (!empty || !empty[c[k]]) listed |= 1u << k;
				else { const uint32_t cx = c[k] % cellsX, cy = c[k] / cellsX; px += (unsigned long long)min(8u, width - cx * 8u) * min(8u, height - cy * 8u); }
			}
		}
		const uint32_t nl = __popc(keep), nt = __popc(listed);
		uint32_t il = nl, it = nt;   // inclusive scan over the wave
		for (uint32_t off = 1; off < 64; off <<= 1) {
			const uint32_t ul = __shfl_up(il, off), ut = __shfl_up(it, off);
			if (lane >= off) { il += ul; it += ut; }
		}
		if (lane == 63) { sLive[wave] = il; sTrace[wave] = it; }
		__syncthreads();
		uint32_t ol = doneLive + il - nl, ot = doneTrace + it - nt;
		for (uint32_t w = 0; w < WAVES; ++w) {
			if (w < wave) { ol += sLive[w]; ot += sTrace[w]; }
			doneLive += sLive[w]; doneTrace += sTrace[w];
		}
		#pragma unroll
		for (int k = 0; k < RL_COMPACT_PER; ++k) {
			if (keep >> k & 1u) live[ol++] = c[k];
			if (listed >> k & 1u) trace[ot++] = c[k];
		}
		__syncthreads();   // (sLive / sTrace are re-used by the next chunk)
	}
	for (int off = 32; off > 0; off >>= 1) px += __shfl_down(px, off);
	if (lane == 0) sPx[wave] = px;
	__syncthreads();
	if (t == 0) {
		unsigned long long sum = 0;
		for (uint32_t w = 0; w < WAVES; ++w) sum += sPx[w];
		counts[0] = doneLive; counts[1] = doneTrace; counts[2] = (uint32_t)sum; counts[3] = (uint32_t)(sum >> 32);
	}
}

#include "rl_k_aov.inl"
#undef RL_VIEWS_TWIN

template <int STACK, bool PRIMS>
__global__ void __launch_bounds__(RL_BLOCK)
k_closest_hit(const DSceneView S, const float* __restrict__ rays, int n, float tMin, DHitOut* __restrict__ out)
{
	RL_TEX_PROLOGUE(S);
	RL_MATH_PROLOGUE();
	__shared__ int s_stack[STACK * RL_BLOCK];
	int* stk = s_stack + threadIdx.x;
	const int i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= n) return;
	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	const V3 o = ld3(rays + 6 * i), d = ld3(rays + 6 * i + 3);
	HitRec h;
	DHitOut r; memset(&r, 0, sizeof(r)); r.material = -1;
	if (Traverse<STACK, false, PRIMS>(S, o, d, 0.0f, tMin, h, stk, c)) {
		Surf s;
		const int material = BuildSurface<PRIMS>(S, o, d, h, s, false, c);
		r.hit = 1; r.t = s.t;
		r.p[0] = s.p.x; r.p[1] = s.p.y; r.p[2] = s.p.z;
		r.n[0] = s.n.x; r.n[1] = s.n.y; r.n[2] = s.n.z;
		r.paramU = s.U; r.paramV = s.V; r.material = material;
	}
	out[i] = r;
}

// Image2D::PostProcess, pass 1: maxWhiteLuminance = max(1, max_i luminance_i) (reference render/image.cc:62-72).
// Luminances <= 1 cannot change the result, and for floats >= 1 the ordering of the values is the ordering of
// their bit patterns, so one integer atomicMax per wave suffices; NaN compares false in the reference and is skipped.
__global__ void __launch_bounds__(RL_BLOCK)
k_pp_max(const float4* __restrict__ px, size_t n, unsigned int* __restrict__ whiteBits)
{
	float m = 1.0f;
	for (size_t i = (size_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * RL_BLOCK) {
		const float4 p = px[i];
		const float L = dot(v3(p.x, p.y, p.z), v3(0.2126f, 0.7152f, 0.0722f));
		if (m < L) m = L;
	}
	for (int off = 32; off > 0; off >>= 1) { const float o = __shfl_down(m, off); if (m < o) m = o; }
	if ((threadIdx.x & 63) == 0 && m > 1.0f) atomicMax(whiteBits, __float_as_uint(m));
}

// pass 2 (reference render/image.cc:76-102)
__global__ void __launch_bounds__(RL_BLOCK)
k_pp_map(float4* __restrict__ px, size_t n, const unsigned int* __restrict__ whiteBits)
{
	RL_MATH_PROLOGUE();
	const size_t i = (size_t)blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= n) return;
	const float maxWhiteLuminance = __uint_as_float(*whiteBits);
	float4 p = px[i];
	V3 rgb = v3(p.x, p.y, p.z);
	const float luminanceOld = dot(rgb, v3(0.2126f, 0.7152f, 0.0722f));
	if (luminanceOld <= 0.0001f) rgb = v3s(0.0f);
	else {
		const float numerator = luminanceOld * (1.0f + (luminanceOld / (maxWhiteLuminance * maxWhiteLuminance)));
		const float luminanceNew = numerator / (1.0f + luminanceOld);
		rgb = rgb * (luminanceNew / luminanceOld);
	}
	// min(vec3(1), rgb) with std::min's operand order (core/vec3.h:151-156): (rgb < 1) ? rgb : 1
	rgb = v3(rgb.x < 1.0f ? rgb.x : 1.0f, rgb.y < 1.0f ? rgb.y : 1.0f, rgb.z < 1.0f ? rgb.z : 1.0f);
	const float K = 1.0f / 2.2f;
	p.x = rtm::pow_(rgb.x, K); p.y = rtm::pow_(rgb.y, K); p.z = rtm::pow_(rgb.z, K);
	px[i] = p;
}

// Test hooks: single functions of the hot path evaluated on arrays, so that tests can pin them one by one against
// the reference's outputs (Material::Scatter / ScatteringPdf / Emitted, Camera::GetCameraRay, Texture2D::Sample).
// Record layouts are those of oracle/ref_glue.cc (ref_scatter, ref_camera_rays, ref_texture_sample).
__global__ void __launch_bounds__(RL_BLOCK)
k_eval_scatter(const DSceneView S, int material, const float* __restrict__ in, int n, unsigned long long seed, float* __restrict__ out)
{
	RL_TEX_PROLOGUE(S);
	RL_MATH_PROLOGUE();
	const int i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= n) return;
	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	const float* a = in + 16 * i;
	const V3 d = ld3(a + 3);
	Surf s;
	s.t = a[7]; s.p = ld3(a + 8); s.n = ld3(a + 11); s.U = a[14]; s.V = a[15];
	{
		V3 T = (fabsf(s.n.x) > 0.9f) ? v3(0.0f, 1.0f, 0.0f) : v3(1.0f, 0.0f, 0.0f);
		V3 B = normalize(cross(T, s.n));
		T = normalize(cross(s.n, B));
		s.tangent = T; s.bitangent = B;
	}
	const Mat m = LoadMat(S, material);
	Rng g; g.s = raylib_rng_begin(seed, (uint32_t)i, 0);
	V3 refl = v3s(0.0f), outD = v3s(0.0f);
	float pdf = 0.0f, sp = 0.0f;
	const bool b = Scatter(S, m, d, s, g, c, refl, outD, pdf, sp);
	const V3 e = Emitted(S, m, s, c);
	float* o = out + 16 * i;
	o[0] = b ? 1.0f : 0.0f;
	o[1] = refl.x; o[2] = refl.y; o[3] = refl.z;
	// the reference leaves the scattered ray default-constructed (0) when a material does not fill it
	const bool wrote = (m.type != MAT_DIFFUSE_LIGHT);
	o[4] = wrote ? outD.x : 0.0f; o[5] = wrote ? outD.y : 0.0f; o[6] = wrote ? outD.z : 0.0f;
	o[7] = wrote ? s.p.x : 0.0f; o[8] = wrote ? s.p.y : 0.0f; o[9] = wrote ? s.p.z : 0.0f;
	o[10] = pdf; o[11] = b ? sp : 0.0f;
	o[12] = e.x; o[13] = e.y; o[14] = e.z;
	o[15] = (m.type == MAT_LAMBERTIAN || m.type == MAT_METAL || m.type == MAT_MICROFACET) ? 2.0f : (m.type == MAT_DIELECTRIC ? 1.0f : 0.0f);
}

__global__ void __launch_bounds__(RL_BLOCK)
k_eval_camera(const DCamera cam, const float* __restrict__ uv, int n, unsigned long long seed, float* __restrict__ out)
{
	RL_MATH_PROLOGUE();
	const int i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= n) return;
	Rng g; g.s = raylib_rng_begin(seed, (uint32_t)i, 0);
	V3 o, d; float t;
	CameraRay(cam, uv[2 * i], uv[2 * i + 1], g, o, d, t);
	float* r = out + 7 * i;
	r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z; r[6] = t;
}

__global__ void __launch_bounds__(RL_BLOCK)
k_eval_texture(const DSceneView S, int tex, int srgb, const float* __restrict__ uv, int n, float* __restrict__ out)
{
	RL_MATH_PROLOGUE();
	const int i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= n) return;
	const float4 p = TexFetch(S.textures, S.texels, tex, srgb != 0, uv[2 * i], uv[2 * i + 1]);
	out[4 * i] = p.x; out[4 * i + 1] = p.y; out[4 * i + 2] = p.z; out[4 * i + 3] = p.w;
}

// Test hook: evaluate one device math routine on an array (tests compare with the host libm bit for bit).
__global__ void __launch_bounds__(RL_BLOCK)
k_eval_math(int fn, const float* __restrict__ x, const float* __restrict__ y, int n, float* __restrict__ out)
{
	RL_MATH_PROLOGUE();
	const int i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= n) return;
	const float a = x[i], b = y ? y[i] : 0.0f;
	float r = 0.0f, s, c;
	switch (fn) {
		case 0: r = rtm::sin_(a); break;
		case 1: r = rtm::cos_(a); break;
		case 2: r = rtm::tan_(a); break;
		case 3: r = rtm::acos_(a); break;
		case 4: r = rtm::asin_(a); break;
		case 5: r = rtm::atan2_(a, b); break;
		case 6: r = rtm::exp_(a); break;
		case 7: r = rtm::log_(a); break;
		case 8: r = rtm::pow_(a, b); break;
		case 9: rtm::sincos_(a, &s, &c); r = s; break;
		case 10: rtm::sincos_(a, &s, &c); r = c; break;
		case 11: r = sqrtf(a); break;
		case 12: r = a / b; break;
		case 13: r = rtm::fmod1_(a); break;
		case 14: r = rtm::rcp1_(a); break;
		case 15: r = rtm::sqrt_(a); break;
		default: break;
	}
	out[i] = r;
}

// Test hook: the short exact sequences against the compiler's IEEE expansions, inside the product library.  out[0] = mismatching cases, out[1] = the
// smallest bit pattern of the swept operand with a mismatch.
//   which 0 / 1: rtm::rcp1_ / rtm::sqrt_ (rl_glibc_math.h) against 1.0f / x and sqrtf(x) on EVERY float bit pattern;
//   which 2: rtm::div_by_(a, b, RN(1 / b)) against a / b -- every bit pattern as the numerator of a set of divisors, and as the divisor of a set of
//            numerators, wherever div_by_'s stated conditions hold (rl_math.h; all significand PAIRS are tools/verify_fastdiv.hip's sweep: this one walks the
//            exponents, the signs and the edges of the conditions);
//   which 3: Barycentric() in its short form against the two divisions and the reference's test -- every bit pattern as X, as Y and as denom of a set of
//            (X, Y, denom) triples, with rden as the host makes it: same verdict, and the same two quotients bit for bit when inside.
__device__ __forceinline__ bool SameBits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }
__device__ __forceinline__ bool DivByHolds(float a, float b)
{
	const float ma = fabsf(a), mb = fabsf(b);
	if (!(mb >= 0x1p-126f && mb <= 0x1p126f)) return false;
	if (!(ma >= 0x1p-102f && ma <= FLT_MAX)) return false;
	const float q = fabsf(a / b);
	return q >= 0x1p-126f && q < 0x1p127f;
}
__device__ __forceinline__ bool BaryDiffers(float X, float Y, float denom)
{
	const float mag = fabsf(denom);
	float rden;
	if (denom == 0.0f || denom != denom) rden = __uint_as_float(0x7fc00000u);
	else if (mag >= 0x1p-62f && mag <= 0x1p125f) rden = 1.0f / denom;
	else return false;   // such a divisor clears DSceneView::fastBary: the whole scene takes the divisions
	float fa, fb, ea, eb;
	const bool f = Barycentric(true, X, Y, denom, rden, fa, fb), e = Barycentric(false, X, Y, denom, rden, ea, eb);
	return f != e || (f && !(SameBits(fa, ea) && SameBits(fb, eb)));
}
__global__ void __launch_bounds__(RL_BLOCK)
k_verify_exact_math(int which, unsigned long long* __restrict__ out)
{
	const unsigned long long tid = (unsigned long long)blockIdx.x * RL_BLOCK + threadIdx.x, n = (unsigned long long)gridDim.x * RL_BLOCK;
	unsigned long long bad = 0, first = ~0ull;
	// operands the sweeps pair every bit pattern with: ordinary values, the launch's and the triangles' kinds of constants, and the edges of the conditions
	const float fixedB[12] = { 3.0f, 1920.0f, 1080.0f, 0.1f, -7.0f, 3.14159274f, 9.5e10f, 2.4e-9f, 0x1.8p-62f, 0x1.fffffep125f, 0x1p-126f, 0x1p126f };
	const float fixedA[10] = { 1.0f, -3.3f, 1e-20f, 5e20f, 0x1p-102f, 0x1.fffffep-103f, 0x1.234568p-100f, 0.75f, 1919.0f, 0x1.fffffep127f };
	for (unsigned long long b = tid; b < (1ull << 32); b += n) {
		const float x = __uint_as_float((uint32_t)b);
		bool differs = false;
		if (which <= 1) {
			const float want = which == 0 ? 1.0f / x : __builtin_sqrtf(x);
			const float got = which == 0 ? rtm::rcp1_(x) : rtm::sqrt_(x);
			differs = !SameBits(want, got);   // a NaN must meet a NaN
		} else if (which == 2) {
			for (int k = 0; k < 12; ++k) { const float d = fixedB[k]; if (DivByHolds(x, d) && !SameBits(rtm::div_by_(x, d, 1.0f / d), x / d)) differs = true; }
			for (int k = 0; k < 10; ++k) { const float a = fixedA[k]; if (DivByHolds(a, x) && !SameBits(rtm::div_by_(a, x, 1.0f / x), a / x)) differs = true; }
		} else if (which == 4) {
			differs = !SameBits(rlm::acosf_t<true>(x), rlm::acosf_t<false>(x)) || !SameBits(rlm::tanf_t<true>(x), rlm::tanf_t<false>(x));
		} else {
			// (X, Y, denom) of ordinary hits, of hits on an edge and at a vertex, of misses by a hair, with tiny, huge and special members
			const float T[14][3] = { { 1.0e9f, 2.0e9f, 9.5e10f }, { -1.0e9f, -2.0e9f, -9.5e10f }, { 0.0f, 4.0e10f, 9.5e10f }, { -0.0f, 0.0f, 9.5e10f }, { 1e-3f, 9.4999e10f, 9.5e10f },
			                         { 3e-12f, 1.0f, 2.4e-9f }, { -3e-12f, 1.0e-10f, 2.4e-9f }, { 1e-30f, 1e-31f, 0x1p-62f }, { 5e-20f, 2e-21f, 0x1.8p-60f }, { 1e-42f, 1e-10f, 1e-9f },
			                         { 0x1p100f, 0x1p99f, 0x1p125f }, { 0x1.fffffep127f, 1.0f, 2.0f }, { 4.75e10f, 4.75e10f, 9.5e10f }, { 4.7500004e10f, 4.75e10f, 9.5e10f } };
			for (int k = 0; k < 14; ++k) {
				differs = differs || BaryDiffers(x, T[k][1], T[k][2]) || BaryDiffers(T[k][0], x, T[k][2]) || BaryDiffers(T[k][0], T[k][1], x);
				differs = differs || BaryDiffers(x, -T[k][1], -T[k][2]) || BaryDiffers(x, x, T[k][2]);
			}
		}
		if (differs) { ++bad; first = min(first, b); }
	}
	if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], first); }
}

// Raylib_DumpImageData's packing (reference render/image.cc:121-135: RGB, 12 bytes per pixel, row-major) on the device: 25 MB cross the bus instead of 33,
// and the host is left with a plain copy.  One thread packs four pixels: four 16-byte loads, three 16-byte stores.
__global__ void __launch_bounds__(RL_BLOCK)
k_pack_rgb(const float4* __restrict__ px, float4* __restrict__ out, float* __restrict__ outTail, size_t n)
{
	const size_t q = (size_t)blockIdx.x * RL_BLOCK + threadIdx.x;
	const size_t i = q * 4;
	if (i + 4 <= n) {
		const float4 a = px[i], b = px[i + 1], c = px[i + 2], d = px[i + 3];
		out[q * 3] = make_float4(a.x, a.y, a.z, b.x); out[q * 3 + 1] = make_float4(b.y, b.z, c.x, c.y); out[q * 3 + 2] = make_float4(c.z, d.x, d.y, d.z);
	} else {
		for (size_t k = i; k < n; ++k) { const float4 a = px[k]; outTail[3 * k] = a.x; outTail[3 * k + 1] = a.y; outTail[3 * k + 2] = a.z; }
	}
}

// The frame from the ranks' cell buffers (N > 1 behind Raylib_Render): cell c was rendered by rank c % N as its (c / N)-th cell (rl_kernels.h ScatterPlan).
__global__ void __launch_bounds__(RL_BLOCK)
k_scatter_cells(const float4* __restrict__ gather, float4* __restrict__ out, uint32_t width, uint32_t height, uint32_t cellsX, const ScatterPlan plan)
{
	const size_t i = (size_t)blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= (size_t)width * height) return;
	const uint32_t x = (uint32_t)(i % width), y = (uint32_t)(i / width);
	const uint32_t cell = (y >> 3) * cellsX + (x >> 3);
	const uint32_t rank = cell % plan.ranks, local = cell / plan.ranks;
	out[i] = gather[plan.offset[rank] + local * 64u + ((y & 7u) << 3) + (x & 7u)];
}

// ---- instances ----
RL_TRACE_INSTANCES(RL_K_TRACE)
RL_AOV_INSTANCES(RL_K_AOV)
template __global__ void k_closest_hit<32, true>(const DSceneView, const float* __restrict__, int, float, DHitOut* __restrict__);
template __global__ void k_closest_hit<64, true>(const DSceneView, const float* __restrict__, int, float, DHitOut* __restrict__);

} // namespace rl
