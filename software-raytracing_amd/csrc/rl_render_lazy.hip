// The leaf-list kernel's lazy-reflectance instance (k_trace_lazy), its hit-queue form (k_trace_lazy_hitq), the resolve that reads their lit-sample mask (k_resolve_lit) and the sweeps of its guards, as a translation
// unit of their own: instantiated beside the other k_trace instances, the lazy one changes how the compiler schedules two loops of the eager PLAIN instance, and
// the eager kernels must stay what they are (tools/isa_equivalence.py) -- the reason the views twins have their unit.

// ---- settings: every default but the sampler's ----
// The Beckmann sampler with the guard-free forms of logf, expf, sqrtf and 1 / x where its arguments cannot reach the guards (rl_dev_shade.h "the ranged sampler";
// swept by k_verify_sampler_ranged below).  Measured on this unit's kernel only: every other unit keeps the general sampler.
#define RL_SAMPLER_RANGED 1
// The normalisations and single square roots of a scattering event without sqrt_'s and rcp1_'s range guards, each behind one wave vote or a written bound
// (rl_dev_core.h "normalize without the two range guards"; swept by k_verify_normalize_ranged below).  Bits 1 | 2 | 4 | 8: the surface frame, the sampler's two
// normalisations, the recomputed half vector, the single-float sites.  As above, this unit's kernels only.
#ifndef RL_NORMALIZE_RANGED
#define RL_NORMALIZE_RANGED 15
#endif

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_lit_mask.h"
#include "rl_dev_litfold.h"

namespace rl {

// ---- the leaf-list kernel's lazy-reflectance instance (rl_dev_shade.h "lazy-reflectance instance"); its lit paths are finished by its own waves (rl_dev_litfold.h) ----
#define RL_VIEWS_TWIN 0
#define RL_LAZY_REFL 1
#include "rl_k_trace.inl"
#undef RL_LAZY_REFL
#undef RL_VIEWS_TWIN

// ---- its hit-queue form (k_trace_lazy_hitq): the idle lanes take camera rays that have been traced already.  In this unit, whose settings it shares ----
#include "rl_k_trace_hitq.inl"

// k_resolve (rl_k_resolve.inl) for a batch with a lit-sample mask: the same contract, one thread per slot.  A culled cell takes SumSlotBatch's branch as it is;
// every other slot adds its flagged samples, in sample order (LitMaskSum) -- the samples the mask leaves out are +0 and were never stored.
__global__ void __launch_bounds__(RL_BLOCK)
k_resolve_lit(const DRenderParams P, const DSceneView S, const SkyRot R, const SampleRGB* __restrict__ samples, float4* __restrict__ accum, float4* __restrict__ out,
              int firstBatch, int lastBatch, const DLitList LL)
{
	RL_MATH_PROLOGUE();
	const uint32_t numSlots = P.numLocalCells * 64u;
	const uint32_t slot = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (slot >= numSlots) return;
	const uint32_t p = slot & 63u, cellLocal = slot >> 6;
	const uint32_t cell = P.cellFirst + cellLocal * P.cellStride;
	const uint32_t x = (cell % P.cellsX) * 8u + (p & 7u), y = (cell / P.cellsX) * 8u + (p >> 3);
	const bool valid = x < P.width && y < P.height;
	float4 a = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
	if (valid) {
		if (!firstBatch) a = accum[slot];
		if (P.cellEmpty && P.cellEmpty[cellLocal]) a = SumSlotBatch(P, S, R, samples, numSlots, slot, cellLocal, x, y, a, [](float, float, float) __attribute__((always_inline)) {});
		else LitMaskSum(LL.mask, LL.maskWords, (const float*)samples, numSlots, slot, a.x, a.y, a.z);
		if (lastBatch) {
			const float k = rtm::rcp1_((float)P.spp);
			a.x *= k; a.y *= k; a.z *= k; a.w = 1.0f;
		} else {
			accum[slot] = a;
		}
	}
	if (lastBatch) {
		if (P.rowMajorOutput) { if (valid) out[(size_t)y * P.width + x] = a; }
		else out[slot] = valid ? a : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	}
}

// The scattering events both sweeps below are made from: event i's generator, its outgoing direction, the sampler's two draws and the roughness.  Returns the
// selector the edge choices cycle by.
__device__ __forceinline__ uint32_t LazySweepEvent(unsigned long long seed, uint32_t i, Rng& g, V3& Wo, float& u0, float& u1, float& rough)
{
	g.s = raylib_rng_begin(seed, i, 0);
	const uint32_t sel = i % 30030u;   // 2 * 3 * 5 * 7 * 11 * 13: the edge choices below cycle with coprime periods
	// Wo: a unit vector with a chosen z
	const uint32_t zk = sel % 11u;
	float z = 2.0f * Next(g) - 1.0f;
	if (zk < 8u) { const float e[8] = { 0.0f, 1.0f, -1.0f, 0x1p-1f, -0x1p-10f, 0x1p-24f, -0x1p-60f, 0x1p-126f }; z = e[zk]; }
	const float phi = 2.0f * RL_PI * Next(g), rxy = rtm::sqrt_(fmaxf(0.0f, 1.0f - z * z));
	float sphi, cphi; rtm::sincos_(phi, &sphi, &cphi);
	Wo = v3(rxy * cphi, rxy * sphi, z);
	const uint32_t uk = sel % 7u, vk = sel % 5u;
	u0 = Next(g); u1 = Next(g);
	if (uk < 3u) u0 = uk == 0u ? 0.0f : uk == 1u ? 1e-6f : 1.0f - 0x1p-24f;
	if (vk < 3u) u1 = vk == 0u ? 0.0f : vk == 1u ? 1e-6f : 1.0f - 0x1p-24f;
	const uint32_t rk = sel % 3u;
	rough = rk == 0u ? RL_LAZY_ROUGHNESS_MIN : rk == 1u ? RL_LAZY_ROUGHNESS_MAX : rtm::exp_(Next(g) * -10.0f * 0.69314718f);
	return sel;
}

// Test hook: LazyVertexSafe's claim, swept inside the product library.  Every thread builds scattering events from edge and random inputs -- Wo.z at 0, +-2^-k and
// +-1 and random directions, the sampler's draws at 0, 1e-6, 1 - 2^-24 and random, roughness at the ends of the lazy instance's interval and log-uniform between,
// metallic 0, 1 and random -- runs the sampler and the ScatteringPdf part as ScatterLazy does, and evaluates the reflectance whatever the guard says.
// out[0]: events; out[1]: events that pass the guard (with pdf > 0, the recorded ones) while a component of refl or sp is not finite -- must be 0;
// out[2]: events with pdf > 0 that fail the guard.
__global__ void __launch_bounds__(RL_BLOCK)
k_verify_lazy_refl(uint32_t n, unsigned long long seed, unsigned long long* __restrict__ out)
{
	RL_MATH_PROLOGUE();
	const uint32_t i0 = blockIdx.x * RL_BLOCK + threadIdx.x, stride = gridDim.x * RL_BLOCK;
	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	unsigned long long events = 0, bad = 0, failed = 0;
	for (uint32_t i = i0; i < n; i += stride) {
		Rng g; V3 Wo; float u0, u1, rough;
		const uint32_t sel = LazySweepEvent(seed, i, g, Wo, u0, u1, rough);
		const uint32_t mk = sel % 2u;
		// metallic 0, 1, the planner's ends +-RL_LAZY_COLOR_MAX and random in between; albedo likewise, of either sign
		const float mr = Next(g);
		const float metallic = mk == 0u ? (mr < 0.25f ? 0.0f : mr < 0.5f ? 1.0f : mr < 0.75f ? RL_LAZY_COLOR_MAX : -RL_LAZY_COLOR_MAX) : RL_LAZY_COLOR_MAX * (2.0f * Next(g) - 1.0f);
		const float ar = Next(g);
		const V3 albedo = sel % 13u == 0u ? v3s(ar < 0.5f ? RL_LAZY_COLOR_MAX : -RL_LAZY_COLOR_MAX)
		                                  : v3(Next(g), RL_LAZY_COLOR_MAX * (2.0f * Next(g) - 1.0f), ar < 0.5f ? -RL_LAZY_COLOR_MAX : RL_LAZY_COLOR_MAX * Next(g));
		// the event, as ScatterLazy makes it (local frame = world frame)
		const V3 N = v3(0.0f, 0.0f, 1.0f);
		const bool bFlip = Wo.z < 0.0f;
		V3 Wh = BeckmannSample(bFlip ? -Wo : Wo, rough, rough, u0, u1, c);
		if (bFlip) Wh = -Wh;
		const V3 Wi = reflect(-Wo, Wh);
		V3 wh = normalize(Wo + Wi);
		if (wh.z < 0.0f) wh.z = -wh.z;
		const float sp = DistributionBeckmann(N, wh, rough) * absDot(wh, N);
		const float pdf = sp / (4.0f * dot(Wo, Wh));
		const V3 refl = ReflFromRecord<true>(albedo, rough, metallic, N, Wo, Wh, Wi, absDot(N, Wi));
		++events;
		if (pdf > 0.0f) {
			const bool finite = fabsf(refl.x) < INFINITY && fabsf(refl.y) < INFINITY && fabsf(refl.z) < INFINITY && fabsf(sp) < INFINITY;
			if (!LazyVertexSafe(Wo, Wh, sp)) ++failed;
			else if (!finite) ++bad;
		}
	}
	for (int off = 32; off > 0; off >>= 1) { events += __shfl_down(events, off); bad += __shfl_down(bad, off); failed += __shfl_down(failed, off); }
	if ((threadIdx.x & 63u) == 0u) { atomicAdd(&out[0], events); if (bad) atomicAdd(&out[1], bad); if (failed) atomicAdd(&out[2], failed); }
}

// Test hook: LazyPdfQuick's claim and the two record forms, swept over the events of k_verify_lazy_refl.  Every thread runs the sampler, evaluates sp and pdf
// eagerly (Scatter's statements), takes what LazyScatterPdf leaves, makes the vertex record k_trace_lazy would store from it and recomputes sp and pdf from the
// record as the fold does (LazyRecordPdf); then the same through the other record form (the exact sp, flagged), which every event may take.
// out[0]: events; out[1]: events that are quick although pdf > 0 is false, sp, wh.x or wh.y is not finite, or whose record (of either form) gives back another
// bit of sp or pdf than the eager evaluation; or that are not quick and whose flagged record does -- must be 0; out[2]: events that are not quick.
__global__ void __launch_bounds__(RL_BLOCK)
k_verify_lazy_pdf(uint32_t n, unsigned long long seed, unsigned long long* __restrict__ out)
{
	RL_MATH_PROLOGUE();
	const uint32_t i0 = blockIdx.x * RL_BLOCK + threadIdx.x, stride = gridDim.x * RL_BLOCK;
	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	unsigned long long events = 0, wrong = 0, refused = 0;
	// (whole waves walk the loop together: LazyScatterPdf votes across the wave, and n is rounded up for the vote's sake alone)
	for (uint32_t i = i0; i < ((n + 63u) & ~63u); i += stride) {
		const bool live = i < n;
		Rng g; V3 Wo; float u0, u1, rough;
		LazySweepEvent(seed, live ? i : 0u, g, Wo, u0, u1, rough);
		// the event, as ScatterLazy makes it (local frame = world frame)
		const V3 N = v3(0.0f, 0.0f, 1.0f);
		const bool bFlip = Wo.z < 0.0f;
		V3 Wh = BeckmannSample(bFlip ? -Wo : Wo, rough, rough, u0, u1, c);
		if (bFlip) Wh = -Wh;
		const V3 Wi = reflect(-Wo, Wh);
		V3 wh = normalize(Wo + Wi);
		if (wh.z < 0.0f) wh.z = -wh.z;
		// eager
		const float spE = DistributionBeckmann(N, wh, rough) * absDot(wh, N);
		const float pdfE = spE / (4.0f * dot(Wo, Wh));
		// lazy: what the event leaves, the record made of it, and the fold's values from the record
		float spSlot, pdfSeen;
		const bool exactSp = LazyScatterPdf(N, Wo, Wh, wh, rough, spSlot, pdfSeen);
		const int mi = (int)(i & 0xffffu);
		const float4 r0 = make_float4(Wo.x, Wo.y, Wo.z, spSlot), r1 = make_float4(Wh.x, Wh.y, Wh.z, __int_as_float(exactSp ? mi | RL_LAZY_REC_EXACT_SP : mi));
		float spR, pdfR;
		LazyRecordPdf(r0, r1, rough, spR, pdfR);
		bool bad = RL_LAZY_REC_MAT(r1.w) != mi || __float_as_uint(spR) != __float_as_uint(spE) || __float_as_uint(pdfR) != __float_as_uint(pdfE);
		// the flagged form, whatever the event chose
		const float4 f0 = make_float4(Wo.x, Wo.y, Wo.z, spE), f1 = make_float4(Wh.x, Wh.y, Wh.z, __int_as_float(mi | RL_LAZY_REC_EXACT_SP));
		LazyRecordPdf(f0, f1, rough, spR, pdfR);
		bad = bad || RL_LAZY_REC_MAT(f1.w) != mi || __float_as_uint(spR) != __float_as_uint(spE) || __float_as_uint(pdfR) != __float_as_uint(pdfE);
		if (!exactSp) {
			bad = bad || !(pdfE > 0.0f) || !(fabsf(spE) < INFINITY) || !(fabsf(wh.x) < INFINITY) || !(fabsf(wh.y) < INFINITY);
			bad = bad || !(pdfSeen > 0.0f) || !(fabsf(spSlot) < INFINITY);   // what k_trace_lazy's two predicates read instead
		} else {
			bad = bad || (pdfSeen > 0.0f) != (pdfE > 0.0f) || __float_as_uint(spSlot) != __float_as_uint(spE);
		}
		if (live) { ++events; if (bad) ++wrong; if (exactSp) ++refused; }
	}
	for (int off = 32; off > 0; off >>= 1) { events += __shfl_down(events, off); wrong += __shfl_down(wrong, off); refused += __shfl_down(refused, off); }
	if ((threadIdx.x & 63u) == 0u) { atomicAdd(&out[0], events); if (wrong) atomicAdd(&out[1], wrong); if (refused) atomicAdd(&out[2], refused); }
}

// Test hook: the ranged sampler's claims (rl_dev_shade.h "the ranged sampler"), each a function of one float and swept over ALL 2^32 bit patterns of it.
//   mode 0: the loop body -- ErfInvRanged(b) and exp_in_range_ of minus its square against ErfInv(b) and exp_;
//   mode 1: the prologue -- SamplerPrologueRanged against SamplerPrologue (tanThetaI, c, fit, normalization) for every cosThetaI that does not take the .9999
//           branch.  Counted: the mismatches inside [RL_SAMPLER_C_MIN, .9999] (must be 0) and those outside; out[2] keeps the largest positive bit pattern below the
//           branch at which the two differ -- the agreeing interval begins one pattern above it and ends at the last one below the branch;
//   mode 2: the branch -- cosThetaI >= RL_SAMPLER_COS_NEAR_ONE against (double)cosThetaI > .9999;
//   mode 3: logf_in_range_, expf_in_range_ and sqrtf_in_range_ (rl_glibc_math.h) against logf_, expf_ and sqrtf, each over its stated domain.
// out[0]: mismatches (a NaN may meet a NaN of another payload); out[1]: the smallest mismatching bit pattern; out[2]: see mode 1 (0: none); out[3]: mode 1's
// mismatches outside the interval; out[4], out[5]: the bits of RL_SAMPLER_C_MIN and RL_SAMPLER_COS_NEAR_ONE as compiled.
__device__ __forceinline__ bool SameBitsOrNaN(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }
__global__ void __launch_bounds__(RL_BLOCK)
k_verify_sampler_ranged(int mode, unsigned long long* __restrict__ out)
{
	RL_MATH_PROLOGUE();
	const unsigned long long tid = (unsigned long long)blockIdx.x * RL_BLOCK + threadIdx.x, n = (unsigned long long)gridDim.x * RL_BLOCK;
	unsigned long long bad = 0, first = ~0ull, outside = 0, top = 0;
	// (every thread of a launch of whole workgroups makes the same number of trips: the general prologue votes across the wave)
	for (unsigned long long b = tid; b < (1ull << 32); b += n) {
		const uint32_t bits = (uint32_t)b;
		const float x = __uint_as_float(bits);
		bool differs = false;
		if (mode == 0) {
			float ig, eg, ir, er;
			SamplerLoopTerms(x, ig, eg);
			SamplerLoopTermsRanged(x, ir, er);
			differs = !SameBitsOrNaN(ig, ir) || !SameBitsOrNaN(eg, er);
		} else if (mode == 1) {
			if (!(x >= RL_SAMPLER_COS_NEAR_ONE)) {
				float tg, cg, fg, ng, tr, cr, fr, nr;
				SamplerPrologue(x, tg, cg, fg, ng);
				SamplerPrologueRanged(x, tr, cr, fr, nr);
				const bool d = !SameBitsOrNaN(tg, tr) || !SameBitsOrNaN(cg, cr) || !SameBitsOrNaN(fg, fr) || !SameBitsOrNaN(ng, nr);
				if (x >= RL_SAMPLER_C_MIN) differs = d;
				else if (d) ++outside;
				if (d && bits - 1u < 0x7f7fffffu) top = max(top, (unsigned long long)bits);   // positive and finite
			}
		} else if (mode == 2) {
			differs = (x >= RL_SAMPLER_COS_NEAR_ONE) != ((double)x > .9999);
		} else {
			if (bits - 0x00800000u < 0x7f800000u - 0x00800000u) differs = differs || !SameBitsOrNaN(rlm::logf_in_range_(x), rlm::logf_(x));
			if (((bits >> 20) & 0x7ffu) < ((rlm::asuint(88.0f) >> 20) & 0x7ffu)) differs = differs || !SameBitsOrNaN(rlm::expf_in_range_(x), rlm::expf_(x));
			if (bits - 0x0d000000u < 0x7f800000u - 0x0d000000u) differs = differs || !SameBitsOrNaN(rlm::sqrtf_in_range_(x), __builtin_sqrtf(x));
		}
		if (differs) { ++bad; first = min(first, b); }
	}
	if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], first); }
	if (top) atomicMax(&out[2], top);
	if (outside) atomicAdd(&out[3], outside);
	if (tid == 0) { out[4] = __float_as_uint(RL_SAMPLER_C_MIN); out[5] = __float_as_uint(RL_SAMPLER_COS_NEAR_ONE); }   // the constants this build was compiled with
}

// Test hook: the ranged normalisations' claims (rl_dev_core.h "normalize without the two range guards"), whatever bits of the setting this build has on.
//   mode 0: all 2^32 bit patterns x of len2 -- rcp1_in_range_(sqrtf_in_range_(x)) against rcp1_(sqrtf_(x)), normalize's scalar chain.  Counted: the mismatches inside
//           NormalizeInRange's domain (must be 0); out[2] keeps the smallest pattern outside it at which the chains differ and out[3] counts those;
//   mode 1: acosf_in_range_ against acos_ on every float of the ranged prologue's interval [RL_SAMPLER_C_MIN, RL_SAMPLER_COS_NEAR_ONE);
//   mode 2: normalize_voted_ against normalize, component bits compared, on one wave of edge vectors (below) and 2^24 generated ones: waves whose lanes share a
//           binary scale (2^0 down to 2^-51, where len2 crosses 2^-101, and up to 2^64, where it overflows), waves of mixed scales, waves with a component +-0.
//           out[1] is the first differing vector's index, out[3] the vectors whose wave took the ranged side.
// out[0]: mismatches (a NaN may meet a NaN of another payload); out[1]: the smallest mismatching input.
#define RL_NORMALIZE_SWEEP_VECTORS (64u + (1u << 24))
__global__ void __launch_bounds__(RL_BLOCK)
k_verify_normalize_ranged(int mode, unsigned long long* __restrict__ out)
{
	RL_MATH_PROLOGUE();
	const unsigned long long tid = (unsigned long long)blockIdx.x * RL_BLOCK + threadIdx.x, n = (unsigned long long)gridDim.x * RL_BLOCK;
	unsigned long long bad = 0, first = ~0ull, firstOutside = ~0ull, count = 0;
	if (mode == 2) {
		// (whole waves walk the loop together -- RL_NORMALIZE_SWEEP_VECTORS is a multiple of 64 -- for the vote's sake)
		const float inf = INFINITY, qnan = __uint_as_float(0x7fc00000u), sub = __uint_as_float(1u), lo = 0x1.6a09e6p-51f, hi = 0x1.6a09e8p-51f;   // lo lo < 2^-101 <= hi hi
		const V3 edge[32] = {
			v3(0.0f, 0.0f, 0.0f), v3(-0.0f, -0.0f, -0.0f), v3(0.0f, -0.0f, 0.0f), v3(0.0f, 1.0f, 1.0f), v3(1.0f, -0.0f, 1.0f), v3(-1.0f, 1.0f, 0.0f), v3(0.0f, 0.0f, -1.0f), v3(-0.0f, 2.0f, -0.0f),
			v3(sub, 0.0f, 0.0f), v3(sub, sub, sub), v3(0x1p-70f, 0x1p-70f, 0.0f), v3(0x1p-127f, -0x1p-130f, 0x1p-149f), v3(0x1p-63f, 0.0f, 0x1p-64f), v3(0.0f, -0x1p-74f, 0.0f), v3(0x1p-126f, 0x1p-126f, 0x1p-126f), v3(-0x1p-60f, 0x1p-61f, 0x1p-62f),
			v3(lo, 0.0f, 0.0f), v3(hi, 0.0f, 0.0f), v3(0.0f, -lo, 0.0f), v3(0.0f, 0.0f, -hi), v3(0x1p-51f, 0x1p-51f, 0.0f), v3(0x1p-51f, 0x1p-52f, 0x1p-52f), v3(0x1p-51f, 0x1p-51f, sub), v3(0x1p-50f, 0.0f, -0.0f),
			v3(inf, 0.0f, 0.0f), v3(-inf, 1.0f, 1.0f), v3(inf, inf, -inf), v3(qnan, 1.0f, 1.0f), v3(1.0f, qnan, 0.0f), v3(0x1p64f, 0x1p64f, 0.0f), v3(FLT_MAX, -FLT_MAX, FLT_MAX), v3(0x1p63f, -0x1p63f, 0x1p63f) };
		const int scale[8] = { 0, -20, -45, -50, -51, 40, 63, 64 };
		for (unsigned long long i = tid; i < RL_NORMALIZE_SWEEP_VECTORS; i += n) {
			const uint32_t w = (uint32_t)(i >> 6), lane = (uint32_t)i & 63u;
			V3 v = edge[lane & 31u];
			if (w > 0u) {
				Rng g; g.s = raylib_rng_begin(0x6e6f726d616c697aull, (uint32_t)i, 0);
				const uint32_t cls = w % 10u;
				int e = scale[cls & 7u];
				v = v3(2.0f * Next(g) - 1.0f, 2.0f * Next(g) - 1.0f, 2.0f * Next(g) - 1.0f);
				if (cls == 8u) e = -80 + (int)(Next(g) * 146.0f);
				if (cls == 9u) { const float z = (lane & 4u) ? -0.0f : 0.0f; const uint32_t k = lane % 3u; if (k == 0u) v.x = z; else if (k == 1u) v.y = z; else v.z = z; }
				const float s = __uint_as_float((uint32_t)(127 + e) << 23);
				v = v3(v.x * s, v.y * s, v.z * s);
			}
			const bool ranged = !rtm::wave_any_(!NormalizeInRange(v.x * v.x + v.y * v.y + v.z * v.z));
			const V3 a = normalize_voted_(v), b = normalize(v);
			if (!SameBitsOrNaN(a.x, b.x) || !SameBitsOrNaN(a.y, b.y) || !SameBitsOrNaN(a.z, b.z)) { ++bad; first = min(first, i); }
			if (ranged) ++count;
		}
	} else {
		for (unsigned long long b = tid; b < (1ull << 32); b += n) {
			const uint32_t bits = (uint32_t)b;
			const float x = __uint_as_float(bits);
			if (mode == 0) {
				const bool d = !SameBitsOrNaN(rlm::rcp1_in_range_(rlm::sqrtf_in_range_(x)), rlm::rcp1_(rlm::sqrtf_(x)));
				if (NormalizeInRange(x)) { if (d) { ++bad; first = min(first, b); } }
				else if (d) { ++count; firstOutside = min(firstOutside, b); }
			} else if (x >= RL_SAMPLER_C_MIN && !(x >= RL_SAMPLER_COS_NEAR_ONE)) {
				if (!SameBitsOrNaN(rtm::acos_in_range_(x), rtm::acos_(x))) { ++bad; first = min(first, b); }
			}
		}
	}
	if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], first); }
	if (firstOutside != ~0ull) atomicMin(&out[2], firstOutside);
	if (count) atomicAdd(&out[3], count);
}

// ---- instances ----
RL_TRACE_LAZY_INSTANCES(RL_K_TRACE_LAZY)
RL_TRACE_LAZY_INSTANCES(RL_K_TRACE_LAZY_HITQ)

} // namespace rl
