// Adaptive gather (RaylibAMD_GatherAdaptive, include/raylib_amd.h statements A1 to A5) as a translation unit of its own: the device code behind the unchanged trace
// kernel (k_gather, rl_gather.hip).  A pass traces the live points -- compacted into a contiguous array, so that k_gather takes them as any caller's -- and
//   k_gather_adaptive_resolve   sums the launch's samples as k_gather_resolve does, keeps the stopping rule's moments beside the sums, and decides after the
//                               pass's last sample range (rl_progressive.h ProgressivePixelError: the progressive renderer's statement, not restated);
//   k_gather_compact_*          make the next pass's live set from the stop flags, in order, over as many workgroups as the list needs;
//   k_gather_scatter_counts     puts a bake's per-point sample counts into the atlas (RaylibAMD_BakeLightmapAdaptive).
// No walk and no shading lives here: rl_gather.hip and rl_radiance.hip stay the code they are (tools/isa_equivalence.py).

// ---- settings ----
// None.

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_progressive.h"

namespace rl {

// k_gather_adaptive_resolve: k_gather_resolve's serial per-point loop (rl_gather.hip: one thread per point of the launch, the samples numPoints slots apart,
// RL_GATHER_AHEAD loads in front of the adds), on the point `orig` the launch's slot stands for.  The sums and the moments are the call's state, indexed by
// orig; they start at +0 (the host clears them) and are always loaded: +0 + x has the bits of k_gather_resolve's `first ? 0 : acc` form, which starts from
// +0 too (x = -0 gives +0 in both).  The moments come from the first plane's xyz -- the hemisphere's weighted sample, the sphere's L -- by statement A2.
// decide: the launch holds the pass's last sample range; a point that stops writes its result exactly as k_gather_resolve's last block does.
#define RL_GATHER_AHEAD 8
template <int GEN>
__global__ void __launch_bounds__(RL_BLOCK)
k_gather_adaptive_resolve(const float4* __restrict__ samples, uint32_t numPoints, uint32_t numSamples, const uint32_t* __restrict__ live, uint32_t pointFirst,
                          const GatherAdaptiveState st, int decide, uint32_t samplesNow, float* __restrict__ out, uint32_t* __restrict__ outSamples)
{
	static_assert(GEN == RL_GEN_HEMISPHERE || GEN == RL_GEN_SPHERE, "generator");
	constexpr int NA = GEN == RL_GEN_HEMISPHERE ? 3 : 27;
	const uint32_t p = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (p >= numPoints) return;
	const uint32_t orig = live ? live[pointFirst + p] : pointFirst + p;
	float a[NA];
#pragma unroll
	for (int j = 0; j < NA; ++j) a[j] = st.sum[(size_t)j * st.numPoints + orig];
	float s1 = st.s1[orig], s2 = st.s2[orig];
	const float4* lp = samples + p;                                    // L (hemisphere: the weighted sample) of sample s at lp[s * numPoints]
	const float4* wp = samples + (size_t)numPoints * numSamples + p;   // the sphere's Wi plane
	auto add = [&](const float4 l, const float4 w) __attribute__((always_inline)) {
		const float lum = dot(v3(l.x, l.y, l.z), v3(0.2126f, 0.7152f, 0.0722f));   // (k_progressive_resolve's statement)
		const float yv = lum / (1.0f + lum);
		s1 += yv; s2 += yv * yv;
		if constexpr (GEN == RL_GEN_HEMISPHERE) {
			(void)w;
			a[0] = a[0] + l.x; a[1] = a[1] + l.y; a[2] = a[2] + l.z;
		} else {
			const float x = w.x, y = w.y, z = w.z;
			float Y[9];
			Y[0] = 0.282095f;
			Y[1] = 0.488603f * y;
			Y[2] = 0.488603f * z;
			Y[3] = 0.488603f * x;
			Y[4] = 1.092548f * (x * y);
			Y[5] = 1.092548f * (y * z);
			Y[6] = 0.315392f * (3.0f * (z * z) - 1.0f);
			Y[7] = 1.092548f * (x * z);
			Y[8] = 0.546274f * (x * x - y * y);
#pragma unroll
			for (int j = 0; j < 9; ++j) {
				a[3 * j + 0] = a[3 * j + 0] + l.x * Y[j];
				a[3 * j + 1] = a[3 * j + 1] + l.y * Y[j];
				a[3 * j + 2] = a[3 * j + 2] + l.z * Y[j];
			}
		}
	};
	uint32_t s = 0u;
	for (; s + RL_GATHER_AHEAD <= numSamples; s += RL_GATHER_AHEAD) {
		float4 l[RL_GATHER_AHEAD], w[RL_GATHER_AHEAD];
#pragma unroll
		for (int k = 0; k < RL_GATHER_AHEAD; ++k) {
			l[k] = lp[(size_t)(s + k) * numPoints];
			if constexpr (GEN == RL_GEN_SPHERE) w[k] = wp[(size_t)(s + k) * numPoints]; else w[k] = l[k];
		}
#pragma unroll
		for (int k = 0; k < RL_GATHER_AHEAD; ++k) add(l[k], w[k]);
	}
	for (; s < numSamples; ++s) {
		const float4 l = lp[(size_t)s * numPoints];
		add(l, GEN == RL_GEN_SPHERE ? wp[(size_t)s * numPoints] : l);
	}
	const bool stops = decide && (samplesNow == st.cap || ProgressiveCellStops(ProgressivePixelError(s1, s2, samplesNow), samplesNow, st.threshold, st.minSamples));
	if (!stops) {
#pragma unroll
		for (int j = 0; j < NA; ++j) st.sum[(size_t)j * st.numPoints + orig] = a[j];
		st.s1[orig] = s1; st.s2[orig] = s2;
		return;
	}
	// the mean, then the solid angle of the directions' domain: 2 pi (bits 0x40C90FDB) or 4 pi (0x41490FDB)
	const float k = rtm::rcp1_((float)samplesNow);
	const float omega = GEN == RL_GEN_HEMISPHERE ? 6.2831855f : 12.566371f;
	if constexpr (GEN == RL_GEN_HEMISPHERE) {
		((float4*)out)[orig] = make_float4(a[0] * k * omega, a[1] * k * omega, a[2] * k * omega, 1.0f);
	} else {
#pragma unroll
		for (int j = 0; j < NA; ++j) out[(size_t)orig * NA + j] = a[j] * k * omega;
	}
	if (outSamples) outSamples[orig] = samplesNow;
	st.stopped[orig] = 1;
}

// ---- the live set of the next pass ----
// A workgroup takes RL_GATHER_COMPACT_TILE consecutive entries of the list, a thread RL_GATHER_COMPACT_PER consecutive ones of those.  Entry i of the list is the
// point live[i] (null: i itself, the first pass), and its record stands at slot i of the pass's point array.
// keep: bit k set when the thread's entry k is inside the list and its point has not stopped
__device__ __forceinline__ uint32_t CompactKeep(const uint32_t* __restrict__ live, const uint8_t* __restrict__ stopped, uint32_t numLive, uint32_t first, uint32_t (&c)[RL_GATHER_COMPACT_PER])
{
	uint32_t keep = 0u;
#pragma unroll
	for (int k = 0; k < RL_GATHER_COMPACT_PER; ++k) {
		const uint32_t i = first + (uint32_t)k;
		c[k] = i < numLive ? (live ? live[i] : i) : 0u;
		if (i < numLive && !stopped[c[k]]) keep |= 1u << k;
	}
	return keep;
}
// the inclusive sum of v over the workgroup's threads in thread order: shuffles inside the wave, the waves' totals through LDS
__device__ __forceinline__ uint32_t CompactBlockInclusive(uint32_t v, uint32_t* sWave)
{
	constexpr uint32_t WAVES = RL_BLOCK / 64;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t incl = v;
	for (uint32_t off = 1; off < 64; off <<= 1) { const uint32_t u = __shfl_up(incl, off); if (lane >= off) incl += u; }
	if (lane == 63u) sWave[wave] = incl;
	__syncthreads();
	for (uint32_t w = 0; w < WAVES; ++w) if (w < wave) incl += sWave[w];
	return incl;
}
// the entries a tile keeps, into blockCounts[tile]
__global__ void __launch_bounds__(RL_BLOCK)
k_gather_compact_count(const uint32_t* __restrict__ live, const uint8_t* __restrict__ stopped, uint32_t numLive, uint32_t* __restrict__ blockCounts)
{
	__shared__ uint32_t sWave[RL_BLOCK / 64];
	uint32_t c[RL_GATHER_COMPACT_PER];
	const uint32_t keep = CompactKeep(live, stopped, numLive, blockIdx.x * RL_GATHER_COMPACT_TILE + threadIdx.x * RL_GATHER_COMPACT_PER, c);
	const uint32_t incl = CompactBlockInclusive(__popc(keep), sWave);
	if (threadIdx.x == RL_BLOCK - 1) blockCounts[blockIdx.x] = incl;
}
// the tiles' counts scanned in place (exclusive) by one workgroup, numTiles = ceil(numLive / RL_GATHER_COMPACT_TILE) values; the total into blockCounts[numTiles]
// and into *count, which the host reads
__global__ void __launch_bounds__(RL_GATHER_COMPACT_SCAN_BLOCK)
k_gather_compact_scan(uint32_t* __restrict__ blockCounts, uint32_t numTiles, uint32_t* __restrict__ count)
{
	constexpr uint32_t WAVES = RL_GATHER_COMPACT_SCAN_BLOCK / 64;
	__shared__ uint32_t sWave[WAVES];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t carry = 0u;   // (the same in every thread)
	for (uint32_t base = 0u; base < numTiles; base += RL_GATHER_COMPACT_SCAN_BLOCK) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < numTiles ? blockCounts[i] : 0u;
		uint32_t incl = v;
		for (uint32_t off = 1; off < 64; off <<= 1) { const uint32_t u = __shfl_up(incl, off); if (lane >= off) incl += u; }
		if (lane == 63u) sWave[wave] = incl;
		__syncthreads();
		uint32_t total = 0u;
		for (uint32_t w = 0; w < WAVES; ++w) { if (w < wave) incl += sWave[w]; total += sWave[w]; }
		if (i < numTiles) blockCounts[i] = carry + (incl - v);
		carry += total;
		__syncthreads();   // (sWave is re-used by the next round)
	}
	if (threadIdx.x == 0) { blockCounts[numTiles] = carry; *count = carry; }
}
// the kept entries to their places: the list, and each point's 32-byte record as two float4 loads and stores
__global__ void __launch_bounds__(RL_BLOCK)
k_gather_compact_move(const uint32_t* __restrict__ live, const uint8_t* __restrict__ stopped, uint32_t numLive, const uint32_t* __restrict__ blockCounts,
                      const float4* __restrict__ points, uint32_t* __restrict__ outLive, float4* __restrict__ outPoints)
{
	__shared__ uint32_t sWave[RL_BLOCK / 64];
	uint32_t c[RL_GATHER_COMPACT_PER];
	const uint32_t first = blockIdx.x * RL_GATHER_COMPACT_TILE + threadIdx.x * RL_GATHER_COMPACT_PER;
	const uint32_t keep = CompactKeep(live, stopped, numLive, first, c);
	const uint32_t mine = __popc(keep);
	uint32_t at = blockCounts[blockIdx.x] + CompactBlockInclusive(mine, sWave) - mine;
#pragma unroll
	for (int k = 0; k < RL_GATHER_COMPACT_PER; ++k) {
		if (!(keep >> k & 1u)) continue;
		const float4* src = points + 2u * (size_t)(first + (uint32_t)k);
		const float4 r0 = src[0], r1 = src[1];
		outLive[at] = c[k];
		float4* dst = outPoints + 2u * (size_t)at;
		dst[0] = r0; dst[1] = r1;
		++at;
	}
}

// RaylibAMD_BakeLightmapAdaptive: one thread per texel, a texel with a point (rank[i + 1] != rank[i], as k_lm_scatter reads it) takes counts[rank[i]], every other 0
__global__ void __launch_bounds__(RL_BLOCK)
k_gather_scatter_counts(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ counts, uint32_t numTexels, uint32_t* __restrict__ atlas)
{
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= numTexels) return;
	const uint32_t at = rank[i];
	atlas[i] = rank[i + 1u] != at ? counts[at] : 0u;
}

// ---- instances ----
template __global__ void k_gather_adaptive_resolve<RL_GEN_HEMISPHERE>(RL_GATHER_ADAPTIVE_RESOLVE_ARGS);
template __global__ void k_gather_adaptive_resolve<RL_GEN_SPHERE>(RL_GATHER_ADAPTIVE_RESOLVE_ARGS);

} // namespace rl
