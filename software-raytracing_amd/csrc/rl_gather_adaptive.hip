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

// ---- kernel bodies ----
// k_gather_adaptive_resolve: k_gather_resolve's twin, from the one source of both
#define RL_GATHER_ADAPTIVE 1
#include "rl_k_gather_resolve.inl"

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
