// k_temporal: the temporal accumulation of RaylibAMD_TemporalAccumulate (include/raylib_amd.h statements T7 and T8).  The per-pixel arithmetic is
// rl_temporal.h's TemporalPixel, which the host oracle compiles too; this unit is how the device reads and writes the planes.
//
// A streaming kernel, bound by memory: per pixel 48 bytes of its own (colour, hit, motion), up to four taps of 36 bytes (history colour, hit, length) and 20
// bytes stored.  The lanes are the G-buffer's: lane p of a wave is pixel (p & 7, p >> 3) of an 8 x 8 cell, so every plane is read and written as rows of
// eight 16-byte records, and a wave's taps fall into the 9 x 9 neighbourhood of where its cell was -- the history is read from memory about once.  One
// cell per wave, a grid-stride loop over the cells; no LDS, no atomics.
//
// k_temporal_moments (RaylibAMD_TemporalAccumulateMoments, statements S1 and S2) is the same walk (TemporalCells) with the moments' planes beside it: a tap
// reads 8 bytes more, a pixel stores 8 bytes more.  It is a kernel of its own, so k_temporal's code is what it was (profiles/variance_filter_isa_equivalence.log).
#include "rl_kernels.h"
#include "rl_temporal.h"

namespace rl {

namespace {
// the history's planes; MOMENTS: with the moments' plane beside the other three
template <bool MOMENTS>
struct DeviceTaps {
	const float4* __restrict__ colour; const float4* __restrict__ hit; const float* __restrict__ length; const float2* __restrict__ moments;
	__device__ __forceinline__ bool Has() const { return colour != nullptr; }
	__device__ __forceinline__ TemporalTap Read(size_t q) const
	{
		const float4 c = colour[q], h = hit[q];
		TemporalTap t;
		t.r = c.x; t.g = c.y; t.b = c.z; t.t = h.x; t.prim = __float_as_int(h.y); t.length = length[q];
		return t;
	}
	__device__ __forceinline__ void Moments(size_t q, float m[2]) const { const float2 v = moments[q]; m[0] = v.x; m[1] = v.y; }
};
// the cell loop of both kernels: one cell per wave at a time, lane p its pixel (p & 7, p >> 3).  T by value, as a kernel holds its argument: by reference the
// compiler allocates other registers (profiles/plane_calls_isa_equivalence.log is of this form)
template <bool MOMENTS>
__device__ __forceinline__ void TemporalCells(const DTemporal T, const float2* __restrict__ histMoments, float2* __restrict__ outMoments)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wavesPerBlock = RL_BLOCK / 64u;
	const DeviceTaps<MOMENTS> taps = { T.histColour, T.histHit, T.histLength, histMoments };
	for (uint32_t cell = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6); cell < T.numCells; cell += gridDim.x * wavesPerBlock) {
		const uint32_t x = (cell % T.cellsX) * 8u + (lane & 7u), y = (cell / T.cellsX) * 8u + (lane >> 3);
		if (x >= T.width || y >= T.height) continue;
		const size_t p = (size_t)y * T.width + x;
		const float4 c = T.colour[p], h = T.hit[p], m = T.motion[p];
		const float rgb[3] = { c.x, c.y, c.z };
		float out[3], len, mom[2];
		TemporalPixelM<MOMENTS>(T.width, T.height, rgb, __float_as_int(h.y), m.x, m.y, m.z, __float_as_uint(m.w), T.depthTolerance, T.maxLength, taps, out, len, mom);
		T.outColour[p] = make_float4(out[0], out[1], out[2], 1.0f);
		T.outLength[p] = len;
		if constexpr (MOMENTS) outMoments[p] = make_float2(mom[0], mom[1]);
	}
}
} // namespace

__global__ void __launch_bounds__(RL_BLOCK)
k_temporal(const DTemporal T)
{
	TemporalCells<false>(T, nullptr, nullptr);
}

__global__ void __launch_bounds__(RL_BLOCK)
k_temporal_moments(const DTemporal T, const float2* __restrict__ histMoments, float2* __restrict__ outMoments)
{
	TemporalCells<true>(T, histMoments, outMoments);
}

} // namespace rl
