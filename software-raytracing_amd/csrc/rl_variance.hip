// The variance-guided a-trous filter on planes (RaylibAMD_FilterVariance, include/raylib_amd.h statements S3 to S7).  The per-pixel arithmetic is
// rl_variance.h's, which the host oracle compiles too; this unit is how the device reads and writes the planes.  A call is 2 + K launches on one stream:
//   k_vf_pack      the caller's colour, hit and surface planes -> a 32-byte guide record and a 16-byte value record per pixel (S3).  The 44-byte surface
//                  record is read once here, as 4-byte words; every tap afterwards is three aligned 16-byte loads.
//   k_vf_variance  the initial variance into the value record's w (S5): the temporal one where the history is long, else the 7 x 7 window.
//   k_vf_iter      one iteration (S6) with the 3 x 3 variance prefilter fused in: it reads the nine neighbours' w of the records whose rows the 25 taps'
//                  middle row reads anyway.  The last iteration writes the caller's planes instead of the ping-pong record.
// The iterations read global memory directly, as k_dn_iter does: a 16 x 16 pixel tile per workgroup, a wave64 is 16 x 4 pixels, so a tap row of a wave is one
// 256-byte run of value records and one 512-byte run of guides at step 1, and 16 separate records at steps >= 16.  DESIGN.md section 2 has the traffic and the
// measured times (profiles/variance_filter_time.log).
// One-dimensional blocks and a one-dimensional grid of tiles: RL_MATH_PROLOGUE() indexes the tables by threadIdx.x and ends in a barrier, so every thread
// reaches it before any returns; W * H up to 2^31 - 1 is at most 2^27 tiles.
#include "rl_kernels.h"

namespace rl {

namespace {
constexpr uint32_t VF_T = 16u;   // the tile's edge: VF_T * VF_T == RL_BLOCK
static_assert(VF_T * VF_T == RL_BLOCK, "a tile is a workgroup");
__device__ __forceinline__ bool TilePixel(uint32_t W, uint32_t H, int& x, int& y)
{
	const uint32_t tilesX = (W + VF_T - 1u) / VF_T;
	const uint32_t px = (blockIdx.x % tilesX) * VF_T + (threadIdx.x % VF_T), py = (blockIdx.x / tilesX) * VF_T + (threadIdx.x / VF_T);
	x = (int)px; y = (int)py;
	return px < W && py < H;
}
} // namespace

__global__ void __launch_bounds__(RL_BLOCK)
k_vf_pack(const float4* __restrict__ colour, const float4* __restrict__ hit, const float* __restrict__ surface, uint32_t pixels, VfGuide* __restrict__ guides,
          VfValue* __restrict__ values)
{
	const uint32_t p = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (p >= pixels) return;
	const float4 c = colour[p];
	const float* s = surface + (size_t)p * 11u;   // {hit, t, p[3], n[3], paramU, paramV, material}
	const float P[3] = { s[2], s[3], s[4] }, n[3] = { s[5], s[6], s[7] };
	guides[p] = VfPackGuide(__float_as_int(hit[p].y), P, n);
	VfValue v;
	v.r = VfFin(c.x); v.g = VfFin(c.y); v.b = VfFin(c.z); v.var = 0.0f;
	values[p] = v;
}

__global__ void __launch_bounds__(RL_BLOCK)
k_vf_variance(const VfGuide* __restrict__ guides, const float* __restrict__ moments, const float* __restrict__ length, uint32_t W, uint32_t H, const VfConst c,
              VfValue* values)
{
	RL_MATH_PROLOGUE();
	int x, y;
	if (!TilePixel(W, H, x, y)) return;
	const size_t p = (size_t)y * W + (size_t)x;
	if (guides[p].prim == -1) return;
	values[p].var = VfInitialVariance(guides, moments, length, (int)W, (int)H, x, y, c);
}

template <bool LAST> __global__ void __launch_bounds__(RL_BLOCK)
k_vf_iter(const VfValue* __restrict__ I, const VfGuide* __restrict__ guides, uint32_t W, uint32_t H, int32_t step, const VfConst c, VfValue* __restrict__ next,
          float4* __restrict__ outColour, float* __restrict__ outVariance)
{
	RL_MATH_PROLOGUE();
	int x, y;
	if (!TilePixel(W, H, x, y)) return;
	const size_t p = (size_t)y * W + (size_t)x;
	const VfValue o = guides[p].prim == -1 ? I[p] : VfFilterPixel(I, guides, (int)W, (int)H, x, y, step, c);   // (a pass-through record's var is +0: k_vf_pack)
	if (!LAST) { next[p] = o; return; }
	outColour[p] = make_float4(o.r, o.g, o.b, 1.0f);
	if (outVariance) outVariance[p] = o.var;
}
template __global__ void k_vf_iter<false>(RL_VF_ITER_ARGS);
template __global__ void k_vf_iter<true>(RL_VF_ITER_ARGS);

} // namespace rl
