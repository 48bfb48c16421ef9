// The lightmap atlas filter (include/raylib_amd.h, statement F; RaylibAMD_BakeLightmapFiltered, RaylibAMD_FilterLightmap, RaylibAMD_FilterLightmapHost): an
// edge-avoiding a-trous filter, as rl_denoise.hip's, whose guides are the covered texels' gather points and whose taps are covered texels only.  FilterPoint
// below is the statement for one texel; k_lm_filter (launched by rl_rt_lightmap.hip) and the host oracle FilterLightmapHost both call it, so one source defines
// the arithmetic and the two agree bit for bit (-ffp-contract=off on both sides, expf_ of rl_glibc_math.h).
//
// The shape.  A thread stands for a covered texel in compacted form -- point i of the raster's `count` --, not for a texel of an atlas tile: the values the
// gather leaves are compacted already, so the filter runs in front of the scatter on two arrays of count x C floats and never reads, writes or launches a lane
// for a gutter (a grid atlas with margins is a third gutters; a packed one of many small charts more).  A tap's point is found through the scanned ranks the
// scatter reads anyway: texel q has a point when rank[q + 1] != rank[q], and that point is rank[q].  The ranks ascend with the texel index, so the lanes of a
// wave stand for neighbouring texels of a row and a tap row of theirs is a run of neighbouring points: the loads coalesce as a tile's would.  A tap's weight is
// computed once and the channels run inside it: SH9 keeps 27 running sums and the weights' sum in registers.
//   k_lm_filter   one iteration, one thread per point
//   k_lm_take     RaylibAMD_FilterLightmap: the covered texels' values out of the caller's atlas, one thread per texel

// ---- the device library ----
#include "rl_kernels.h"   // (rl_dev_core.h: the exact-libm tables in LDS and RL_MATH_PROLOGUE, which fills them)
#include "rl_lightmap.h"

#include <string.h>
#include <new>
#include <vector>

namespace rl {

#define LF_HD __host__ __device__ static inline

LF_HD float LfFin(float v) { return lm::finite_(v) ? v : 0.0f; }
LF_HD float LfKey(float x)
{
	const float c = x > 0.0f ? x : 0.0f;
	return c / (1.0f + c);
}
LF_HD float LfDist2(float a0, float a1, float a2, float b0, float b1, float b2)
{
	const float d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2;
	return d0 * d0 + d1 * d1 + d2 * d2;
}
// a point's C values: on the device an IRRADIANCE value is one 16-byte load (the arrays are the library's, count x 4 floats from an allocation's start)
template <int C> LF_HD const float* LfValues(const float* values, uint32_t i)
{
	const float* p = values + (size_t)i * C;
#if defined(__HIP_DEVICE_COMPILE__)
	if (C == 4) p = (const float*)__builtin_assume_aligned(p, 16);
#endif
	return p;
}

// Statement F5 for point i, whose texel is t: one iteration src -> dst[i].  points: two float4 per point (pos, time | normal, stream).  prep: src is the
// input (F3), whose channels that are not finite read as 0.
template <int C>
LF_HD void FilterPoint(const uint32_t* rank, const float4* points, const float* src, float* dst, uint32_t i, uint32_t t, int W, int H, int s,
                       float invC, float invN, float invP, bool prep)
{
	constexpr int NF = C == 4 ? 3 : C;   // the filtered channels
	const float k[5] = { 1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f };
	const int x = (int)(t % (uint32_t)W), y = (int)(t / (uint32_t)W);
	const float* ip = LfValues<C>(src, i);
	const float p0 = prep ? LfFin(ip[0]) : ip[0], p1 = prep ? LfFin(ip[1]) : ip[1], p2 = prep ? LfFin(ip[2]) : ip[2];
	const float gp0 = LfKey(p0), gp1 = LfKey(p1), gp2 = LfKey(p2);
	const float4 Pp = points[2 * (size_t)i], Np = points[2 * (size_t)i + 1];
	float sw = 0.0f, sum[NF];
	for (int c = 0; c < NF; ++c) sum[c] = 0.0f;
	for (int dy = -2; dy <= 2; ++dy) {
		const int qy = y + s * dy;
		if (qy < 0 || qy >= H) continue;
		for (int dx = -2; dx <= 2; ++dx) {
			const int qx = x + s * dx;
			if (qx < 0 || qx >= W) continue;
			const uint32_t q = (uint32_t)qy * (uint32_t)W + (uint32_t)qx;
			const uint32_t r = rank[q];
			if (rank[q + 1u] == r) continue;   // not a covered texel
			const float* iq = LfValues<C>(src, r);
			float v[NF];
			for (int c = 0; c < NF; ++c) v[c] = prep ? LfFin(iq[c]) : iq[c];
			const float4 Pq = points[2 * (size_t)r], Nq = points[2 * (size_t)r + 1];
			const float dc = LfDist2(LfKey(v[0]), LfKey(v[1]), LfKey(v[2]), gp0, gp1, gp2);
			const float dn = LfDist2(Nq.x, Nq.y, Nq.z, Np.x, Np.y, Np.z);
			const float dp = LfDist2(Pq.x, Pq.y, Pq.z, Pp.x, Pp.y, Pp.z);
			const float w = (k[dx + 2] * k[dy + 2]) * rlm::expf_(-(dc * invC + dn * invN + dp * invP));
			sw = sw + w;
			for (int c = 0; c < NF; ++c) sum[c] = sum[c] + w * v[c];
		}
	}
	float* o = dst + (size_t)i * C;
	for (int c = 0; c < NF; ++c) o[c] = sum[c] / sw;
	if (C == 4) o[3] = 1.0f;
}

// ---- the kernels ----
// One-dimensional blocks: RL_MATH_PROLOGUE() indexes the tables by threadIdx.x and ends in a barrier, so every thread reaches it before any returns.
template <int C> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_filter(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ texel, const float4* __restrict__ points, const float* __restrict__ src, float* __restrict__ dst,
            uint32_t count, int32_t width, int32_t height, int32_t step, float invC, float invN, float invP, int32_t prep)
{
	RL_MATH_PROLOGUE();
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= count) return;
	FilterPoint<C>(rank, points, src, dst, i, texel[i], width, height, step, invC, invN, invP, prep != 0);
}

template <int C> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_take(const uint32_t* __restrict__ rank, const float* __restrict__ atlas, uint32_t numTexels, float* __restrict__ values)
{
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= numTexels) return;
	const uint32_t at = rank[i];
	if (rank[i + 1u] == at) return;
	const float* src = atlas + (size_t)i * C;
	float* dst = values + (size_t)at * C;
#pragma unroll
	for (int c = 0; c < C; ++c) dst[c] = src[c];
}

// ---- instances ----
RL_LM_FILTER_INSTANCES(, 4)
RL_LM_FILTER_INSTANCES(, 27)

// ---- the host ----
LmFilterInv MakeLmFilterInv(const RaylibAMDLightmapFilterParams& F)
{
	LmFilterInv v;
	for (int i = 0; i < 8; ++i) {
		v.invC[i] = (float)(1u << (2 * i)) / (F.sigmaColor * F.sigmaColor);
		const float sp = F.sigmaPosition * (float)(1u << i);
		v.invP[i] = 1.0f / (sp * sp);
	}
	v.invN = 1.0f / (F.sigmaNormal * F.sigmaNormal);
	return v;
}

template <int C>
static void FilterHost(int32_t W, int32_t H, const RaylibAMDLightmapFilterParams& F, const uint32_t* rank, const float4* points, const uint32_t* texel, uint32_t count,
                       std::vector<float>& a, std::vector<float>& b)
{
	const LmFilterInv inv = MakeLmFilterInv(F);
	for (int i = 0; i < F.iterations; ++i) {
		for (uint32_t p = 0; p < count; ++p) FilterPoint<C>(rank, points, a.data(), b.data(), p, texel[p], W, H, 1 << i, inv.invC[i], inv.invN, inv.invP[i], i == 0);
		a.swap(b);
	}
}

bool FilterLightmapHost(int32_t W, int32_t H, int32_t kind, const RaylibAMDLightmapFilterParams& F, const RaylibAMDGatherPoint* points, const uint32_t* texel,
                        int64_t count, const float* values, float* outValues)
{
	const uint64_t nTex = (uint64_t)W * (uint64_t)H;
	for (int64_t p = 0; p < count; ++p)
		if (texel[p] >= nTex || (p > 0 && texel[p] <= texel[p - 1])) {
			Log("RaylibAMD_FilterLightmapHost: texel[%lld] = %u is not above its predecessor, or not inside the %d x %d atlas", (long long)p, texel[p], W, H);
			return false;
		}
	if (count == 0) return true;
	const uint32_t n = (uint32_t)count, C = kind == RAYLIB_AMD_GATHER_SH9 ? 27u : 4u;   // (count <= the atlas' texels <= 2^28)
	// the scanned ranks the kernel finds a tap's point through, and copies of the caller's arrays: float4 records for the points (the caller's need not be
	// 16-byte aligned), two arrays for the iterations (outValues may be values)
	std::vector<uint32_t> rank; std::vector<float4> pts; std::vector<float> a, b;
	try { rank.resize((size_t)nTex + 1); pts.resize(2 * (size_t)n); a.assign(values, values + (size_t)n * C); b.resize((size_t)n * C); }
	catch (const std::bad_alloc&) { Log("RaylibAMD_FilterLightmapHost: no memory for a %d x %d atlas of %u points", W, H, n); return false; }
	uint32_t r = 0;
	for (uint64_t t = 0; t < nTex; ++t) { rank[(size_t)t] = r; if (r < n && texel[r] == t) ++r; }
	rank[(size_t)nTex] = r;
	memcpy(pts.data(), points, (size_t)n * sizeof(RaylibAMDGatherPoint));
	if (C == 27u) FilterHost<27>(W, H, F, rank.data(), pts.data(), texel, n, a, b);
	else FilterHost<4>(W, H, F, rank.data(), pts.data(), texel, n, a, b);
	memcpy(outValues, a.data(), (size_t)n * C * sizeof(float));
	return true;
}

} // namespace rl
