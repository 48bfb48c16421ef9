// The lightmap kernels (RaylibAMD_BakeLightmap, include/raylib_amd.h; launched by rl_rt_lightmap.hip): a rasteriser in lightmap-UV space that is balanced over
// (triangle, texel) pairs rather than over triangles or texels -- one triangle may fill the atlas and a million may be smaller than a texel each --, the scans
// between its stages, and the atlas stages behind the gather.  Nothing here walks a tree or shades: the unit shares no device function with the render kernels.
//   k_lm_setup     per triangle: snap, area, the rectangle of texel centres in its box, that rectangle's texel count
//   (scan)         the counts' exclusive scan, 64-bit: pair p belongs to the triangle t with offs[t] <= p < offs[t + 1]
//   k_lm_cover     per pair: binary search for t, the coverage test, atomicMin(owner[texel], t) -- a vector atomic whose result does not depend on arrival order
//   k_lm_points    per texel: statements 3 to 5 again from the owner alone (nothing depends on which lane won), first for the flags, then, after the flags'
//                  scan has ranked them, for the records
//   k_lm_scatter, k_lm_dilate   statements 8 and 9

// ---- settings ----
// None: integers, single float operations without FMA (the Makefile's -ffp-contract=off), IEEE double division, rlm::rcp1_ and rlm::sqrtf_ (rl_glibc_math.h) for 1 / x and sqrt, as rl_lightmap.h.

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_lightmap.h"

namespace rl {

static_assert(RL_BLOCK == 256, "the scans' tiles and LDS arrays are sized for 256 lanes");

__global__ void __launch_bounds__(RL_BLOCK)
k_lm_setup(const float* __restrict__ tris, const float* __restrict__ uv, uint32_t numTris, int32_t width, int32_t height, DLmTri* __restrict__ rec, unsigned long long* __restrict__ counts)
{
	const uint32_t k = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (k >= numTris) return;
	const float* src = uv ? uv + (size_t)k * 6 : tris + (size_t)k * 26 + 18;
	float t[6];
#pragma unroll
	for (int i = 0; i < 6; ++i) t[i] = src[i];
	DLmTri r; int64_t A2; int32_t xlo = 0, ylo = 0, rw = 0;
	uint32_t cells = 0u;
	if (lm::Snap(t, width, height, r.X, r.Y, A2)) cells = lm::Rect(r.X, r.Y, width, height, xlo, ylo, rw);
	else { r.X[0] = r.X[1] = r.X[2] = 0; r.Y[0] = r.Y[1] = r.Y[2] = 0; }
	r.lo = (uint32_t)xlo | ((uint32_t)ylo << 16); r.rw = cells ? (uint32_t)rw : 0u;
	rec[k] = r;
	counts[k] = cells;
}

// the corners and twice the area again from the record (exact: the record holds the snapped integers)
__device__ __forceinline__ int64_t AreaOf(const DLmTri& r)
{
	return (int64_t)(r.X[1] - r.X[0]) * (int64_t)(r.Y[2] - r.Y[0]) - (int64_t)(r.Y[1] - r.Y[0]) * (int64_t)(r.X[2] - r.X[0]);
}

__global__ void __launch_bounds__(RL_BLOCK)
k_lm_cover(const DLmTri* __restrict__ rec, const unsigned long long* __restrict__ offs, uint32_t numTris, unsigned long long base, uint32_t pairs, int32_t width, uint32_t numTexels, uint32_t* __restrict__ owner)
{
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= pairs) return;
	const unsigned long long p = base + i;
	// offs[0] = 0 <= p < offs[numTris]: the last t with offs[t] <= p (triangles without texels share their successor's offset and are never the last)
	uint32_t lo = 0u, hi = numTris;
	while (hi - lo > 1u) {
		const uint32_t mid = lo + (hi - lo) / 2u;
		if (offs[mid] <= p) lo = mid; else hi = mid;
	}
	const DLmTri r = rec[lo];
	const uint32_t local = (uint32_t)(p - offs[lo]);   // < the rectangle's texels <= 2^28
	if (r.rw == 0u) return;                            // (unreachable: such a triangle has no pairs)
	const int32_t x = (int32_t)(r.lo & 0xffffu) + (int32_t)(local % r.rw), y = (int32_t)(r.lo >> 16) + (int32_t)(local / r.rw);
	int64_t wB, wC;
	const uint32_t at = (uint32_t)y * (uint32_t)width + (uint32_t)x;
	if (at >= numTexels) return;                       // (unreachable: the rectangle was clipped to the atlas)
	if (lm::Cover(r.X, r.Y, AreaOf(r), x, y, wB, wC)) atomicMin(owner + at, lo);
}

template <bool WRITE> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_points(const DLmTri* __restrict__ rec, const float* __restrict__ tris, const uint32_t* __restrict__ owner, uint32_t* __restrict__ rank, int32_t width, uint32_t numTexels,
            float time, float4* __restrict__ points, uint32_t* __restrict__ texel, unsigned long long capacity)
{
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= numTexels) return;
	uint32_t at = 0u;
	if (WRITE) {
		at = rank[i];
		if (rank[i + 1u] == at || at >= capacity) return;
	}
	const uint32_t k = owner[i];
	bool has = false;
	float pos[3], nrm[3];
	if (k != 0xffffffffu) {
		const DLmTri r = rec[k];
		const int64_t A2 = AreaOf(r);
		int64_t wB, wC;
		(void)lm::Cover(r.X, r.Y, A2, (int32_t)(i % (uint32_t)width), (int32_t)(i / (uint32_t)width), wB, wC);
		float t[18];
		const float* src = tris + (size_t)k * 26;
#pragma unroll
		for (int j = 0; j < 18; ++j) t[j] = src[j];
		has = lm::Point(t, wB, wC, A2, pos, nrm);
	}
	if (!WRITE) { rank[i] = has ? 1u : 0u; return; }
	if (!has) return;   // (never: the flag was this computation)
	points[2 * (size_t)at] = make_float4(pos[0], pos[1], pos[2], time);
	points[2 * (size_t)at + 1] = make_float4(nrm[0], nrm[1], nrm[2], __uint_as_float(i));
	if (texel) texel[at] = i;
}

// ---- the scan ----
// a block's inclusive scan of one value per lane through LDS (Hillis and Steele: log2(N) rounds); sh holds N values
template <typename T, int N>
__device__ __forceinline__ T BlockInclusive(T v, T* sh)
{
	const uint32_t tid = threadIdx.x;
	sh[tid] = v;
	__syncthreads();
	for (uint32_t off = 1u; off < (uint32_t)N; off <<= 1) {
		const T a = tid >= off ? sh[tid - off] : (T)0;
		__syncthreads();
		sh[tid] += a;
		__syncthreads();
	}
	return sh[tid];
}

template <typename T> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_scan_reduce(const T* __restrict__ data, unsigned long long n, T* __restrict__ sums)
{
	__shared__ T sh[RL_BLOCK];
	const unsigned long long first = (unsigned long long)blockIdx.x * RL_SCAN_TILE + (unsigned long long)threadIdx.x * RL_SCAN_PER;
	T s = 0;
#pragma unroll
	for (int j = 0; j < RL_SCAN_PER; ++j) if (first + j < n) s += data[first + j];
	const T incl = BlockInclusive<T, RL_BLOCK>(s, sh);
	if (threadIdx.x == RL_BLOCK - 1) sums[blockIdx.x] = incl;
}

template <typename T> __global__ void __launch_bounds__(RL_SCAN_SUMS_BLOCK)
k_lm_scan_sums(T* __restrict__ sums, uint32_t numTiles)
{
	__shared__ T sh[RL_SCAN_SUMS_BLOCK];
	T carry = 0;
	for (uint32_t base = 0u; base < numTiles; base += RL_SCAN_SUMS_BLOCK) {
		const uint32_t i = base + threadIdx.x;
		const T v = i < numTiles ? sums[i] : (T)0;
		const T incl = BlockInclusive<T, RL_SCAN_SUMS_BLOCK>(v, sh);
		if (i < numTiles) sums[i] = carry + (incl - v);
		carry += sh[RL_SCAN_SUMS_BLOCK - 1];
		__syncthreads();   // (the next round overwrites sh)
	}
	if (threadIdx.x == 0) sums[numTiles] = carry;
}

template <typename T> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_scan_add(T* __restrict__ data, unsigned long long n, const T* __restrict__ sums, uint32_t numTiles)
{
	__shared__ T sh[RL_BLOCK];
	const unsigned long long first = (unsigned long long)blockIdx.x * RL_SCAN_TILE + (unsigned long long)threadIdx.x * RL_SCAN_PER;
	T v[RL_SCAN_PER];
	T s = 0;
#pragma unroll
	for (int j = 0; j < RL_SCAN_PER; ++j) { v[j] = first + j < n ? data[first + j] : (T)0; s += v[j]; }
	T run = sums[blockIdx.x] + (BlockInclusive<T, RL_BLOCK>(s, sh) - s);
#pragma unroll
	for (int j = 0; j < RL_SCAN_PER; ++j) { if (first + j < n) data[first + j] = run; run += v[j]; }
	if (blockIdx.x == numTiles - 1u && threadIdx.x == 0) data[n] = sums[numTiles];
}

// ---- the atlas ----
template <int C> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_scatter(const uint32_t* __restrict__ rank, const float* __restrict__ values, uint32_t numTexels, float* __restrict__ atlas, uint8_t* __restrict__ coverage)
{
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= numTexels) return;
	const uint32_t at = rank[i];
	const bool has = rank[i + 1u] != at;
	float* dst = atlas + (size_t)i * C;
	const float* src = values + (size_t)at * C;
#pragma unroll
	for (int c = 0; c < C; ++c) dst[c] = has ? src[c] : 0.0f;
	coverage[i] = has ? 1 : 0;
}

template <int C> __global__ void __launch_bounds__(RL_BLOCK)
k_lm_dilate(const float* __restrict__ src, const uint8_t* __restrict__ srcCov, float* __restrict__ dst, uint8_t* __restrict__ dstCov, int32_t width, int32_t height, int32_t pass)
{
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= (uint32_t)width * (uint32_t)height) return;
	const int32_t x = (int32_t)(i % (uint32_t)width), y = (int32_t)(i / (uint32_t)width);
	const uint8_t cov = srcCov[i];
	// the neighbours in the contract's order, those inside the atlas with coverage != 0 as bits of `mask`
	const int dx[8] = { -1, 0, 1, -1, 1, -1, 0, 1 }, dy[8] = { -1, -1, -1, 0, 0, 1, 1, 1 };
	uint32_t mask = 0u, m = 0u;
	if (cov == 0) {
#pragma unroll
		for (int j = 0; j < 8; ++j) {
			const int32_t nx = x + dx[j], ny = y + dy[j];
			if (nx >= 0 && ny >= 0 && nx < width && ny < height && srcCov[(size_t)ny * (size_t)width + (size_t)nx] != 0) { mask |= 1u << j; ++m; }
		}
	}
	float* out = dst + (size_t)i * C;
	if (m == 0u) {
		const float* in = src + (size_t)i * C;
#pragma unroll
		for (int c = 0; c < C; ++c) out[c] = in[c];
		dstCov[i] = cov;
		return;
	}
	const float k = rlm::rcp1_((float)m);
	for (int c = 0; c < C; ++c) {
		float s = 0.0f;
#pragma unroll
		for (int j = 0; j < 8; ++j)
			if (mask & (1u << j)) s = s + src[((size_t)(y + dy[j]) * (size_t)width + (size_t)(x + dx[j])) * C + c];
		out[c] = s * k;
	}
	if (C == 4) out[3] = 1.0f;
	dstCov[i] = (uint8_t)(1 + pass);
}

// ---- instances ----
template __global__ void k_lm_points<false>(const DLmTri* __restrict__, const float* __restrict__, const uint32_t* __restrict__, uint32_t* __restrict__, int32_t, uint32_t, float, float4* __restrict__, uint32_t* __restrict__, unsigned long long);
template __global__ void k_lm_points<true>(const DLmTri* __restrict__, const float* __restrict__, const uint32_t* __restrict__, uint32_t* __restrict__, int32_t, uint32_t, float, float4* __restrict__, uint32_t* __restrict__, unsigned long long);
RL_LM_SCAN_INSTANCES(, uint32_t)
RL_LM_SCAN_INSTANCES(, unsigned long long)
RL_LM_ATLAS_INSTANCES(, 4)
RL_LM_ATLAS_INSTANCES(, 27)

} // namespace rl
