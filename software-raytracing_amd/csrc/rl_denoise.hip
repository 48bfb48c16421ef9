// Edge-avoiding a-trous wavelet denoiser (Dammertz et al. 2010, "Edge-Avoiding A-Trous Wavelet Transform for fast Global
// Illumination Filtering"), guided by the two AOVs the front-ends already render: Albedo (linear RGB) and MicrosurfaceNormal
// (0.5 * N + 0.5, 0 where the camera ray missed).  RaylibAMD_Denoise runs it on the device (DeviceDenoise), RaylibAMD_DenoiseHost
// on the host (DenoiseHost); both evaluate the per-pixel functions below, so one source defines the arithmetic and the two agree
// bit for bit (-ffp-contract=off on both sides, expf_ of rl_glibc_math.h).
//
// Per pixel p and colour channel (every non-finite input channel is read as 0):
//   a  = (albedo given && A > 1e-3f) ? A : 1          demodulation divisor
//   I0 = C / a                                         (0 where that is not finite; non-finite C channels are counted and logged)
//   n  = 2 * N - 1                                     (a miss decodes to (-1, -1, -1): apart from every surface)
//   g(x) = bHDR ? x / (1 + x) : x                      colour-distance space (x < 0 is taken as 0 under bHDR)
// Iteration i = 0 .. K-1, step s = 2^i, taps q = p + s * (dx, dy), dy outer, dx inner, both -2 .. 2, taps outside the image skipped:
//   w = k[dx+2] * k[dy+2] * expf_(-(dc * invC_i + dn * invN + da * invA)),  k = {1/16, 1/4, 3/8, 1/4, 1/16}
//   dc = sum_ch (g(Ii(q)) - g(Ii(p)))^2,  dn = sum_ch (n(q) - n(p))^2 (0 without N),  da = sum_ch (A(q) - A(p))^2 (0 without A)
//   I(i+1)(p) = sum w * Ii(q) / sum w, summed in tap order
// invC_i = 4^i / sigmaColor^2 (the colour tolerance halves per step), invN = 1 / sigmaNormal^2, invA = 1 / sigmaAlbedo^2: computed on
// the host once (DenoiseInv) and handed to both paths as they are.  out = IK * a, alpha 1.
#include <hip/hip_runtime.h>

#include "rl_host.h"
// exact-libm tables in LDS for expf_ (rl_glibc_math.h): filled by rlm_fill_lds_tables() at the top of k_dn_iter
#define RLM_LDS_TABLES 1
static __shared__ double rlm_lds_tab[80];
#include "rl_glibc_math.h"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <vector>

namespace rl {

namespace {

#define DN_HD __host__ __device__ static inline

DN_HD float Fin(float v) { return isfinite(v) ? v : 0.0f; }
DN_HD float Demod(float a) { return a > 1e-3f ? a : 1.0f; }
DN_HD float WeightSpace(float x, bool hdr)
{
	if (!hdr) return x;
	const float c = x > 0.0f ? x : 0.0f;
	return c / (1.0f + c);
}

// preparation of one pixel: irradiance (xyz) from colour and albedo; returns the number of non-finite colour channels
DN_HD int PrepPixel(float4 c, const float4* A, size_t p, float4& I)
{
	const float ax = A ? Demod(Fin(A[p].x)) : 1.0f, ay = A ? Demod(Fin(A[p].y)) : 1.0f, az = A ? Demod(Fin(A[p].z)) : 1.0f;
	const int bad = !isfinite(c.x) + !isfinite(c.y) + !isfinite(c.z);
	I.x = Fin(Fin(c.x) / ax); I.y = Fin(Fin(c.y) / ay); I.z = Fin(Fin(c.z) / az); I.w = 0.0f;
	return bad;
}

DN_HD float3 Normal(const float4* N, size_t q)
{
	const float4 v = N[q];
	return make_float3(2.0f * Fin(v.x) - 1.0f, 2.0f * Fin(v.y) - 1.0f, 2.0f * Fin(v.z) - 1.0f);
}
DN_HD float3 Albedo(const float4* A, size_t q)
{
	const float4 v = A[q];
	return make_float3(Fin(v.x), Fin(v.y), Fin(v.z));
}
DN_HD float Dist2(float3 a, float3 b)
{
	const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z;
	return d0 * d0 + d1 * d1 + d2 * d2;
}

// one a-trous step for pixel (x, y): N / A may be null (guide absent)
DN_HD float4 FilterPixel(const float4* I, const float4* N, const float4* A, int W, int H, int x, int y, int s,
                         float invC, float invN, float invA, bool hdr)
{
	const float k[5] = { 1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f };
	const size_t p = (size_t)y * (size_t)W + (size_t)x;
	const float4 ip = I[p];
	const float3 gp = make_float3(WeightSpace(ip.x, hdr), WeightSpace(ip.y, hdr), WeightSpace(ip.z, hdr));
	float3 np = make_float3(0.0f, 0.0f, 0.0f), ap = make_float3(0.0f, 0.0f, 0.0f);
	if (N) np = Normal(N, p);
	if (A) ap = Albedo(A, p);
	float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
	for (int dy = -2; dy <= 2; ++dy) {
		const int qy = y + s * dy;
		if (qy < 0 || qy >= H) continue;
		for (int dx = -2; dx <= 2; ++dx) {
			const int qx = x + s * dx;
			if (qx < 0 || qx >= W) continue;
			const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
			const float4 iq = I[q];
			const float3 gq = make_float3(WeightSpace(iq.x, hdr), WeightSpace(iq.y, hdr), WeightSpace(iq.z, hdr));
			const float dc = Dist2(gq, gp);
			const float dn = N ? Dist2(Normal(N, q), np) : 0.0f;
			const float da = A ? Dist2(Albedo(A, q), ap) : 0.0f;
			const float w = (k[dx + 2] * k[dy + 2]) * rlm::expf_(-(dc * invC + dn * invN + da * invA));
			sw = sw + w;
			sx = sx + w * iq.x; sy = sy + w * iq.y; sz = sz + w * iq.z;
		}
	}
	return make_float4(sx / sw, sy / sw, sz / sw, 0.0f);
}

DN_HD float4 RemodPixel(float4 I, const float4* A, size_t p)
{
	if (!A) return make_float4(I.x, I.y, I.z, 1.0f);
	return make_float4(I.x * Demod(Fin(A[p].x)), I.y * Demod(Fin(A[p].y)), I.z * Demod(Fin(A[p].z)), 1.0f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// kernels: a 16 x 16 pixel tile per block, so a wave64 covers 16 x 4 pixels and a tap row of it is one 256-byte run of float4.
// The block is one-dimensional (256 threads, pixel (tid % 16, tid / 16) of the tile): rlm_fill_lds_tables() indexes the tables by threadIdx.x
// alone and needs 32 distinct values of it.
constexpr int DN_BX = 16, DN_BY = 16;
__device__ __forceinline__ int TileX() { return (int)blockIdx.x * DN_BX + (int)(threadIdx.x % DN_BX); }
__device__ __forceinline__ int TileY() { return (int)blockIdx.y * DN_BY + (int)(threadIdx.x / DN_BX); }

__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_prep(const float4* __restrict__ C, const float4* __restrict__ A, int W, int H,
                                                           float4* __restrict__ I, unsigned int* __restrict__ nonFinite)
{
	const int x = TileX(), y = TileY();
	if (x >= W || y >= H) return;
	const size_t p = (size_t)y * (size_t)W + (size_t)x;
	float4 v;
	const int bad = PrepPixel(C[p], A, p, v);
	I[p] = v;
	if (bad) atomicAdd(nonFinite, (unsigned int)bad);
}

__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_iter(const float4* __restrict__ I, const float4* __restrict__ N, const float4* __restrict__ A,
                                                           int W, int H, int s, float invC, float invN, float invA, int hdr, float4* __restrict__ out)
{
	rlm::rlm_fill_lds_tables();   // every thread, before any returns: it ends in a barrier
	const int x = TileX(), y = TileY();
	if (x >= W || y >= H) return;
	out[(size_t)y * (size_t)W + (size_t)x] = FilterPixel(I, N, A, W, H, x, y, s, invC, invN, invA, hdr != 0);
}

__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_remod(const float4* __restrict__ I, const float4* A, int W, int H, float4* out)
{
	// (A and out may be the same image: each thread reads its own pixel of A before it writes that pixel of out)
	const int x = TileX(), y = TileY();
	if (x >= W || y >= H) return;
	const size_t p = (size_t)y * (size_t)W + (size_t)x;
	out[p] = RemodPixel(I[p], A, p);
}

// the filter's constants, computed once on the host for both paths
struct DenoiseInv { float invC[8], invN, invA; };
DenoiseInv MakeInv(const RaylibAMDDenoiseParams& P)
{
	DenoiseInv v;
	for (int i = 0; i < 8; ++i) v.invC[i] = (float)(1u << (2 * i)) / (P.sigmaColor * P.sigmaColor);
	v.invN = 1.0f / (P.sigmaNormal * P.sigmaNormal);
	v.invA = 1.0f / (P.sigmaAlbedo * P.sigmaAlbedo);
	return v;
}

// device state of the filter: a stream and the two ping-pong buffers on the images' device, grown as needed
struct DenoiseDev {
	std::mutex mu;
	int device = -1;
	hipStream_t stream = nullptr;
	float4* buf[2] = { nullptr, nullptr };
	size_t bufBytes = 0;
	unsigned int* counter = nullptr;
};
DenoiseDev g_dn;

#define DN_OK(x) do { if ((x) != hipSuccess) { Log("RaylibAMD_Denoise: %s failed", #x); return false; } } while (0)

// the device buffer of an input image; `upload`: its pixels live only on the host and go to that buffer first (on the filter's stream)
const float4* InputPixels(Image* img, bool& upload)
{
	upload = false;
	if (!img) return nullptr;
	void* dev = DeviceImagePixels(*img);
	upload = dev && !img->devValid;
	return (const float4*)dev;
}

} // namespace

void DenoiseHost(uint32_t W, uint32_t H, const float* color, bool hdr, const float* albedo, const float* normal,
                 const RaylibAMDDenoiseParams& P, float* out)
{
	const size_t n = (size_t)W * H;
	if (n == 0) return;
	const DenoiseInv inv = MakeInv(P);
	// float4 copies of the caller's arrays (which need not be 16-byte aligned, and `out` may be one of them)
	auto copy = [n](const float* src) { std::vector<float4> v(src ? n : 0); if (src) memcpy(v.data(), src, n * sizeof(float4)); return v; };
	const std::vector<float4> C = copy(color), A = copy(albedo), N = copy(normal);
	const float4* Ap = albedo ? A.data() : nullptr;
	const float4* Np = normal ? N.data() : nullptr;
	std::vector<float4> I(n), J(n);
	uint64_t bad = 0;
	for (size_t p = 0; p < n; ++p) bad += (uint64_t)PrepPixel(C[p], Ap, p, I[p]);
	if (bad) Log("RaylibAMD_DenoiseHost: %llu non-finite colour channels replaced by 0", (unsigned long long)bad);
	for (int i = 0; i < P.iterations; ++i) {
		for (int y = 0; y < (int)H; ++y)
			for (int x = 0; x < (int)W; ++x)
				J[(size_t)y * W + x] = FilterPixel(I.data(), Np, Ap, (int)W, (int)H, x, y, 1 << i, inv.invC[i], inv.invN, inv.invA, hdr);
		I.swap(J);
	}
	for (size_t p = 0; p < n; ++p) { const float4 v = RemodPixel(I[p], Ap, p); memcpy(out + 4 * p, &v, sizeof(float4)); }
}

bool DeviceDenoise(Image& main, bool hdr, Image* albedo, Image* normal, Image& out, const RaylibAMDDenoiseParams& P)
{
	const uint32_t W = main.width, H = main.height;
	const size_t n = (size_t)W * H;
	if (n == 0) { if (out.width != W || out.height != H) out.Reallocate(W, H, 0.0f, 0.0f, 0.0f, 1.0f); return true; }
	std::lock_guard<std::mutex> lk(g_dn.mu);
	Image* inputs[3] = { &main, albedo, normal };
	const float4* dev[3];
	bool upload[3];
	for (int k = 0; k < 3; ++k) dev[k] = InputPixels(inputs[k], upload[k]);
	const float4 *C = dev[0], *A = dev[1], *N = dev[2];
	if (!C || (albedo && !A) || (normal && !N)) { Log("RaylibAMD_Denoise: an input could not be placed on the device"); return false; }
	// out is reallocated to main's size (out == main, or a guide, already has it: their buffers are not touched)
	if (out.width != W || out.height != H) out.Reallocate(W, H, 0.0f, 0.0f, 0.0f, 1.0f);
	float4* O = (float4*)DeviceImagePixels(out);
	if (!O) { Log("RaylibAMD_Denoise: no device buffer for the output image"); return false; }
	hipPointerAttribute_t attr;
	DN_OK(hipPointerGetAttributes(&attr, C));
	DN_OK(hipSetDevice(attr.device));
	if (g_dn.device != attr.device) {   // (first call, or the images' device changed)
		if (g_dn.stream) { (void)hipStreamDestroy(g_dn.stream); g_dn.stream = nullptr; }
		for (float4*& b : g_dn.buf) if (b) { (void)hipFree(b); b = nullptr; }
		if (g_dn.counter) { (void)hipFree(g_dn.counter); g_dn.counter = nullptr; }
		g_dn.bufBytes = 0;
		DN_OK(hipStreamCreateWithFlags(&g_dn.stream, hipStreamNonBlocking));
		DN_OK(hipMalloc(&g_dn.counter, sizeof(unsigned int)));
		g_dn.device = attr.device;
	}
	const size_t bytes = n * sizeof(float4);
	if (g_dn.bufBytes < bytes) {
		for (float4*& b : g_dn.buf) if (b) { (void)hipFree(b); b = nullptr; }
		g_dn.bufBytes = 0;
		DN_OK(hipMalloc(&g_dn.buf[0], bytes));
		DN_OK(hipMalloc(&g_dn.buf[1], bytes));
		g_dn.bufBytes = bytes;
	}
	hipStream_t st = g_dn.stream;
	const DenoiseInv inv = MakeInv(P);
	const dim3 block(DN_BX * DN_BY), grid((W + DN_BX - 1) / DN_BX, (H + DN_BY - 1) / DN_BY);
	for (int k = 0; k < 3; ++k)   // (an image passed twice is uploaded twice: the same bytes)
		if (upload[k]) DN_OK(hipMemcpyAsync((void*)dev[k], inputs[k]->rgba.data(), bytes, hipMemcpyHostToDevice, st));
	DN_OK(hipMemsetAsync(g_dn.counter, 0, sizeof(unsigned int), st));
	hipLaunchKernelGGL(k_dn_prep, grid, block, 0, st, C, A, (int)W, (int)H, g_dn.buf[0], g_dn.counter);
	DN_OK(hipGetLastError());
	int cur = 0;
	for (int i = 0; i < P.iterations; ++i, cur ^= 1) {
		hipLaunchKernelGGL(k_dn_iter, grid, block, 0, st, (const float4*)g_dn.buf[cur], N, A, (int)W, (int)H, 1 << i,
		                   inv.invC[i], inv.invN, inv.invA, hdr ? 1 : 0, g_dn.buf[cur ^ 1]);
		DN_OK(hipGetLastError());
	}
	hipLaunchKernelGGL(k_dn_remod, grid, block, 0, st, (const float4*)g_dn.buf[cur], A, (int)W, (int)H, O);
	DN_OK(hipGetLastError());
	unsigned int bad = 0;
	DN_OK(hipMemcpyAsync(&bad, g_dn.counter, sizeof(bad), hipMemcpyDeviceToHost, st));
	DN_OK(hipStreamSynchronize(st));
	if (bad) Log("RaylibAMD_Denoise: %u non-finite colour channels replaced by 0", bad);
	for (int k = 0; k < 3; ++k) if (upload[k]) inputs[k]->devValid = true;   // host and device copies agree (hostStale stays false)
	out.devValid = true;
	out.hostStale = true;   // read back when the pixels are asked for (Image::SyncHost), as after Raylib_Render
	out.Touch();
	return true;
}

} // namespace rl
