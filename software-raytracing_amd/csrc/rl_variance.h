// The variance-guided filter's arithmetic (include/raylib_amd.h statements S3 to S6), one statement for the host and the device: the kernels of
// rl_variance.hip and the host oracle RaylibAMD_FilterVarianceHost (rl_oracle.cc) compile this file.  Everything is float, single IEEE operations without FMA
// (the Makefile's -ffp-contract=off on either side); a / b and sqrt are the compiler's correctly rounded ones, expf is rl_glibc_math.h's expf_.  Sums run in
// the stated tap order from +0, left to right: a + b + c is (a + b) + c.
//
// Both sides work on the same packed planes, which the call makes once from the caller's: a guide record per pixel (VfGuide, 32 bytes: world position, prim,
// normal) and a value record per pixel (VfValue, 16 bytes: the colour with its variance in w), so a tap is three 16-byte loads.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rl_glibc_math.h"

#if defined(__HIPCC__)
#define RL_VARIANCE_HD __host__ __device__ inline
#else
#define RL_VARIANCE_HD inline
#endif

namespace rl {

struct alignas(16) VfGuide { float p[3]; int32_t prim; float n[3]; float pad; };   // prim -1: not a participant (S3)
struct alignas(16) VfValue { float r, g, b, var; };
static_assert(sizeof(VfGuide) == 32 && sizeof(VfValue) == 16, "the filter's packed records");

// what the host computes once for both paths, as the denoiser's DenoiseInv: sigmaLuminance as it is, 1 / sigmaNormal^2, 1 / sigmaPlane^2, historyLength
struct VfConst { float sigmaL, invN, invPl, historyLength; };
RL_VARIANCE_HD VfConst MakeVfConst(float sigmaLuminance, float sigmaNormal, float sigmaPlane, float historyLength)
{
	VfConst c;
	c.sigmaL = sigmaLuminance; c.invN = 1.0f / (sigmaNormal * sigmaNormal); c.invPl = 1.0f / (sigmaPlane * sigmaPlane); c.historyLength = historyLength;
	return c;
}

RL_VARIANCE_HD float VfFin(float v) { return (rlm::asuint(v) & 0x7f800000u) != 0x7f800000u ? v : 0.0f; }
RL_VARIANCE_HD float VfLuminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
RL_VARIANCE_HD float VfMax0(float v) { return v > 0.0f ? v : 0.0f; }   // (a NaN is 0)

// S3: the packed records of one pixel.  prim: the hit record's; P, n: the surface record's position and normal; rgb: the caller's colour.
RL_VARIANCE_HD VfGuide VfPackGuide(int32_t prim, const float P[3], const float n[3])
{
	VfGuide g;
	g.p[0] = P[0]; g.p[1] = P[1]; g.p[2] = P[2]; g.prim = prim; g.n[0] = n[0]; g.n[1] = n[1]; g.n[2] = n[2]; g.pad = 0.0f;
	return g;
}

// S4: dn + dp between the centre p and a tap q
RL_VARIANCE_HD float VfGuideDistance(const VfGuide& p, const VfGuide& q, const VfConst& c)
{
	const float e0 = q.n[0] - p.n[0], e1 = q.n[1] - p.n[1], e2 = q.n[2] - p.n[2];
	const float dn = (e0 * e0 + e1 * e1 + e2 * e2) * c.invN;
	const float d0 = q.p[0] - p.p[0], d1 = q.p[1] - p.p[1], d2 = q.p[2] - p.p[2];
	const float dd = d0 * d0 + d1 * d1 + d2 * d2;
	const float nd = p.n[0] * d0 + p.n[1] * d1 + p.n[2] * d2;
	const float dp = dd == 0.0f ? 0.0f : (nd * nd) / dd * c.invPl;
	return dn + dp;
}

// S5: the initial variance of a participating pixel (x, y).  moments: two floats per pixel, length: one (arrays of floats, 4-byte reads).
RL_VARIANCE_HD float VfInitialVariance(const VfGuide* guides, const float* moments, const float* length, int W, int H, int x, int y, const VfConst& c)
{
	const size_t p = (size_t)y * (size_t)W + (size_t)x;
	const float len = length[p];
	if (len >= c.historyLength) {
		const float m1 = moments[2 * p], m2 = moments[2 * p + 1];
		return VfMax0(m2 - m1 * m1);
	}
	const VfGuide gp = guides[p];
	float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
	for (int dy = -3; dy <= 3; ++dy) {
		const int qy = y + dy;
		if (qy < 0 || qy >= H) continue;
		for (int dx = -3; dx <= 3; ++dx) {
			const int qx = x + dx;
			if (qx < 0 || qx >= W) continue;
			const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
			const VfGuide gq = guides[q];
			if (gq.prim == -1) continue;
			const float w = rlm::expf_(-VfGuideDistance(gp, gq, c));
			sw = sw + w;
			s1 = s1 + w * moments[2 * q]; s2 = s2 + w * moments[2 * q + 1];
		}
	}
	const float M1 = s1 / sw, M2 = s2 / sw;   // (the centre's weight is expf_(-0) = 1: sw >= 1)
	return VfMax0(M2 - M1 * M1) * (c.historyLength / (len > 1.0f ? len : 1.0f));
}

// S6: one iteration at step s for a participating pixel (x, y): I(i) -> I(i+1)(p), colour and variance
RL_VARIANCE_HD VfValue VfFilterPixel(const VfValue* I, const VfGuide* guides, int W, int H, int x, int y, int s, const VfConst& c)
{
	const float k[5] = { 1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f };
	const float k3[3] = { 1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f };   // the 3 x 3 prefilter: 1/4 centre, 1/8 edges, 1/16 corners
	const size_t p = (size_t)y * (size_t)W + (size_t)x;
	const VfGuide gp = guides[p];
	const VfValue ip = I[p];
	// gv(p): var_i under the 3 x 3 kernel at step 1, over the participating taps in the frame
	float gw = 0.0f, gs = 0.0f;
	for (int dy = -1; dy <= 1; ++dy) {
		const int qy = y + dy;
		if (qy < 0 || qy >= H) continue;
		for (int dx = -1; dx <= 1; ++dx) {
			const int qx = x + dx;
			if (qx < 0 || qx >= W) continue;
			const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
			if (guides[q].prim == -1) continue;
			const float w = k3[dx + 1] * k3[dy + 1];
			gw = gw + w;
			gs = gs + w * I[q].var;
		}
	}
	const float gv = gs / gw;
	const float lambda = 1.0f / (c.sigmaL * __builtin_sqrtf(gv) + 1e-6f);
	const float yp = VfLuminance(ip.r, ip.g, ip.b);
	float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
	for (int dy = -2; dy <= 2; ++dy) {
		const int qy = y + s * dy;
		if (qy < 0 || qy >= H) continue;
		for (int dx = -2; dx <= 2; ++dx) {
			const int qx = x + s * dx;
			if (qx < 0 || qx >= W) continue;
			const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
			const VfGuide gq = guides[q];
			if (gq.prim == -1) continue;
			const VfValue iq = I[q];
			const float dl = __builtin_fabsf(VfLuminance(iq.r, iq.g, iq.b) - yp) * lambda;
			const float w = (k[dx + 2] * k[dy + 2]) * rlm::expf_(-(dl + VfGuideDistance(gp, gq, c)));
			sw = sw + w;
			sr = sr + w * iq.r; sg = sg + w * iq.g; sb = sb + w * iq.b;
			sv = sv + (w * w) * iq.var;
		}
	}
	VfValue o;
	o.r = sr / sw; o.g = sg / sw; o.b = sb / sw; o.var = sv / (sw * sw);
	return o;
}

} // namespace rl
