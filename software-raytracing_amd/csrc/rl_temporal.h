// The temporal accumulation's arithmetic (include/raylib_amd.h statement T7), one statement for the host and the device: k_temporal (rl_temporal.hip) and
// the host oracle RaylibAMD_TemporalAccumulateHost (rl_oracle.cc) compile this file.  Everything is float, single IEEE operations without FMA (the Makefile's
// -ffp-contract=off on either side); a / b is the compiler's correctly rounded division.  The two sides differ in how they read a record -- 16-byte loads on
// the device, memcpy from arrays of any alignment on the host -- which is the `Taps` argument.
//
// MOMENTS (statement S1, RaylibAMD_TemporalAccumulateMoments): the luminance moments ride on the very taps and weights the colour counted; the colour and the
// length are computed by the same statements in the same order either way (S2), and without MOMENTS nothing of it is compiled.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RL_TEMPORAL_HD __host__ __device__ inline
#else
#define RL_TEMPORAL_HD inline
#endif

namespace rl {

// what a tap reads of the history at pixel q = y * W + x: colour.rgb, hit.t, hit.prim, length
struct TemporalTap { float r, g, b, t; int32_t prim; float length; };

// S1's luminance: Y = (0.2126 r + 0.7152 g) + 0.0722 b
RL_TEMPORAL_HD float TemporalLuminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// One pixel.  colour: this frame's rgb; prim: its hit record's; (prevX, prevY, prevT, status): its motion record; taps: null-like (taps.Has() false) for the
// first frame, else taps.Read(q) gives the history at pixel q.  out: rgb and the new length.  MOMENTS: outMoments (two floats) too, and taps.Moments(q, m) gives
// the history's pair at pixel q.
template <bool MOMENTS, typename Taps>
RL_TEMPORAL_HD void TemporalPixelM(uint32_t W, uint32_t H, const float colour[3], int32_t prim, float prevX, float prevY, float prevT, uint32_t status,
                                   float depthTolerance, float maxLength, const Taps& taps, float out[3], float& outLength, float* outMoments)
{
	out[0] = colour[0]; out[1] = colour[1]; out[2] = colour[2]; outLength = 1.0f;   // the reset
	float m[2] = { 0.0f, 0.0f };
	if constexpr (MOMENTS) {
		m[0] = TemporalLuminance(colour[0], colour[1], colour[2]); m[1] = m[0] * m[0];
		outMoments[0] = m[0]; outMoments[1] = m[1];
	}
	if (status == 0u || !taps.Has()) return;
	const float fx = __builtin_floorf(prevX), fy = __builtin_floorf(prevY);
	if (!(fx >= -1.0f && fx <= 2147483648.0f && fy >= -1.0f && fy <= 2147483648.0f)) return;   // (false for NaN: no tap can lie in the frame)
	const float wx = prevX - fx, wy = prevY - fy, ox = 1.0f - wx, oy = 1.0f - wy;
	const long long ix = (long long)fx, iy = (long long)fy;
	const float wt[4] = { ox * oy, wx * oy, ox * wy, wx * wy };
	const float bound = depthTolerance * prevT;
	float Wsum = 0.0f, S[3] = { 0.0f, 0.0f, 0.0f }, L = 0.0f, M[2] = { 0.0f, 0.0f };
	for (int k = 0; k < 4; ++k) {
		const long long tx = ix + (k & 1), ty = iy + (k >> 1);
		if (tx < 0 || ty < 0 || tx >= (long long)W || ty >= (long long)H) continue;
		const float w = wt[k];
		if (!(w > 0.0f)) continue;
		const TemporalTap h = taps.Read((size_t)ty * W + (size_t)tx);
		if (!(h.length > 0.0f) || h.prim != prim) continue;
		if (status == 1u && !(__builtin_fabsf(h.t - prevT) <= bound)) continue;
		Wsum = Wsum + w;
		S[0] = S[0] + w * h.r; S[1] = S[1] + w * h.g; S[2] = S[2] + w * h.b;
		L = L + w * h.length;
		if constexpr (MOMENTS) {
			float hm[2];
			taps.Moments((size_t)ty * W + (size_t)tx, hm);
			M[0] = M[0] + w * hm[0]; M[1] = M[1] + w * hm[1];
		}
	}
	if (!(Wsum > 0.0f)) return;
	const float n = L / Wsum;
	const float n1 = n + 1.0f;
	const float np = n1 < maxLength ? n1 : maxLength;
	for (int a = 0; a < 3; ++a) {
		const float hist = S[a] / Wsum;
		out[a] = hist + (colour[a] - hist) / np;
	}
	outLength = np;
	if constexpr (MOMENTS)
		for (int a = 0; a < 2; ++a) {
			const float hist = M[a] / Wsum;
			outMoments[a] = hist + (m[a] - hist) / np;
		}
}
template <typename Taps>
RL_TEMPORAL_HD void TemporalPixel(uint32_t W, uint32_t H, const float colour[3], int32_t prim, float prevX, float prevY, float prevT, uint32_t status,
                                  float depthTolerance, float maxLength, const Taps& taps, float out[3], float& outLength)
{
	TemporalPixelM<false>(W, H, colour, prim, prevX, prevY, prevT, status, depthTolerance, maxLength, taps, out, outLength, nullptr);
}

} // namespace rl
