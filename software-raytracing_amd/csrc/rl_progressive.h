// The stopping rule of progressive rendering (include/raylib_amd.h RaylibAMD_BeginProgressive), one statement for the device and the host:
// k_progressive_resolve (rl_render.hip) decides with it, RaylibAMD_ProgressiveDecideHost (rl_abi.cc) is its oracle, as
// RaylibAMD_GatherAdaptiveDecideHost (rl_oracle.cc) is the adaptive gather's.  Both sides are built with -ffp-contract=off, and every operation below is one IEEE operation
// (+ - * / sqrt, correctly rounded on gfx950 and x86-64), so the two agree bit for bit.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RL_HD __host__ __device__ inline
#else
#define RL_HD inline
#endif

namespace rl {

// The standard error of a pixel's mean after n >= 2 samples, from S1 = sum of y and S2 = sum of y * y (y = L / (1 + L), L the sample's luminance):
// sqrt(max(0, (S2 - S1 * S1 / n) / (n - 1)) / n).  Sums that are not finite, and a value that is not finite (n < 2), give +inf: such a pixel never
// lets its cell stop.
RL_HD float ProgressivePixelError(float s1, float s2, uint32_t n)
{
	if (!(s1 - s1 == 0.0f) || !(s2 - s2 == 0.0f)) return __builtin_inff();   // (x - x is 0 for every finite x, NaN for inf and NaN)
	const float nf = (float)n;
	float v = (s2 - s1 * s1 / nf) / (nf - 1.0f);
	if (v < 0.0f) v = 0.0f;   // (NaN stays NaN)
	const float se = __builtin_sqrtf(v / nf);
	return se <= 3.40282347e+38f ? se : __builtin_inff();
}

// A cell stops when it has at least minSamples samples and the largest error of its valid pixels is below the threshold (threshold 0: never).
RL_HD bool ProgressiveCellStops(float cellError, uint32_t n, float threshold, uint32_t minSamples)
{
	return n >= minSamples && cellError < threshold;
}

} // namespace rl
