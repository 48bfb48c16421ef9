// The motion plane's arithmetic (include/raylib_amd.h statements T2 to T4), one statement for the host and the device: k_motion (rl_k_motion.inl) and the
// host oracle RaylibAMD_MotionHost (rl_oracle.cc) compile this file.  Everything is float, single IEEE operations without FMA (the Makefile's
// -ffp-contract=off on either side); a / b and __builtin_sqrtf are the compiler's correctly rounded division and square root;
// dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RL_MOTION_HD __host__ __device__ inline
#else
#define RL_MOTION_HD inline
#endif

namespace rl {

#define RL_MOTION_DOT(a, b) (((a)[0] * (b)[0] + (a)[1] * (b)[1]) + (a)[2] * (b)[2])

// T2: the previous point of a hit on a moved triangle -- pp holds its nine previous coordinates, (b1, b2) is the walk's pair
RL_MOTION_HD void MotionTrianglePoint(const float* pp, float b1, float b2, float P[3])
{
	for (int a = 0; a < 3; ++a) P[a] = (pp[a] + b1 * (pp[3 + a] - pp[a])) + b2 * (pp[6 + a] - pp[a]);
}
// T2: the point the ray found
RL_MOTION_HD void MotionRayPoint(const float o[3], const float d[3], float t, float P[3])
{
	for (int a = 0; a < 3; ++a) P[a] = o[a] + t * d[a];
}

// T3, T4: the record {prevX, prevY, prevT, status} of the point P (surface) or the direction P (sky: the point at infinity) through the previous camera's
// origin po, top_left pc, horizontal ph and vertical pv, in a frame of W x H pixels.  Returns the status; out holds the three floats (+0 for NONE).
RL_MOTION_HD uint32_t MotionProject(const float po[3], const float pc[3], const float ph[3], const float pv[3], float W, float H, bool surface, const float P[3], float out[3])
{
	float e[3], a[3], w[3], q[3];
	for (int k = 0; k < 3; ++k) { e[k] = surface ? P[k] - po[k] : P[k]; a[k] = pc[k] - po[k]; }
	w[0] = ph[1] * pv[2] - ph[2] * pv[1]; w[1] = ph[2] * pv[0] - ph[0] * pv[2]; w[2] = ph[0] * pv[1] - ph[1] * pv[0];
	const float lambda = RL_MOTION_DOT(a, w) / RL_MOTION_DOT(e, w);
	const float big = 3.40282347e+38f;
	if (!(lambda > 0.0f && lambda <= big)) { out[0] = out[1] = out[2] = 0.0f; return 0u; }   // (false for NaN too)
	for (int k = 0; k < 3; ++k) q[k] = lambda * e[k] - a[k];
	const float s = RL_MOTION_DOT(q, ph) / RL_MOTION_DOT(ph, ph), u = RL_MOTION_DOT(q, pv) / RL_MOTION_DOT(pv, pv);
	out[0] = s * W;
	out[1] = (1.0f - u) * H;
	out[2] = surface ? __builtin_sqrtf(RL_MOTION_DOT(e, e)) : 0.0f;
	return surface ? 1u : 2u;
}
#undef RL_MOTION_DOT

} // namespace rl
