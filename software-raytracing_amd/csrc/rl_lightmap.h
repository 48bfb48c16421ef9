// The lightmap rasteriser's arithmetic (include/raylib_amd.h, RaylibAMD_BakeLightmap, statements 1 to 5), written once for the host oracle
// (rl_lightmap_host.cc) and the kernels (rl_lightmap.hip): the integers are exact on both, the floats are single operations without FMA (the Makefile's
// -ffp-contract=off), the double division is IEEE on both, and 1.0f / x and sqrtf are rlm::rcp1_ and rlm::sqrtf_, which are those values bit for bit.
#pragma once

#include <stdint.h>
#include "rl_glibc_math.h"

namespace rl { namespace lm {

#define RL_LM_MAX_SIZE 16384
#define RL_LM_MAX_DILATE 64
// The (triangle, texel-of-its-clipped-box) pairs a call tests at most: 2^36, 256 atlases of 16384 x 16384 tested whole.  A call with more -- many triangles whose
// boxes span a large atlas, the case a hierarchical rasteriser would be for -- is refused by the device calls and the oracle alike.
#define RL_LM_MAX_PAIRS (1ull << 36)

RLM_FN bool finite_(float x) { return (rlm::asuint(x) & 0x7f800000u) != 0x7f800000u; }
RLM_FN int32_t min3_(int32_t a, int32_t b, int32_t c) { const int32_t m = a < b ? a : b; return m < c ? m : c; }
RLM_FN int32_t max3_(int32_t a, int32_t b, int32_t c) { const int32_t m = a > b ? a : b; return m > c ? m : c; }

// Statements 1 and 2: the snapped vertices and twice the signed area; false: the triangle is skipped
RLM_FN bool Snap(const float* uv, int32_t width, int32_t height, int32_t X[3], int32_t Y[3], int64_t& A2)
{
	const float fw = (float)width, fh = (float)height;
	for (int k = 0; k < 3; ++k) {
		const float fx = (uv[2 * k] * fw) * 256.0f, fy = (uv[2 * k + 1] * fh) * 256.0f;
		if (!finite_(fx) || !finite_(fy) || rlm::fabsf_(fx) > 16777216.0f || rlm::fabsf_(fy) > 16777216.0f) return false;
		X[k] = (int32_t)__builtin_floorf(fx + 0.5f); Y[k] = (int32_t)__builtin_floorf(fy + 0.5f);
	}
	A2 = (int64_t)(X[1] - X[0]) * (int64_t)(Y[2] - Y[0]) - (int64_t)(Y[1] - Y[0]) * (int64_t)(X[2] - X[0]);
	return A2 != 0;
}
// The texels whose centres (256 x + 128, 256 y + 128) lie in the triangle's bounding box and in the atlas: columns xlo .. xlo + rw - 1, rows ylo .. ylo + rh - 1;
// returns rw * rh (0: none).  (v + 127) >> 8 is ceil((v - 128) / 256), (v - 128) >> 8 its floor: the shifts are arithmetic.
RLM_FN uint32_t Rect(const int32_t X[3], const int32_t Y[3], int32_t width, int32_t height, int32_t& xlo, int32_t& ylo, int32_t& rw)
{
	int32_t x0 = (min3_(X[0], X[1], X[2]) + 127) >> 8, x1 = (max3_(X[0], X[1], X[2]) - 128) >> 8;
	int32_t y0 = (min3_(Y[0], Y[1], Y[2]) + 127) >> 8, y1 = (max3_(Y[0], Y[1], Y[2]) - 128) >> 8;
	if (x0 < 0) x0 = 0;
	if (y0 < 0) y0 = 0;
	if (x1 > width - 1) x1 = width - 1;
	if (y1 > height - 1) y1 = height - 1;
	xlo = x0; ylo = y0; rw = 0;
	if (x1 < x0 || y1 < y0) return 0u;
	rw = x1 - x0 + 1;
	return (uint32_t)rw * (uint32_t)(y1 - y0 + 1);
}
RLM_FN int64_t Orient(int32_t qx, int32_t qy, int32_t rx, int32_t ry, int32_t px, int32_t py)
{
	return (int64_t)(rx - qx) * (int64_t)(py - qy) - (int64_t)(ry - qy) * (int64_t)(px - qx);
}
// Statement 3: does the triangle cover texel (x, y); wB and wC are the weights of its second and third vertex
RLM_FN bool Cover(const int32_t X[3], const int32_t Y[3], int64_t A2, int32_t x, int32_t y, int64_t& wB, int64_t& wC)
{
	const int32_t px = 256 * x + 128, py = 256 * y + 128;
	const int64_t s = A2 > 0 ? 1 : -1;
	const int64_t wA = s * Orient(X[1], Y[1], X[2], Y[2], px, py);
	wB = s * Orient(X[2], Y[2], X[0], Y[0], px, py);
	wC = s * Orient(X[0], Y[0], X[1], Y[1], px, py);
	return wA >= 0 && wB >= 0 && wC >= 0;
}
RLM_FN float Dot(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// Statements 4 and 5 from the owner's record (t: v0, v1, v2, n0, n1, n2, 18 floats); false: the texel is empty
RLM_FN bool Point(const float* t, int64_t wB, int64_t wC, int64_t A2, float pos[3], float normal[3])
{
	const double area = (double)(A2 < 0 ? -A2 : A2);
	const float b1 = (float)((double)wB / area), b2 = (float)((double)wC / area);
	float e1[3], e2[3], n[3];
	for (int i = 0; i < 3; ++i) {
		e1[i] = t[3 + i] - t[i]; e2[i] = t[6 + i] - t[i];
		pos[i] = (t[i] + b1 * e1[i]) + b2 * e2[i];
		n[i] = (t[9 + i] + b1 * (t[12 + i] - t[9 + i])) + b2 * (t[15 + i] - t[9 + i]);
	}
	float d = Dot(n, n);
	if (!(finite_(d) && d > 0.0f)) {
		n[0] = e1[1] * e2[2] - e1[2] * e2[1]; n[1] = e1[2] * e2[0] - e1[0] * e2[2]; n[2] = e1[0] * e2[1] - e1[1] * e2[0];
		d = Dot(n, n);
	}
	if (!(finite_(d) && d > 0.0f) || !finite_(pos[0]) || !finite_(pos[1]) || !finite_(pos[2])) return false;
	const float k = rlm::rcp1_(rlm::sqrtf_(d));
	normal[0] = n[0] * k; normal[1] = n[1] * k; normal[2] = n[2] * k;
	return true;
}

} } // namespace rl::lm
