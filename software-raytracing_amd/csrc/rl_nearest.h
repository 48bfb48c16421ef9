// The nearest-point query's arithmetic (include/raylib_amd.h statements N1 to N3), one statement for the host and the device: k_nearest (rl_k_nearest.inl)
// and the host oracle RaylibAMD_NearestPointsHost (rl_oracle.cc) compile this file.  Everything is float, single IEEE operations without FMA (the Makefile's
// -ffp-contract=off on either side); a / b and 1.0f / x are the compiler's correctly rounded divisions; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
// Why the result cannot depend on the tree walked: NearestBoxDist2 rounds monotonically at every operation, so a box that contains another is never farther
// than it; a triangle's distance is at least its own box's (N3), the own box lies in its leaf's box, a binary node's boxes are the min / max of its children's,
// and a grid box, decoded as origin + (float)q * step (one rounding, monotone), contains the float box it was quantised from (rl_grid.h).  A node whose
// box distance exceeds the best distance found so far therefore holds no winner -- with no widening factor anywhere.
#pragma once

#if defined(__HIPCC__)
#define RL_NEAREST_HD __host__ __device__ inline
#else
#define RL_NEAREST_HD inline
#endif

namespace rl {

// N2 on any box: per axis the gap between the point and the box (0 inside), squared and summed
RL_NEAREST_HD float NearestAxisGap(float p, float lo, float hi)
{
	const float t = lo - p, u = p - hi;
	return t > 0.0f ? t : (u > 0.0f ? u : 0.0f);
}
RL_NEAREST_HD float NearestBoxDist2(float px, float py, float pz, float lox, float loy, float loz, float hix, float hiy, float hiz)
{
	const float dx = NearestAxisGap(px, lox, hix), dy = NearestAxisGap(py, loy, hiy), dz = NearestAxisGap(pz, loz, hiz);
	return (dx * dx + dy * dy) + dz * dz;
}
// N2 on a triangle's own box: the componentwise least and greatest of its vertices, by comparisons
RL_NEAREST_HD float NearestOwnBoxDist2(const float p[3], const float v0[3], const float v1[3], const float v2[3])
{
	float d[3];
	for (int a = 0; a < 3; ++a) {
		float lo = v1[a] < v0[a] ? v1[a] : v0[a]; lo = v2[a] < lo ? v2[a] : lo;
		float hi = v0[a] < v1[a] ? v1[a] : v0[a]; hi = hi < v2[a] ? v2[a] : hi;
		d[a] = NearestAxisGap(p[a], lo, hi);
	}
	return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
}

#define RL_NEAREST_DOT(a, b) (((a)[0] * (b)[0] + (a)[1] * (b)[1]) + (a)[2] * (b)[2])
// N1: the closest point of the triangle in Ericson's regions (the first condition that holds decides), its barycentric pair and the squared distance E to it
RL_NEAREST_HD float NearestTriangleE(const float p[3], const float v0[3], const float v1[3], const float v2[3], float& b1, float& b2)
{
	float ab[3], ac[3], ap[3], bp[3], cp[3];
	for (int a = 0; a < 3; ++a) { ab[a] = v1[a] - v0[a]; ac[a] = v2[a] - v0[a]; ap[a] = p[a] - v0[a]; bp[a] = p[a] - v1[a]; cp[a] = p[a] - v2[a]; }
	const float d1 = RL_NEAREST_DOT(ab, ap), d2 = RL_NEAREST_DOT(ac, ap);
	const float d3 = RL_NEAREST_DOT(ab, bp), d4 = RL_NEAREST_DOT(ac, bp);
	const float d5 = RL_NEAREST_DOT(ab, cp), d6 = RL_NEAREST_DOT(ac, cp);
	const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
	const float e = d4 - d3, g = d5 - d6;
	if (d1 <= 0.0f && d2 <= 0.0f) { b1 = 0.0f; b2 = 0.0f; }
	else if (d3 >= 0.0f && d4 <= d3) { b1 = 1.0f; b2 = 0.0f; }
	else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { b1 = d1 / (d1 - d3); b2 = 0.0f; }
	else if (d6 >= 0.0f && d5 <= d6) { b1 = 0.0f; b2 = 1.0f; }
	else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { b1 = 0.0f; b2 = d2 / (d2 - d6); }
	else if (va <= 0.0f && e >= 0.0f && g >= 0.0f) { const float w = e / (e + g); b1 = 1.0f - w; b2 = w; }
	else { const float den = 1.0f / ((va + vb) + vc); b1 = vb * den; b2 = vc * den; }
	float r[3];
	for (int a = 0; a < 3; ++a) { const float q = (v0[a] + b1 * ab[a]) + b2 * ac[a]; r[a] = p[a] - q; }
	return RL_NEAREST_DOT(r, r);
}
#undef RL_NEAREST_DOT
// N3: the triangle's distance D = E >= B ? E : B (a NaN E, from a degenerate triangle, yields B)
RL_NEAREST_HD float NearestTriangleD(float E, float B) { return E >= B ? E : B; }

// N4: a point takes part when its position is finite and maxDist >= 0 (+inf allowed; NaN and negative values not; -0.0 is 0)
RL_NEAREST_HD bool NearestTakesPart(float px, float py, float pz, float maxDist)
{
	const float big = 3.40282347e+38f;
	return px >= -big && px <= big && py >= -big && py <= big && pz >= -big && pz <= big && maxDist >= 0.0f;
}

} // namespace rl
