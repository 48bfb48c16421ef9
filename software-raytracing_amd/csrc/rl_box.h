// The oriented-box range query's arithmetic (include/raylib_amd.h statements B1 to B4), one statement for the host and the device: k_overlap_box
// (rl_k_overlap_box.inl) and the host oracle RaylibAMD_OverlapBoxesHost (rl_oracle.cc) compile this file.  Everything is float, single IEEE operations without
// FMA (the Makefile's -ffp-contract=off on either side); dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; least and greatest are rl_overlap.h's, in its order.
// Why a tree walk can equal the loop over every triangle with no slack anywhere: B2 makes the box that encloses the query -- centre -/+ the sum of the axes'
// absolute components times their half extents -- part of the verdict: a triangle whose own box does not meet it under O2's closed comparison is not accepted,
// whatever B4 would say.  That test is pure comparisons on values computed once per query, so rl_overlap.h's argument holds word for word with B2's box in the
// place of the query triangle's: a node whose box does not meet it holds no triangle whose own box does.  In exact arithmetic, with orthonormal axes, B2's box
// contains the oriented box and removes nothing B4 accepts; at rounding level it may (the trade of the sweep's W5: the cull is exact because the verdict says so).
// The axes are used as given: neither normalised nor checked for orthogonality.  With identity axes every frame coordinate of B3 is exactly v - centre (the
// products with 1 and 0 and the sums with +0 are exact for finite values), so an axis-aligned box touches exactly where the comparison says.
#pragma once

#include "rl_overlap.h"   // RL_NEAREST_HD, OverlapFinite3, OverlapMin3 / OverlapMax3, OverlapOwnBox, OverlapBoxesMeet, OverlapCross

namespace rl {

// a query as the walk holds it: the record's 15 floats (axis k's direction in a[k], its half extent in h[k]) and, once BoxEnclosing has run, B2's box
struct BoxQ { float c[3]; float a[3][3]; float h[3]; float lo[3], hi[3]; };

#define RL_BOX_DOT(a, b) (((a)[0] * (b)[0] + (a)[1] * (b)[1]) + (a)[2] * (b)[2])
#define RL_BOX_ABS(x) __builtin_fabsf(x)

// B1: a query takes part when all 15 of its floats are finite and every half extent is >= 0 (-0.0 is 0)
RL_NEAREST_HD bool BoxTakesPart(const BoxQ& Q)
{
	return OverlapFinite3(Q.c) && OverlapFinite3(Q.a[0]) && OverlapFinite3(Q.a[1]) && OverlapFinite3(Q.a[2]) && OverlapFinite3(Q.h) && Q.h[0] >= 0.0f && Q.h[1] >= 0.0f &&
	       Q.h[2] >= 0.0f;
}

// B2: the enclosing box (an overflow gives +inf, never a NaN: every factor is finite, and 0 * finite is 0)
RL_NEAREST_HD void BoxEnclosing(BoxQ& Q)
{
	for (int k = 0; k < 3; ++k) {
		const float e = (RL_BOX_ABS(Q.a[0][k]) * Q.h[0] + RL_BOX_ABS(Q.a[1][k]) * Q.h[1]) + RL_BOX_ABS(Q.a[2][k]) * Q.h[2];
		Q.lo[k] = Q.c[k] - e; Q.hi[k] = Q.c[k] + e;
	}
}

// B3: a vertex in the box's frame
RL_NEAREST_HD void BoxFrame(const BoxQ& Q, const float v[3], float p[3])
{
	const float d[3] = { v[0] - Q.c[0], v[1] - Q.c[1], v[2] - Q.c[2] };
	p[0] = RL_BOX_DOT(Q.a[0], d); p[1] = RL_BOX_DOT(Q.a[1], d); p[2] = RL_BOX_DOT(Q.a[2], d);
}

// B4: no one of the 13 axes separates -- the three faces, the triangle's plane, the nine edge axes with the box axis outer.  (The first axis that separates
// ends the test: the verdict asks for none.  A NaN compares false and separates nothing.)
RL_NEAREST_HD bool BoxNoAxisSeparates(const BoxQ& Q, const float v0[3], const float v1[3], const float v2[3])
{
	float p0[3], p1[3], p2[3];
	BoxFrame(Q, v0, p0); BoxFrame(Q, v1, p1); BoxFrame(Q, v2, p2);
	const float* h = Q.h;
	RL_OVERLAP_UNROLL
	for (int i = 0; i < 3; ++i) {
		const float least = OverlapMin3(p0[i], p1[i], p2[i]), greatest = OverlapMax3(p0[i], p1[i], p2[i]);
		if (least > h[i] || greatest < -h[i]) return false;
	}
	float e[3][3], n[3];
	for (int k = 0; k < 3; ++k) { e[0][k] = p1[k] - p0[k]; e[1][k] = p2[k] - p1[k]; e[2][k] = p0[k] - p2[k]; }
	OverlapCross(e[0], e[1], n);
	{
		const float r = (h[0] * RL_BOX_ABS(n[0]) + h[1] * RL_BOX_ABS(n[1])) + h[2] * RL_BOX_ABS(n[2]);
		const float s = RL_BOX_DOT(n, p0);
		if (s > r || s < -r) return false;
	}
	RL_OVERLAP_UNROLL
	for (int i = 0; i < 3; ++i) {
		const int u = (i + 1) % 3, w = (i + 2) % 3;
		RL_OVERLAP_UNROLL
		for (int j = 0; j < 3; ++j) {
			const float eu = e[j][u], ew = e[j][w];
			const float s0 = p0[w] * eu - p0[u] * ew, s1 = p1[w] * eu - p1[u] * ew, s2 = p2[w] * eu - p2[u] * ew;
			const float r = h[u] * RL_BOX_ABS(ew) + h[w] * RL_BOX_ABS(eu);
			const float least = OverlapMin3(s0, s1, s2), greatest = OverlapMax3(s0, s1, s2);
			if (least > r || greatest < -r) return false;
		}
	}
	return true;
}

// B2 to B4 for a query that takes part (BoxEnclosing done) and one scene triangle
RL_NEAREST_HD bool BoxAccepts(const BoxQ& Q, const float v0[3], const float v1[3], const float v2[3])
{
	float lo[3], hi[3];
	OverlapOwnBox(v0, v1, v2, lo, hi);
	if (!OverlapBoxesMeet(Q.lo, Q.hi, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2])) return false;
	return BoxNoAxisSeparates(Q, v0, v1, v2);
}

#undef RL_BOX_ABS
#undef RL_BOX_DOT

} // namespace rl
