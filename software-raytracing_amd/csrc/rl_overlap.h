// The triangle-overlap query's arithmetic (include/raylib_amd.h statements O1 to O4), one statement for the host and the device: k_overlap (rl_k_overlap.inl)
// and the host oracle RaylibAMD_OverlapTrianglesHost (rl_oracle.cc) compile this file.  Everything is float, single IEEE operations without FMA (the Makefile's
// -ffp-contract=off on either side); dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; least and greatest are found by comparisons, in the order written here.
// Why a tree walk can equal the loop over every triangle with no slack anywhere: O2, the test of the query's own box against a triangle's own box, is pure
// comparisons -- nothing rounds.  A triangle's own box lies in its leaf's box, a binary node's boxes are the min / max of its children's, and a grid box,
// decoded as origin + (float)q * step, contains the float box it was quantised from (rl_grid.h).  "Meets" under the closed comparison is monotone under
// containment: a box that meets Q's box makes every box around it meet Q's box.  So a node whose box does not meet Q's box under the same comparison holds
// no triangle whose own box does, and O2 rejects each of them before O3 and O4 are asked: the walk drops only what the loop rejects.
// The verdict of O4 is a property of the ordered pair (Q, T) alone; every projection is taken relative to Q's first vertex, so it is not promised to be the
// verdict of (T, Q) at rounding level.
#pragma once

#include "rl_nearest.h"   // RL_NEAREST_HD

// (the device build unrolls the axis loops, so that the edge arrays stay in registers)
#if defined(__HIPCC__)
#define RL_OVERLAP_UNROLL _Pragma("unroll")
#else
#define RL_OVERLAP_UNROLL
#endif

namespace rl {

// O1: a query takes part when all nine of its floats are finite
RL_NEAREST_HD bool OverlapFinite3(const float v[3])
{
	const float big = 3.40282347e+38f;
	return v[0] >= -big && v[0] <= big && v[1] >= -big && v[1] <= big && v[2] >= -big && v[2] <= big;
}
RL_NEAREST_HD bool OverlapTakesPart(const float q0[3], const float q1[3], const float q2[3]) { return OverlapFinite3(q0) && OverlapFinite3(q1) && OverlapFinite3(q2); }

// least and greatest of three by comparisons, in this order (a NaN in front is replaced by nothing, a NaN behind replaces nothing)
RL_NEAREST_HD float OverlapMin3(float a, float b, float c) { float m = b < a ? b : a; m = c < m ? c : m; return m; }
RL_NEAREST_HD float OverlapMax3(float a, float b, float c) { float m = a < b ? b : a; m = m < c ? c : m; return m; }

// O2: a triangle's own box, and whether two boxes meet (closed on every axis)
RL_NEAREST_HD void OverlapOwnBox(const float v0[3], const float v1[3], const float v2[3], float lo[3], float hi[3])
{
	for (int a = 0; a < 3; ++a) { lo[a] = OverlapMin3(v0[a], v1[a], v2[a]); hi[a] = OverlapMax3(v0[a], v1[a], v2[a]); }
}
RL_NEAREST_HD bool OverlapBoxesMeet(const float loQ[3], const float hiQ[3], float lox, float loy, float loz, float hix, float hiy, float hiz)
{
	return loQ[0] <= hix && lox <= hiQ[0] && loQ[1] <= hiy && loy <= hiQ[1] && loQ[2] <= hiz && loz <= hiQ[2];
}

// O3: one of T's vertices equals one of Q's (componentwise ==, so -0 == +0 and a NaN equals nothing)
RL_NEAREST_HD bool OverlapSameVertex(const float a[3], const float b[3]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }
RL_NEAREST_HD bool OverlapSharesVertex(const float q0[3], const float q1[3], const float q2[3], const float v0[3], const float v1[3], const float v2[3])
{
	return OverlapSameVertex(q0, v0) || OverlapSameVertex(q0, v1) || OverlapSameVertex(q0, v2) || OverlapSameVertex(q1, v0) || OverlapSameVertex(q1, v1) ||
	       OverlapSameVertex(q1, v2) || OverlapSameVertex(q2, v0) || OverlapSameVertex(q2, v1) || OverlapSameVertex(q2, v2);
}

#define RL_OVERLAP_DOT(a, b) (((a)[0] * (b)[0] + (a)[1] * (b)[1]) + (a)[2] * (b)[2])
RL_NEAREST_HD void OverlapCross(const float a[3], const float b[3], float c[3])
{
	c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// O4, one axis: Q projects to {+0, dot(a, q1 - q0), dot(a, q2 - q0)}, T to dot(a, v_k - q0); the axis separates when one interval ends before the other begins
// (a NaN compares false and separates nothing)
RL_NEAREST_HD bool OverlapAxisSeparates(const float a[3], const float d1[3], const float d2[3], const float t0[3], const float t1[3], const float t2[3])
{
	const float p1 = RL_OVERLAP_DOT(a, d1), p2 = RL_OVERLAP_DOT(a, d2);
	const float s0 = RL_OVERLAP_DOT(a, t0), s1 = RL_OVERLAP_DOT(a, t1), s2 = RL_OVERLAP_DOT(a, t2);
	const float minQ = OverlapMin3(0.0f, p1, p2), maxQ = OverlapMax3(0.0f, p1, p2);
	const float minT = OverlapMin3(s0, s1, s2), maxT = OverlapMax3(s0, s1, s2);
	return maxQ < minT || maxT < minQ;
}
#undef RL_OVERLAP_DOT
// O4: no one of the 17 axes separates -- nQ, nT, cross(eQi, eTj) with i outer, cross(nQ, eQi), cross(nT, eTj).  (The first axis that separates ends the test:
// the verdict asks for none.)
RL_NEAREST_HD bool OverlapNoAxisSeparates(const float q0[3], const float q1[3], const float q2[3], const float v0[3], const float v1[3], const float v2[3])
{
	float eQ[3][3], eT[3][3], d2[3], t0[3], t1[3], t2[3], nQ[3], nT[3], ax[3];
	for (int a = 0; a < 3; ++a) {
		eQ[0][a] = q1[a] - q0[a]; eQ[1][a] = q2[a] - q1[a]; eQ[2][a] = q0[a] - q2[a];
		eT[0][a] = v1[a] - v0[a]; eT[1][a] = v2[a] - v1[a]; eT[2][a] = v0[a] - v2[a];
		d2[a] = q2[a] - q0[a];
		t0[a] = v0[a] - q0[a]; t1[a] = v1[a] - q0[a]; t2[a] = v2[a] - q0[a];
	}
	const float* d1 = eQ[0];   // q1 - q0
	OverlapCross(eQ[0], eQ[1], nQ);
	if (OverlapAxisSeparates(nQ, d1, d2, t0, t1, t2)) return false;
	OverlapCross(eT[0], eT[1], nT);
	if (OverlapAxisSeparates(nT, d1, d2, t0, t1, t2)) return false;
	RL_OVERLAP_UNROLL
	for (int i = 0; i < 3; ++i)
		RL_OVERLAP_UNROLL
		for (int j = 0; j < 3; ++j) {
			OverlapCross(eQ[i], eT[j], ax);
			if (OverlapAxisSeparates(ax, d1, d2, t0, t1, t2)) return false;
		}
	RL_OVERLAP_UNROLL
	for (int i = 0; i < 3; ++i) {
		OverlapCross(nQ, eQ[i], ax);
		if (OverlapAxisSeparates(ax, d1, d2, t0, t1, t2)) return false;
	}
	RL_OVERLAP_UNROLL
	for (int j = 0; j < 3; ++j) {
		OverlapCross(nT, eT[j], ax);
		if (OverlapAxisSeparates(ax, d1, d2, t0, t1, t2)) return false;
	}
	return true;
}

// O2 to O4 for a query that takes part (loQ, hiQ: its own box) and one scene triangle
RL_NEAREST_HD bool OverlapAccepts(const float q0[3], const float q1[3], const float q2[3], const float loQ[3], const float hiQ[3], const float v0[3], const float v1[3],
                                  const float v2[3], bool skipShared)
{
	float lo[3], hi[3];
	OverlapOwnBox(v0, v1, v2, lo, hi);
	if (!OverlapBoxesMeet(loQ, hiQ, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2])) return false;
	if (skipShared && OverlapSharesVertex(q0, q1, q2, v0, v1, v2)) return false;
	return OverlapNoAxisSeparates(q0, q1, q2, v0, v1, v2);
}

} // namespace rl
