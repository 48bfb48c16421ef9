// The contact segment of an accepted triangle pair (include/raylib_amd.h statements C1 to C6), one statement for the host and the device: k_overlap's contacts
// instances (rl_k_overlap.inl) and the host oracle RaylibAMD_OverlapContactsHost (rl_oracle.cc) compile this file.  Everything is float, single IEEE operations
// without FMA (the Makefile's -ffp-contract=off on either side); dot and cross are rl_overlap.h's, a / b is the IEEE quotient.
// The shape of the arithmetic: each triangle's two crossing edges are cut by the other triangle's plane, once, and the segment's ends are
// chosen among those four points by comparing one coordinate -- no endpoint is interpolated twice, so every endpoint lies on the edge its feature names, with a
// weight in [0, 1], whatever the conditioning of the pair.  The three edges are unrolled with selects, not indexed arrays: the device keeps everything in
// registers.
// A record is a property of the ordered pair (Q, T) alone.
#pragma once

#include "rl_overlap.h"

namespace rl {

enum { RL_CONTACT_NONE = 0, RL_CONTACT_SEGMENT = 1, RL_CONTACT_GAP = 2, RL_CONTACT_NO_CROSSING = 3 };   // RAYLIB_AMD_CONTACT_*

// C6: p0, kind, p1, features -- 32 bytes, two 16-byte stores on the device
struct ContactRecord { float p0[3]; uint32_t kind; float p1[3]; uint32_t features; };

#define RL_CONTACT_DOT(a, b) (((a)[0] * (b)[0] + (a)[1] * (b)[1]) + (a)[2] * (b)[2])

// C2: the edge from a vertex with plane value ai to one with aj crosses the plane (a vertex on the plane counts with the non-positive side; a NaN crosses nothing)
RL_NEAREST_HD bool ContactCrosses(float ai, float aj) { return (ai <= 0.0f && 0.0f < aj) || (aj <= 0.0f && 0.0f < ai); }

// C2 and C3 for one triangle (p0, p1, p2; edges e0 = p1 - p0, e1 = p2 - p1, e2 = p0 - p2; plane values a0, a1, a2): false unless exactly two edges cross; the
// two piercing points, the lower edge index first, and those indices
RL_NEAREST_HD bool ContactPierce(const float p0[3], const float p1[3], const float p2[3], const float e0[3], const float e1[3], const float e2[3], float a0, float a1,
                                 float a2, float P0[3], float P1[3], uint32_t& f0, uint32_t& f1)
{
	const bool c0 = ContactCrosses(a0, a1), c1 = ContactCrosses(a1, a2), c2 = ContactCrosses(a2, a0);
	if ((int)c0 + (int)c1 + (int)c2 != 2) return false;
	// the lower crossing edge is 0 or 1, the higher 1 or 2
	f0 = c0 ? 0u : 1u;
	f1 = c2 ? 2u : 1u;
	const float ai0 = c0 ? a0 : a1, aj0 = c0 ? a1 : a2;
	const float ai1 = c2 ? a2 : a1, aj1 = c2 ? a0 : a2;
	const float w0 = ai0 / (ai0 - aj0), w1 = ai1 / (ai1 - aj1);
	RL_OVERLAP_UNROLL
	for (int a = 0; a < 3; ++a) {
		const float s0 = c0 ? p0[a] : p1[a], d0 = c0 ? e0[a] : e1[a];
		const float s1 = c2 ? p2[a] : p1[a], d1 = c2 ? e2[a] : e1[a];
		P0[a] = s0 + w0 * d0;
		P1[a] = s1 + w1 * d1;
	}
	return true;
}

// C1 to C6 for a pair that O1 to O4 accepted
RL_NEAREST_HD ContactRecord ContactOfPair(const float q0[3], const float q1[3], const float q2[3], const float v0[3], const float v1[3], const float v2[3])
{
	float eQ0[3], eQ1[3], eQ2[3], eT0[3], eT1[3], eT2[3], nQ[3], nT[3], r0[3], r1[3], r2[3], s0[3], s1[3], s2[3];
	RL_OVERLAP_UNROLL
	for (int a = 0; a < 3; ++a) {
		eQ0[a] = q1[a] - q0[a]; eQ1[a] = q2[a] - q1[a]; eQ2[a] = q0[a] - q2[a];
		eT0[a] = v1[a] - v0[a]; eT1[a] = v2[a] - v1[a]; eT2[a] = v0[a] - v2[a];
		r0[a] = q0[a] - v0[a]; r1[a] = q1[a] - v0[a]; r2[a] = q2[a] - v0[a];
		s0[a] = v0[a] - q0[a]; s1[a] = v1[a] - q0[a]; s2[a] = v2[a] - q0[a];
	}
	OverlapCross(eQ0, eQ1, nQ);
	OverlapCross(eT0, eT1, nT);
	// C1
	const float a0 = RL_CONTACT_DOT(nT, r0), a1 = RL_CONTACT_DOT(nT, r1), a2 = RL_CONTACT_DOT(nT, r2);
	const float b0 = RL_CONTACT_DOT(nQ, s0), b1 = RL_CONTACT_DOT(nQ, s1), b2 = RL_CONTACT_DOT(nQ, s2);
	ContactRecord R;
	R.p0[0] = R.p0[1] = R.p0[2] = 0.0f; R.p1[0] = R.p1[1] = R.p1[2] = 0.0f;
	R.kind = RL_CONTACT_NO_CROSSING; R.features = 0u;
	// C2, C3
	float PQ0[3], PQ1[3], PT0[3], PT1[3];
	uint32_t fQ0 = 0u, fQ1 = 0u, fT0 = 0u, fT1 = 0u;
	const bool okQ = ContactPierce(q0, q1, q2, eQ0, eQ1, eQ2, a0, a1, a2, PQ0, PQ1, fQ0, fQ1);
	const bool okT = ContactPierce(v0, v1, v2, eT0, eT1, eT2, b0, b1, b2, PT0, PT1, fT0, fT1);
	if (!okQ || !okT) return R;
	// C4
	float d[3];
	OverlapCross(nQ, nT, d);
	const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
	const bool m0 = ax >= ay && ax >= az, m1 = ay >= az;
#define RL_CONTACT_PARAM(P) (m0 ? (P)[0] : m1 ? (P)[1] : (P)[2])
	// C5
	const bool swQ = RL_CONTACT_PARAM(PQ1) < RL_CONTACT_PARAM(PQ0), swT = RL_CONTACT_PARAM(PT1) < RL_CONTACT_PARAM(PT0);
	float loQ[3], hiQ[3], loT[3], hiT[3];
	RL_OVERLAP_UNROLL
	for (int a = 0; a < 3; ++a) {
		loQ[a] = swQ ? PQ1[a] : PQ0[a]; hiQ[a] = swQ ? PQ0[a] : PQ1[a];
		loT[a] = swT ? PT1[a] : PT0[a]; hiT[a] = swT ? PT0[a] : PT1[a];
	}
	const uint32_t fLoQ = swQ ? fQ1 : fQ0, fHiQ = swQ ? fQ0 : fQ1, fLoT = 3u + (swT ? fT1 : fT0), fHiT = 3u + (swT ? fT0 : fT1);
	const bool startT = RL_CONTACT_PARAM(loT) > RL_CONTACT_PARAM(loQ), endT = RL_CONTACT_PARAM(hiT) < RL_CONTACT_PARAM(hiQ);
	RL_OVERLAP_UNROLL
	for (int a = 0; a < 3; ++a) { R.p0[a] = startT ? loT[a] : loQ[a]; R.p1[a] = endT ? hiT[a] : hiQ[a]; }
	R.kind = RL_CONTACT_PARAM(R.p0) <= RL_CONTACT_PARAM(R.p1) ? RL_CONTACT_SEGMENT : RL_CONTACT_GAP;
	R.features = (startT ? fLoT : fLoQ) | (endT ? fHiT : fHiQ) << 8;
#undef RL_CONTACT_PARAM
	return R;
}
#undef RL_CONTACT_DOT

} // namespace rl
