// The swept-sphere query's arithmetic (include/raylib_amd.h RaylibAMD_SweepSpheres, statements W1 to W7), one statement for the host and the device: k_sweep
// (rl_k_sweep.inl) and the host oracle RaylibAMD_SweepSpheresHost (rl_oracle.cc) compile this file.  Everything is float, single IEEE operations without FMA (the
// Makefile's -ffp-contract=off on either side); a / b and 1.0f / x are the compiler's correctly rounded divisions, __builtin_sqrtf the correctly rounded root;
// dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, cross(a, b).x = a.y b.z - a.z b.y (and cyclic).
//
// A sphere of radius r moves from o to o + d; c(t) = o + t d, t in [0, 1], is its centre.
//   W1. Who takes part.  Every component of o and d and r are finite and r >= 0 (-0.0 is 0); a query that does not take part misses.  inv = 1.0f / d per
//       component, taken once per query; a component whose inv is not finite (0, -0.0, a denormal below 2^-128) is read as 0 everywhere below.
//   W2. The time bound of a box, Bt(lo, hi): the entry time of the centre's path into the box grown by r, by slabs.  Per axis l = lo - r, h = hi + r.  An axis
//       with d != 0 gives tl = (l - o) * inv, th = (h - o) * inv, near = d > 0 ? tl : th, far = d > 0 ? th : tl; an axis with d == 0 passes when
//       l <= o && o <= h.  entry = the greatest of 0 and the nears, exit = the least of +inf and the fars (comparisons, x and y before z);
//       Bt = every d == 0 axis passes && entry <= exit ? entry : +inf.  No operand is NaN: l, h, o and inv are not, and a product has a finite inv.
//       Why the result cannot depend on the tree walked: each operation rounds monotonically, so for a box that contains another every l is no larger and every
//       h no smaller, hence every near no larger and every far no smaller: entry(outer) <= entry(inner) <= exit(inner) <= exit(outer), a d == 0 axis that
//       passes for the inner box passes for the outer one, and so Bt(outer) <= Bt(inner) -- an outer miss (+inf) implies an inner miss.  A triangle's time is at
//       least its own box's (W5), the own box lies in its leaf's box, a binary node's boxes are the min / max of its children's, and a grid box decoded as
//       origin + (float)q * step contains the float box it was quantised from (rl_grid.h).  A node whose Bt exceeds the best time found so far therefore holds no
//       winner -- with no widening factor anywhere.
//   W3. Touching at the start.  N1 to N3 of the nearest-point family (rl_nearest.h) at p = o give D; when D <= r * r the triangle's t is 0, its feature 7 and
//       its point N1's q = (v0 + b1 * ab) + b2 * ac.
//   W4. The first impact otherwise: the least t in [0, 1] over seven features, evaluated in the order of their numbers; a later feature replaces an earlier
//       one only with a smaller t.  The root of |M + t V| = r, Root(M, V): a = dot(V, V), b = dot(M, V), f = b / a, H = M - f * V (the closest approach),
//       disc = a * (r * r - dot(H, H)); when a > 0 && disc >= 0, t = ((0 - b) - sqrt(disc)) / a, accepted when 0 <= t && t <= 1.  (disc is the textbook's
//       b * b - a * c with the difference taken where it does not cancel: written as b * b - a * c it loses (|M| / r)^2 units of the last place.)
//         0, the face.  ab = v1 - v0, ac = v2 - v0, n = cross(ab, ac), len = sqrt(dot(n, n)), s = dot(n, o - v0), nd = dot(n, d), rl = r * len,
//            closing = s > 0 ? 0 - nd : nd.  A candidate when |s| > rl && closing > 0: t = (|s| - rl) / closing, accepted when t <= 1.  The point is
//            P = c(t) -/+ (r * n) / len (- for s > 0), c(t) = o + t * d, accepted when dot(cross(ab, P - v0), n) >= 0, dot(cross(v2 - v1, P - v1), n) >= 0 and
//            dot(cross(v0 - v2, P - v2), n) >= 0.
//         1..3, the edges v0v1, v1v2, v2v0, A to B: e = B - A, m = o - A, ie = 1 / dot(e, e), fd = dot(d, e) * ie, fm = dot(m, e) * ie; the root of the
//            parts across the edge, Root(m - fm * e, d - fd * e) -- the infinite cylinder of radius r about the edge --, accepted when the axial parameter
//            u = fm + t * fd lies in [0, 1].  The point is A + u * e.
//         4..6, the vertices v0, v1, v2: Root(o - V, d).  The point is V.
//       A NaN anywhere (a degenerate triangle: len == 0, dot(e, e) == 0) fails its comparison and drops that feature only.  d == 0 gives every feature a == 0 or
//       closing == 0: W3 alone decides.
//   W5. N3's rule for time.  T = t >= Bt(own box) ? t : Bt(own box), the own box being the componentwise least and greatest of the vertices, by comparisons
//       (N2).  The triangle is a candidate when T <= 1.  In exact arithmetic the centre at a touching time is within r of the triangle, hence inside its grown
//       box, and t >= Bt always: the rule moves T at rounding level only, and it holds for W3's t = 0 as for W4's.  It buys W2's conclusion.
//   W6. CLOSEST is the candidate with the least (T, k), k the export index; it writes {T, k, feature, point}.  ANY is 1 exactly when a candidate exists.
//   W7. The result is a property of the query and the triangles alone: it does not depend on the tree, the order of the walk, the cut into waves, or whether the
//       trees are fresh or refitted.
// r == 0 is accepted: the query is then a segment test whose edge and vertex features are degenerate (disc >= 0 only on exact contact); it carries no
// watertightness promise, and RaylibAMD_TraceRays is the entry for rays.
#pragma once

#include "rl_nearest.h"

#if defined(__HIPCC__)
#define RL_SWEEP_HD __host__ __device__ inline
#else
#define RL_SWEEP_HD inline
#endif

namespace rl {

#define RL_SWEEP_DOT(a, b) (((a)[0] * (b)[0] + (a)[1] * (b)[1]) + (a)[2] * (b)[2])
#define RL_SWEEP_CROSS(out, a, b) { (out)[0] = (a)[1] * (b)[2] - (a)[2] * (b)[1]; (out)[1] = (a)[2] * (b)[0] - (a)[0] * (b)[2]; (out)[2] = (a)[0] * (b)[1] - (a)[1] * (b)[0]; }

// W1: the move as the statements read it -- o, d (a component without a finite reciprocal is 0), inv (0 where d is 0: not read) and r
struct SweepMove { float o[3], d[3], inv[3], r; };
RL_SWEEP_HD bool SweepTakesPart(const float o[3], const float delta[3], float r, SweepMove& M)
{
	const float big = 3.40282347e+38f;
	bool ok = r >= 0.0f && r <= big;
	for (int a = 0; a < 3; ++a) {
		ok = ok && o[a] >= -big && o[a] <= big && delta[a] >= -big && delta[a] <= big;
		const float inv = 1.0f / delta[a];
		const bool finite = inv >= -big && inv <= big;
		M.o[a] = o[a]; M.d[a] = finite ? delta[a] : 0.0f; M.inv[a] = finite ? inv : 0.0f;
	}
	M.r = r;
	return ok;
}

// W2 on any box
RL_SWEEP_HD float SweepBoxTime(const SweepMove& M, const float lo[3], const float hi[3])
{
	float entry = 0.0f, exit = __builtin_huge_valf();
	bool pass = true;
	for (int a = 0; a < 3; ++a) {
		const float l = lo[a] - M.r, h = hi[a] + M.r;
		if (M.d[a] != 0.0f) {
			const float tl = (l - M.o[a]) * M.inv[a], th = (h - M.o[a]) * M.inv[a];
			const float near = M.d[a] > 0.0f ? tl : th, far = M.d[a] > 0.0f ? th : tl;
			entry = near > entry ? near : entry;
			exit = far < exit ? far : exit;
		} else if (!(l <= M.o[a] && M.o[a] <= h)) pass = false;
	}
	return pass && entry <= exit ? entry : __builtin_huge_valf();
}
// W2 on a triangle's own box (N2's box: the componentwise least and greatest of its vertices, by comparisons)
RL_SWEEP_HD float SweepOwnBoxTime(const SweepMove& M, const float v0[3], const float v1[3], const float v2[3])
{
	float lo[3], hi[3];
	for (int a = 0; a < 3; ++a) {
		lo[a] = v1[a] < v0[a] ? v1[a] : v0[a]; lo[a] = v2[a] < lo[a] ? v2[a] : lo[a];
		hi[a] = v0[a] < v1[a] ? v1[a] : v0[a]; hi[a] = hi[a] < v2[a] ? v2[a] : hi[a];
	}
	return SweepBoxTime(M, lo, hi);
}

// W4's root: the first t in [0, 1] at which |m + t v| = r
RL_SWEEP_HD bool SweepRoot(const float m[3], const float v[3], float r, float& t)
{
	const float a = RL_SWEEP_DOT(v, v), b = RL_SWEEP_DOT(m, v);
	const float f = b / a;
	float h[3];
	for (int k = 0; k < 3; ++k) h[k] = m[k] - f * v[k];
	const float disc = a * (r * r - RL_SWEEP_DOT(h, h));
	if (!(a > 0.0f && disc >= 0.0f)) return false;
	t = ((0.0f - b) - __builtin_sqrtf(disc)) / a;
	return t >= 0.0f && t <= 1.0f;
}

// W3 and W4: whether the sphere touches the triangle within the move, and then the time t, the feature and the touched point
RL_SWEEP_HD bool SweepTriangle(const SweepMove& M, const float v0[3], const float v1[3], const float v2[3], float& t, int& feature, float point[3])
{
	const float* const V[3] = { v0, v1, v2 };
	float ab[3], ac[3];
	for (int k = 0; k < 3; ++k) { ab[k] = v1[k] - v0[k]; ac[k] = v2[k] - v0[k]; }
	// W3
	{
		float b1, b2;
		const float E = NearestTriangleE(M.o, v0, v1, v2, b1, b2);
		const float D = NearestTriangleD(E, NearestOwnBoxDist2(M.o, v0, v1, v2));
		if (D <= M.r * M.r) {
			t = 0.0f; feature = 7;
			for (int k = 0; k < 3; ++k) point[k] = (v0[k] + b1 * ab[k]) + b2 * ac[k];
			return true;
		}
	}
	// W4
	t = __builtin_huge_valf(); feature = -1;
	{	// the face
		float n[3], w[3];
		RL_SWEEP_CROSS(n, ab, ac)
		for (int k = 0; k < 3; ++k) w[k] = M.o[k] - v0[k];
		const float len = __builtin_sqrtf(RL_SWEEP_DOT(n, n)), s = RL_SWEEP_DOT(n, w), nd = RL_SWEEP_DOT(n, M.d), rl = M.r * len;
		const float as = __builtin_fabsf(s), closing = s > 0.0f ? 0.0f - nd : nd;
		if (as > rl && closing > 0.0f) {
			const float tf = (as - rl) / closing;
			if (tf <= 1.0f) {
				float P[3];
				for (int k = 0; k < 3; ++k) {
					const float c = M.o[k] + tf * M.d[k], off = (M.r * n[k]) / len;
					P[k] = s > 0.0f ? c - off : c + off;
				}
				bool inside = true;
				for (int j = 0; j < 3; ++j) {
					const float *A = V[j], *B = V[(j + 1) % 3];
					float e[3], q[3], x[3];
					for (int k = 0; k < 3; ++k) { e[k] = B[k] - A[k]; q[k] = P[k] - A[k]; }
					RL_SWEEP_CROSS(x, e, q)
					if (!(RL_SWEEP_DOT(x, n) >= 0.0f)) inside = false;
				}
				if (inside) { t = tf; feature = 0; for (int k = 0; k < 3; ++k) point[k] = P[k]; }
			}
		}
	}
	for (int j = 0; j < 3; ++j) {   // the edges
		const float *A = V[j], *B = V[(j + 1) % 3];
		float e[3], m[3], mp[3], dp[3];
		for (int k = 0; k < 3; ++k) { e[k] = B[k] - A[k]; m[k] = M.o[k] - A[k]; }
		const float ie = 1.0f / RL_SWEEP_DOT(e, e);
		const float fd = RL_SWEEP_DOT(M.d, e) * ie, fm = RL_SWEEP_DOT(m, e) * ie;
		for (int k = 0; k < 3; ++k) { mp[k] = m[k] - fm * e[k]; dp[k] = M.d[k] - fd * e[k]; }
		float te;
		if (!SweepRoot(mp, dp, M.r, te)) continue;
		const float u = fm + te * fd;
		if (u >= 0.0f && u <= 1.0f && te < t) { t = te; feature = 1 + j; for (int k = 0; k < 3; ++k) point[k] = A[k] + u * e[k]; }
	}
	for (int j = 0; j < 3; ++j) {   // the vertices
		float m[3], tv;
		for (int k = 0; k < 3; ++k) m[k] = M.o[k] - V[j][k];
		if (SweepRoot(m, M.d, M.r, tv) && tv < t) { t = tv; feature = 4 + j; for (int k = 0; k < 3; ++k) point[k] = V[j][k]; }
	}
	return feature >= 0;
}

// W5: the triangle's time T = t >= Bt ? t : Bt
RL_SWEEP_HD float SweepTriangleT(float t, float Bt) { return t >= Bt ? t : Bt; }

#undef RL_SWEEP_CROSS
#undef RL_SWEEP_DOT

} // namespace rl
