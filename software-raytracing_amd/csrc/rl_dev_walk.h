// Device library, part 3 of 6: the closest-hit walks -- the box rules, the slab test, the analytic primitives, the one triangle test, and the three
// whole walks: Traverse (binary tree), TraverseLeafList (the leaf list in LDS) and Traverse4 (the 4-wide trees).
#pragma once

#include "rl_dev_scene.h"
#include "rl_slack.h"   // RL_BOX_WIDEN and RL_CANDIDATE_SLACK: the box tests' relative slack and the candidate rule's, shared with the host's restatements

namespace rl {

// A candidate that passed the triangle test counts only if the ray also passes the reference's own box test
// (geom/aabb.h:39-54, unwidened, t_max = FLT_MAX) on the triangle's exact AABB.  Why: the barycentric test accepts points a few
// ulp -- on slivers far more -- outside the triangle, i.e. outside every box around it; whether such a candidate is ever REACHED then
// depends on which boxes a traversal happens to test (BVH2 or BVH4, widened by 3 or 6 ulp, the reference's random tree).  With
// this rule the set of accepted hits is a property of the ray and the triangle alone: every schedule and tree width returns the
// same hit, and since every box of the reference's tree contains this AABB (and rounding is monotone) the reference accepts
// whatever is accepted here.  (What it accepts beyond that -- a hit outside the triangle's own box but inside its random
// parent's -- is tree-dependent on its side; the oracle counts those events so that tests can tell them from real mismatches.)
// RL_OWN_BOX_WIDEN_TMIN is a translation unit's setting, made before its includes, and only the ray queries' unit (rl_query.hip) sets it: there
// "the box's exit lies before tMin" is widened like the exit of every other box of a walk (Slab: tf * widen
// < tn); the box's own entry against its own exit -- does the ray pass the box at all -- stays exact, so a query accepts what a render accepts.  A render starts
// its rays at rayTMin, far from any surface the ray is meant to meet; a query's tMin is the caller's and may be a surface's own t (the point interval [t, t], or
// tMin = the previous hit's t).  The box of a triangle that lies in an axis plane is flat, its exit (corner - o) * (1 / d) is the plane's t up to an ulp, and
// unwidened "exit < tMin" then rejects, for about one such ray in ten, a hit with tMin <= t (tests/test_gpu_ray_query_intervals.py set 2).
#ifndef RL_OWN_BOX_WIDEN_TMIN
#define RL_OWN_BOX_WIDEN_TMIN 0
#endif
__device__ __forceinline__ bool OwnBoxPassBox(V3 mn, V3 mx, V3 o, V3 inv /* exact 1/d */, float tMin, float t);
__device__ __forceinline__ bool OwnBoxPass(V3 a, V3 b, V3 c, V3 o, V3 inv /* exact 1/d */, float tMin, float t)
{
	const V3 mn = v3(fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z));
	const V3 mx = v3(fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z));
	return OwnBoxPassBox(mn, mx, o, inv, tMin, t);
}
// the same with the box in hand (the leaf-list kernel's six-float4 triangle record keeps it in float4 4 and 5)
__device__ __forceinline__ bool OwnBoxPassMnMx(const float4* rec, V3 o, V3 inv, float tMin, float t)
{
	const float4 q4 = rec[4], q5 = rec[5];
	return OwnBoxPassBox(v3(q4.x, q4.y, q4.z), v3(q4.w, q5.x, q5.y), o, inv, tMin, t);
}
__device__ __forceinline__ bool OwnBoxPassBox(V3 mn, V3 mx, V3 o, V3 inv /* exact 1/d */, float tMin, float t)
{
	// (lo = t0 > lo ? t0 : lo and hi = t1 < hi ? t1 : hi -- a NaN keeps the old bound -- are fmaxf(lo, t0) and fminf(hi, t1), one v_max / v_min each
	// instead of a compare and a select; the sign of a zero, the one thing the two forms may disagree on, plays no part in the comparisons below)
#if RL_OWN_BOX_WIDEN_TMIN
	float lo = -INFINITY, hi = FLT_MAX;   // the box alone; tMin joins below
#else
	float lo = tMin, hi = FLT_MAX;
#endif
	{ float t0 = (mn.x - o.x) * inv.x, t1 = (mx.x - o.x) * inv.x; if (inv.x < 0.0f) { const float q = t0; t0 = t1; t1 = q; } lo = fmaxf(lo, t0); hi = fminf(hi, t1); }
	bool ok = !(hi < lo);
	{ float t0 = (mn.y - o.y) * inv.y, t1 = (mx.y - o.y) * inv.y; if (inv.y < 0.0f) { const float q = t0; t0 = t1; t1 = q; } lo = fmaxf(lo, t0); hi = fminf(hi, t1); }
	ok = ok && !(hi < lo);
	{ float t0 = (mn.z - o.z) * inv.z, t1 = (mx.z - o.z) * inv.z; if (inv.z < 0.0f) { const float q = t0; t0 = t1; t1 = q; } lo = fmaxf(lo, t0); hi = fminf(hi, t1); }
	// ... and the candidate's t must not lie before the ray enters that box (by more than the slack the box tests are
	// widened by): then "this box starts beyond the best hit so far" implies "nothing in it is closer", whatever the order
#if RL_OWN_BOX_WIDEN_TMIN
	// (hi only falls and lo only rises from axis to axis, so "hi < max(tMin, entries)" at any axis is "hi < tMin at the end, or hi < the entries at that axis")
	return ok && !(hi < lo) && !(hi * RL_BOX_WIDEN < tMin) && t * RL_CANDIDATE_SLACK >= fmaxf(lo, tMin);
#else
	return ok && !(hi < lo) && t * RL_CANDIDATE_SLACK >= lo;
#endif
}

// Slab test of one child box against [tMin, tMax] (reference geom/aabb.h:39-54:
// same products (bound - o) * invD, same "swap if invD < 0", NaN keeps the old
// bound).  tMax is widened by 2 ulp so the test stays conservative.
__device__ __forceinline__ bool Slab(float mnx, float mny, float mnz, float mxx, float mxy, float mxz,
                                     V3 o, V3 inv, bool nx, bool ny, bool nz, float tMin, float tMax, float& tNear, const float widen = RL_BOX_WIDEN)
{
	float tn = tMin, tf = tMax;
	float a0 = ((nx ? mxx : mnx) - o.x) * inv.x, a1 = ((nx ? mnx : mxx) - o.x) * inv.x;
	tn = fmaxf(tn, a0); tf = fminf(tf, a1);
	float b0 = ((ny ? mxy : mny) - o.y) * inv.y, b1 = ((ny ? mny : mxy) - o.y) * inv.y;
	tn = fmaxf(tn, b0); tf = fminf(tf, b1);
	float c0 = ((nz ? mxz : mnz) - o.z) * inv.z, c1 = ((nz ? mnz : mxz) - o.z) * inv.z;
	tn = fmaxf(tn, c0); tf = fminf(tf, c1);
	tNear = tn;
	return !(tf * widen < tn);
}

// v_rcp_f32 (1 ulp) is enough for the slab test's 1/d when the test is widened to 6 ulp (RL_POOL_WIDEN) instead of 3:
// Slab() is only asked to be conservative.  0 -> inf and the sign of a zero survive, as with the division.
__device__ __forceinline__ float FastRcp(float x) { return __builtin_amdgcn_rcpf(x); }
// ... and the exact one, RN(1 / d) per axis: what the candidate rule and the reference's own box test divide by
__device__ __forceinline__ V3 ExactInv(V3 d) { return v3(rtm::rcp1_(d.x), rtm::rcp1_(d.y), rtm::rcp1_(d.z)); }

// First traversal step only: true when the ray misses both child boxes of the root node.
template <int LDS = 0>
__device__ __forceinline__ bool RootMiss(const DSceneView& S, V3 o, V3 d, float tMin, const float4* sm = nullptr)
{
	// a filter: "true" only has to imply that a traversal finds nothing.  v_rcp_f32 reciprocals (1 ulp; 8 issue cycles each against the 36 of an
	// IEEE division) under the 1e-5 widening of every box test here, as in the pool schedule's slab tests.  0 -> inf and the sign of a zero survive.
#if RL_ROOTMISS_RCP
	const V3 inv = v3(FastRcp(d.x), FastRcp(d.y), FastRcp(d.z));
#else
	const V3 inv = ExactInv(d);
#endif
	const bool nx = inv.x < 0.0f, ny = inv.y < 0.0f, nz = inv.z < 0.0f;
	const float4* np = LDS ? sm + RL_LDS_ROOT : (const float4*)(S.nodes);
	const float4 q0 = np[0], q1 = np[1], q2 = np[2];
	const int4 k = ((const int4*)np)[3];
	float tl, tr;
	bool hl = Slab(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, o, inv, nx, ny, nz, tMin, FLT_MAX, tl);
	bool hr = Slab(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, o, inv, nx, ny, nz, tMin, FLT_MAX, tr);
	hl = hl && (k.x != DNODE_EMPTY);
	hr = hr && (k.y != DNODE_EMPTY);
	return !(hl || hr);
}

// stk: this lane's column of the LDS stack; entry k at stk[k * RL_BLOCK].
// Sphere::Hit (reference geom/sphere.cc:3-45): open interval (t_min, t_max); the near root if it is inside, else the
// far root.  t_max is the current best t (the reference compares all hits afterwards; same closest hit).
// tOpen: the interval's open upper end -- FLT_MAX for a render; a ray query's own tMax (SphereHitBelow).  A root outside (t_min, tOpen) is no root at all: it
// must not be returned and dropped later, or it shadows a cube at that same t, whose interval is closed and whose test asks "t < best".
// Returns t, or NaN for a miss (results by value: an out-parameter of an out-of-line function would live in scratch).
__device__ __forceinline__ float SphereRoots(const DSphere* spheres, int index, V3 o, V3 d, float t_min, float tBest, const float tOpen)
{
	const float4 q = ((const float4*)(spheres + index))[0];
	const V3 center = v3(q.x, q.y, q.z); const float radius = q.w;
	V3 oc = o - center;
	float a = dot(d, d);
	float b = dot(oc, d);
	float c = dot(oc, oc) - radius * radius;
	float D = b * b - a * c;
	if (D > 0.0f) {
		float temp = (-b - rtm::sqrt_(b * b - a * c)) / a;
		if (t_min < temp && temp < tOpen) return (temp < tBest) ? temp : NAN;   // the reference takes this root and compares later
		temp = (-b + rtm::sqrt_(b * b - a * c)) / a;
		if (t_min < temp && temp < tOpen) return (temp < tBest) ? temp : NAN;
	}
	return NAN;
}
__device__ __noinline__ float SphereHit(const DSphere* spheres, int index, V3 o, V3 d, float t_min, float tBest)
{
	return SphereRoots(spheres, index, o, d, t_min, tBest, FLT_MAX);
}
__device__ __noinline__ float SphereHitBelow(const DSphere* spheres, int index, V3 o, V3 d, float t_min, float tBest, float tOpen)
{
	return SphereRoots(spheres, index, o, d, t_min, tBest, tOpen);
}
// Cube::Hit (reference geom/cube.cc:3-43): slab box moving with velocity * max(0, rayTime - timeStartMove); closed
// interval [t_min, t_max]; entry face by the reference's float == chain (outFace 0..5 = -x +x -y +y -z +z, 6 = none matched).
// Returns (t, face as int bits), t = NaN for a miss.
__device__ __noinline__ float2 CubeHit(const DCube* cubes, int index, V3 o, V3 d, float rayTime, float t_min, float tBest)
{
	const float4* p = (const float4*)(cubes + index);
	const float4 q0 = p[0], q1 = p[1], q2 = p[2];
	const V3 velocity = v3(q2.x, q2.y, q2.z);
	const V3 movement = velocity * fmaxf(0.0f, rayTime - q0.w);
	const V3 mn = v3(q0.x, q0.y, q0.z) + movement, mx = v3(q1.x, q1.y, q1.z) + movement;
	const float t1 = (mn.x - o.x) / d.x, t2 = (mx.x - o.x) / d.x;
	const float t3 = (mn.y - o.y) / d.y, t4 = (mx.y - o.y) / d.y;
	const float t5 = (mn.z - o.z) / d.z, t6 = (mx.z - o.z) / d.z;
	// std::max(a, b) = (a < b) ? b : a; std::min(a, b) = (b < a) ? b : a
	#define RL_STDMAX(a, b) (((a) < (b)) ? (b) : (a))
	#define RL_STDMIN(a, b) (((b) < (a)) ? (b) : (a))
	const float mnx = RL_STDMIN(t1, t2), mny = RL_STDMIN(t3, t4), mnz = RL_STDMIN(t5, t6);
	const float mxx = RL_STDMAX(t1, t2), mxy = RL_STDMAX(t3, t4), mxz = RL_STDMAX(t5, t6);
	const float m12 = RL_STDMAX(mnx, mny); const float t7 = RL_STDMAX(m12, mnz);
	const float n12 = RL_STDMIN(mxx, mxy); const float t8 = RL_STDMIN(n12, mxz);
	#undef RL_STDMAX
	#undef RL_STDMIN
	if (t8 < 0 || t7 > t8) return make_float2(NAN, 0.0f);
	if (t_min <= t7 && t7 <= FLT_MAX && t7 < tBest) {
		const int face = (t7 == t1) ? 0 : (t7 == t2) ? 1 : (t7 == t3) ? 2 : (t7 == t4) ? 3 : (t7 == t5) ? 4 : (t7 == t6) ? 5 : 6;
		return make_float2(t7, __int_as_float(face));
	}
	return make_float2(NAN, 0.0f);
}

// The barycentric coordinates of a plane hit and their test, reference geom/triangle.cc:41-47:  pa = X / denom, pb = Y / denom, inside <=> 0 <= pa, 0 <= pb,
// pa + pb <= 1.  Two IEEE divisions are 72 of the ~380 issue cycles of a triangle step, and the divisor is a constant of the triangle: with rden = RN(1 / denom)
// from the record, rtm::div_by_ gives the same two quotients in 12 (all 2^46 significand pairs checked: tools/verify_fastdiv.hip).  Its conditions -- the ones
// v_div_scale tests -- are met like this:
//   * S.fastBary (host, rl_scene.cc FlattenScene): every triangle of the scene has denom == 0 or NaN (rden = NaN: both quotients NaN, "outside", as X / 0 and
//     X / NaN make it) or 2^-62 <= |denom| <= 2^125; a scene with any other divisor takes the divisions (a uniform branch);
//   * a quotient of at least 2^-38 then has |X| > 2^-101 (div_by_ wants 2^-102): exact.  Anything smaller -- tiny, zero (whose sign the short form may get wrong), negative by less
//     than that -- may be off in the last place, which cannot change "pa + pb <= 1" (a term below 2^-38 moves a sum near 1 by less than a thousandth of its
//     half-ulp), so: outside by more than 2^-38 is outside, inside by more than 2^-38 on both is inside, and the band between takes the divisions and the
//     reference's own test.  (A ray through a vertex or along an edge; tests/test_gpu_parity.py aims rays there.)
#ifndef RL_FAST_BARY
#define RL_FAST_BARY 1
#endif
__device__ __forceinline__ bool Barycentric(bool fast, float X, float Y, float denom, float rden, float& pa, float& pb)
{
#if RL_FAST_BARY
	if (fast) {
		pa = rtm::div_by_(X, denom, rden); pb = rtm::div_by_(Y, denom, rden);
		const float eps = 3.637978807091713e-12f;   // 2^-38
		const float m = __builtin_fminf(pa, pb), sum = pa + pb;   // (a NaN quotient: the sum is NaN)
		if (!(sum <= 1.0f && m >= -eps)) return false;
		if (m >= eps) return true;
	}
#endif
	pa = X / denom; pb = Y / denom;
	return 0.0f <= pa && 0.0f <= pb && pa + pb <= 1.0f;
}

// diagnostic build only: count wave-level steps (first active lane adds 1) next to the lane-level counters
#if defined(RL_DIAG_STAMPS) && RL_DIAG_STAMPS >= 2
#define RL_WSTEP(k) { const unsigned long long em_ = Ballot(1); if (c.diag && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)em_) - 1u) atomicAdd(&c.diag[CNT_COUNT + k], 1ull); }
#else
#define RL_WSTEP(k)
#endif

// A leaf reference (rl_device.h, DNode): ~ref = (first << 6) | (kind << 4) | (alphaTested << 3) | (count - 1).
struct LeafRef { int first, count; uint32_t kind; bool alpha; };
__device__ __forceinline__ LeafRef DecodeLeaf(int ref)
{
	const uint32_t code = (uint32_t)~ref;
	return { (int)(code >> LEAF_FIRST_SHIFT), (int)(code & LEAF_COUNT_MASK) + 1, (code >> LEAF_KIND_SHIFT) & LEAF_KIND_MASK, (code & LEAF_ALPHA_BIT) != 0u };
}

// The triangle test of every closest-hit search here, written once: Traverse, TraverseLeafList and Traverse4 below, LeafStep and LeafStep8 of the pool
// schedule (rl_dev_pool.h).  Which hit a ray gets is a property of the ray and the triangle alone, never of the tree, its width or the schedule -- and that
// holds only while all five apply the same rules: the tie rule, the barycentric test, the candidate rule, then the cut-out test.
//   T_       the triangle: a Tri, or anything with its v0, n, u, v, uv, uu, vv, denom, rden (the leaf list's LDS record)
//   slot_    its slot; best_ the search's HitRec; alpha_ whether its leaf runs the cut-out test (a compile-time false stays one); c_ the Counters
//   ownbox_  the candidate rule, OwnBoxPass / OwnBoxPassMnMx above, on the triangle's own box (the plane hit is `t` in it); anyhit_ leave the function with
//            `true` at the first accepted hit: a template argument in the walks, Trav's flag in the pool steps
//   ONLY_IF_ how a failed condition ends the test.  RL_ELSE_CONTINUE: the test is the body of a walk's loop over a leaf's triangles; RL_NESTED: one triangle per
//            call, the step's tail follows.  The same thing twice, but not to the compiler: with each kind of site in the form it was written in, every kernel is,
//            instruction for instruction, the one it was as five copies; one form for all, or a function, is not (profiles/r18_walk_dedup_isa_equivalence.log).
#define RL_ELSE_CONTINUE(ok_) if (!(ok_)) continue;
#define RL_NESTED(ok_) if (ok_)
#define RL_TRIANGLE_TEST(S_, T_, slot_, o_, d_, tMin_, best_, alpha_, ownbox_, anyhit_, c_, ONLY_IF_) { \
	/* the plane hit, reference geom/triangle.cc:22-27 */ \
	const float t = dot(((T_).v0 - (o_)), (T_).n) / dot((d_), (T_).n); \
	/* closer, or exactly as far with a lower slot: which of two surfaces at the same t wins must not depend on the order a traversal tests them in (the reference's answer depends on its random tree, SURVEY A) */ \
	ONLY_IF_(t >= (tMin_) && t <= FLT_MAX && (t < (best_).t || (t == (best_).t && (slot_) < (best_).tri))) { \
		const V3 p_ = (o_) + t * (d_); \
		const V3 w_ = p_ - (T_).v0; \
		const float wv_ = dot(w_, (T_).v), wu_ = dot(w_, (T_).u); \
		float pa_, pb_; \
		if (Barycentric((S_).fastBary != 0, (T_).uv * wv_ - (T_).vv * wu_, (T_).uv * wu_ - (T_).uu * wv_, (T_).denom, (T_).rden, pa_, pb_) && (ownbox_)) { \
			ONLY_IF_(!(alpha_) || AlphaTestCandidate(S_, slot_, pa_, pb_, c_)) { \
				(best_).t = t; (best_).a = pa_; (best_).b = pb_; (best_).tri = (slot_); \
				if (anyhit_) return true; \
			} \
		} \
	} \
}
// The leaf of one analytic primitive (kind 1: sphere, 2: cube: `first_` is its number), for Traverse and LeafStep; a macro for the same reason.
// open_ (a compile-time constant): a sphere's interval ends at tOpen_ instead of FLT_MAX.
#define RL_PRIMITIVE_LEAF(S_, kind_, first_, o_, d_, rayTime_, tMin_, best_, anyhit_, open_, tOpen_) { \
	float2 r_; \
	if ((kind_) == 1u) r_ = make_float2((open_) ? SphereHitBelow((S_).spheres, first_, o_, d_, tMin_, (best_).t, tOpen_) : SphereHit((S_).spheres, first_, o_, d_, tMin_, (best_).t), 0.0f); \
	else r_ = CubeHit((S_).cubes, first_, o_, d_, rayTime_, tMin_, (best_).t); \
	if (r_.x == r_.x) {   /* not NaN: a hit */ \
		(best_).t = r_.x; (best_).a = r_.y; (best_).b = 0.0f; (best_).tri = (int)(((kind_) << 28) | (uint32_t)(first_)); \
		if (anyhit_) return true; \
	} \
}

// "while-while" traversal: every lane first descends through inner nodes until it holds a leaf (cheap steps:
// one 64-byte record, two slab tests), THEN the wave intersects leaves together.  With a single
// "if inner else leaf" loop a wave pays node + leaf cost on every trip as soon as one lane is at a leaf, and
// the ~4x dearer triangle code ran with a handful of lanes (measured: 14 % VALU lane utilisation on the
// 298 k-triangle scene).
// tBound: where the search starts, "best" before any hit (the ray queries: the float above their tMax, rl_k_query.inl).
// OPEN, tOpen: the open end of a sphere's interval is tOpen instead of FLT_MAX (the ray queries with spheres: their tMax).
template <int STACK, bool ANYHIT, bool PRIMS, bool OPEN = false>
__device__ __forceinline__ bool Traverse(const DSceneView& S, V3 o, V3 d, float rayTime, float tMin, HitRec& best, int* stk, Counters& c, const float tBound = INFINITY,
                                         const float tOpen = FLT_MAX)
{
	c.rays++;
	const V3 inv = ExactInv(d);
	const bool nx = inv.x < 0.0f, ny = inv.y < 0.0f, nz = inv.z < 0.0f;
	best.t = tBound; best.tri = -1; best.a = 0.0f; best.b = 0.0f;
	int sp = 0;
	int cur = 0;                  // root is an inner node
	const int DONE = 0x7fffffff;  // not a node index (nodes < 2^31 - 1), not negative
	for (;;) {
		// ---- descend: inner nodes until this lane holds a leaf or has nothing left ----
		while (cur >= 0 && cur != DONE) {
			RL_WSTEP(4);
			const float4* np = (const float4*)(S.nodes + cur);
			const float4 q0 = np[0], q1 = np[1], q2 = np[2];
			const int4 k = ((const int4*)np)[3];
			c.nodes++;
			float tl, tr;
			const float tmx = fminf(best.t, FLT_MAX);
			bool hl = Slab(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, o, inv, nx, ny, nz, tMin, tmx, tl);
			bool hr = Slab(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, o, inv, nx, ny, nz, tMin, tmx, tr);
			hl = hl && (k.x != DNODE_EMPTY);
			hr = hr && (k.y != DNODE_EMPTY);
			if (hl && hr) {
				const bool leftFirst = tl <= tr;
				const int nearC = leftFirst ? k.x : k.y, farC = leftFirst ? k.y : k.x;
				if (sp < STACK) { stk[sp * RL_BLOCK] = farC; ++sp; }
				cur = nearC;
			} else if (hl) cur = k.x;
			else if (hr) cur = k.y;
			else if (sp == 0) cur = DONE;
			else { --sp; cur = stk[sp * RL_BLOCK]; }
		}
		if (cur == DONE) break;
		// ---- leaf: <= 4 triangles stored back to back, or one analytic primitive ----
		{
			RL_WSTEP(6);
			const LeafRef L = DecodeLeaf(cur);
			if (!PRIMS || L.kind == 0u) {
				for (int i = 0; i < L.count; ++i) {
					RL_WSTEP(5);
					const Tri T = LoadTri(S, L.first + i);
					c.tris++;
					RL_TRIANGLE_TEST(S, T, L.first + i, o, d, tMin, best, L.alpha, OwnBoxPass(T.v0, T.v1, T.v2, o, inv, tMin, t), ANYHIT, c, RL_ELSE_CONTINUE)
				}
			} else { c.tris++; RL_PRIMITIVE_LEAF(S, L.kind, L.first, o, d, rayTime, tMin, best, ANYHIT, OPEN, tOpen) }
		}
		if (sp == 0) break;
		--sp;
		cur = stk[sp * RL_BLOCK];
	}
	return best.tri >= 0;
}

// ---- one step on the wide tree: entry distances t0..t3 (INFINITY: not entered) of the four children of S.nodes4[cur] ----
// The 64-byte grid node (DNode4Q).  The planes are never decoded: with A = step * inv and B = (origin - o) * inv
// per axis, plane q's parameter is fma(q, A, B) -- one v_cvt_f32_ubyte and one v_fma per plane, four 16-byte loads per lane instead
// of seven.  The fused form rounds differently from the reference's (bound - o) * inv, by at most (|B| + 255 |A|) * 2^-23 in
// absolute terms (cancellation when the ray starts inside the node); four times that bound widens every slab -- near planes earlier,
// far planes later.  A box test only has to be conservative (the candidate rule decides what counts as a hit), so the image does
// not change.  A zero direction component (inv = +-inf) would turn the fused form into inf - inf: inv is clamped to +-1e30 for the
// box tests, which keeps the "no constraint while the origin lies between the planes" meaning and errs towards visiting.
__device__ __forceinline__ V3 ClampInv(V3 inv)
{
	// only infinities: a finite reciprocal, however large, scales its axis' parameters exactly as the reference's arithmetic does
	return v3(isinf(inv.x) ? copysignf(1e30f, inv.x) : inv.x, isinf(inv.y) ? copysignf(1e30f, inv.y) : inv.y, isinf(inv.z) ? copysignf(1e30f, inv.z) : inv.z);
}
typedef float rl_v4f __attribute__((ext_vector_type(4)));
typedef uint32_t rl_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 GLoadF4(const void* p, int i) { const rl_v4f v = ((const __attribute__((address_space(1))) rl_v4f*)p)[i]; return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ uint4 GLoadU4(const void* p, int i) { const rl_v4u v = ((const __attribute__((address_space(1))) rl_v4u*)p)[i]; return make_uint4(v.x, v.y, v.z, v.w); }
// the rounding of a grid node's fused plane parameters, four times over (above): (|B| + 255 |A|) * 2^-21 as |A * c1| + |B * c2| -- two multiplies by literals and an add with |.|
// modifiers, 2 issue cycles each; as an fma with 255 the constant sat in an SGPR (the three-operand encoding takes no literal) next to the |.| modifiers, and an SGPR operand makes it 4
#define RL_GRID_ERR(A_, B_) (fabsf((A_) * 1.21593475e-4f) + fabsf((B_) * 4.76837158e-7f))
// four children (entry distance, reference) in ascending order of entry distance: the five-comparator network
#define RL_SORT4_STEP(ta, ra, tb, rb) { const bool sw = tb < ta; const float tt = sw ? tb : ta; tb = sw ? ta : tb; ta = tt; const int rr = sw ? rb : ra; rb = sw ? ra : rb; ra = rr; }
#define RL_SORT4(t0, r0, t1, r1, t2, r2, t3, r3) RL_SORT4_STEP(t0, r0, t1, r1) RL_SORT4_STEP(t2, r2, t3, r3) RL_SORT4_STEP(t0, r0, t2, r2) RL_SORT4_STEP(t1, r1, t3, r3) RL_SORT4_STEP(t1, r1, t2, r2)
#define RL_WIDE_STEP_Q(S_, cur_, o_, inv_, nx_, ny_, nz_, tMin_, tmx_, widen_, t0, t1, t2, t3, ch) \
	/* (the loads spell the global address space out: the pool kernel keeps the base in a VGPR pair behind an empty asm statement, which hides where it */ \
	/*  points -- and a flat_load counts against the LDS counter as well and waits for both) */ \
	const DNode4Q* np_ = (S_).nodes4 + (cur_); \
	const float4 h0_ = GLoadF4(np_, 0); const uint4 l_ = GLoadU4(np_, 1); const uint4 u_ = GLoadU4(np_, 2); \
	const uint4 chu_ = GLoadU4(np_, 3); const int4 ch = make_int4((int)chu_.x, (int)chu_.y, (int)chu_.z, (int)chu_.w); \
	const float Ax_ = h0_.w * (inv_).x, Ay_ = __uint_as_float(l_.w) * (inv_).y, Az_ = __uint_as_float(u_.w) * (inv_).z; \
	const float Bx_ = (h0_.x - (o_).x) * (inv_).x, By_ = (h0_.y - (o_).y) * (inv_).y, Bz_ = (h0_.z - (o_).z) * (inv_).z; \
	const float Ex_ = RL_GRID_ERR(Ax_, Bx_), Ey_ = RL_GRID_ERR(Ay_, By_), Ez_ = RL_GRID_ERR(Az_, Bz_); \
	const float Bnx_ = Bx_ - Ex_, Bfx_ = Bx_ + Ex_, Bny_ = By_ - Ey_, Bfy_ = By_ + Ey_, Bnz_ = Bz_ - Ez_, Bfz_ = Bz_ + Ez_; \
	const uint32_t nX_ = (nx_) ? u_.x : l_.x, fX_ = (nx_) ? l_.x : u_.x, nY_ = (ny_) ? u_.y : l_.y, fY_ = (ny_) ? l_.y : u_.y, nZ_ = (nz_) ? u_.z : l_.z, fZ_ = (nz_) ? l_.z : u_.z; \
	const float tMinL_ = (tMin_), tmxL_ = (tmx_), widenL_ = (widen_); \
	float t0, t1, t2, t3; \
	RL_QSLAB(0, t0) RL_QSLAB(8, t1) RL_QSLAB(16, t2) RL_QSLAB(24, t3)
#define RL_QSLAB(sh, tk) { \
	float tn = tMinL_, tf = tmxL_; \
	tn = fmaxf(tn, __builtin_fmaf((float)((nX_ >> sh) & 0xffu), Ax_, Bnx_)); tf = fminf(tf, __builtin_fmaf((float)((fX_ >> sh) & 0xffu), Ax_, Bfx_)); \
	tn = fmaxf(tn, __builtin_fmaf((float)((nY_ >> sh) & 0xffu), Ay_, Bny_)); tf = fminf(tf, __builtin_fmaf((float)((fY_ >> sh) & 0xffu), Ay_, Bfy_)); \
	tn = fmaxf(tn, __builtin_fmaf((float)((nZ_ >> sh) & 0xffu), Az_, Bnz_)); tf = fminf(tf, __builtin_fmaf((float)((fZ_ >> sh) & 0xffu), Az_, Bfz_)); \
	tk = (tf * widenL_ < tn) ? INFINITY : tn; }
#define RL_WIDE_STEP_F(np_expr, o_, inv_, nx_, ny_, nz_, tMin_, tmx_, widen_, t0, t1, t2, t3, ch) \
	const float4* np_ = (np_expr); \
	const float4 lox_ = np_[0], loy_ = np_[1], loz_ = np_[2], hix_ = np_[3], hiy_ = np_[4], hiz_ = np_[5]; \
	const int4 ch = ((const int4*)np_)[6]; \
	const float4 nX_ = (nx_) ? hix_ : lox_, fX_ = (nx_) ? lox_ : hix_; \
	const float4 nY_ = (ny_) ? hiy_ : loy_, fY_ = (ny_) ? loy_ : hiy_; \
	const float4 nZ_ = (nz_) ? hiz_ : loz_, fZ_ = (nz_) ? loz_ : hiz_; \
	const float tMinL_ = (tMin_), tmxL_ = (tmx_), widenL_ = (widen_); const V3 oL_ = (o_), invL_ = (inv_); \
	float t0, t1, t2, t3; \
	RL_FSLAB(x, t0) RL_FSLAB(y, t1) RL_FSLAB(z, t2) RL_FSLAB(w, t3)
#define RL_FSLAB(k, tk) { \
	float tn = tMinL_, tf = tmxL_; \
	tn = fmaxf(tn, (nX_.k - oL_.x) * invL_.x); tf = fminf(tf, (fX_.k - oL_.x) * invL_.x); \
	tn = fmaxf(tn, (nY_.k - oL_.y) * invL_.y); tf = fminf(tf, (fY_.k - oL_.y) * invL_.y); \
	tn = fmaxf(tn, (nZ_.k - oL_.z) * invL_.z); tf = fminf(tf, (fZ_.k - oL_.z) * invL_.z); \
	tk = (tf * widenL_ < tn) ? INFINITY : tn; }

// A scene of at most 4 * RL_LEAFLIST_RECORDS leaves (rl_bvh.cc "the leaf list"), resident in LDS: no tree.  Every lane tests the box of every
// leaf, four to a record, in lockstep -- the same code on the same records for all 64 rays, so the wave pays for 1 walk, not for the union
// of 64 -- and keeps what it hit as sortable keys: the entry distance with the slot number in the 5 low mantissa bits, i.e. rounded DOWN by
// at most 31 ulp (nearer than the truth, so the cut below only comes later; a negative entry distance, possible with a negative rayTMin,
// counts as 0, and the cut is then not taken at all).  Then it visits its leaves nearest first and stops at the first one that starts behind the best hit -- the order and the cut
// of a tree walk.  The candidates are every leaf whose box the ray meets: a superset of those a tree walk opens, and with the candidate rule
// and the tie rule of the triangle test the result does not depend on which superset is tested in which order.  The cut is safe for the
// same reason every widened box test here is: an accepted hit has t * RL_CANDIDATE_SLACK >= the entry into its triangle's own box (OwnBoxPass),
// which lies inside the leaf's box, and RL_BOX_WIDEN exceeds RL_CANDIDATE_SLACK by 1e-6 -- four times the rounding of either side.
// Measured on the Cornell frame: DESIGN.md section 2.
// (Round 3, measured and not kept: the candidate rule applied once, to the winner of the search, instead of to every candidate that passes the barycentric
// test, with an out-of-line walk that applies it per candidate for the lane whose winner fails it.  Sound -- the search finds the nearest of a larger set, and
// a winner that passes the rule is the nearest of the smaller one too -- and 0.5 % faster, but the call made the register allocator keep the 24 keys in
// scratch memory: 28 GB of spill traffic per frame, three times everything else the kernel moves.)
// The candidate rule takes invb, the reciprocal of the box loop: the same bits as ExactInv(d).  Written as a second ExactInv(d) at the triangle test -- as the
// tree walks write it, where the reciprocal of the box tests may be a clamped one -- the compiler did not fold the two: behind the first pick it ran three
// whole IEEE expansions of 1 / x (v_div_scale x 2, v_rcp, five fma, v_div_fmas, v_div_fixup each) on every lane of every walk with a candidate, in each of the
// four walks the hit-queue kernel inlines: 0.137 G of its 5.97 G VALU instructions a frame and 3.3 % of its time ("one reciprocal per walk").
// (Measured there and not kept: the record count as a template argument, which takes the six scalar branches and little else out of the box loop -- the
// compiler had sunk the key presets into the branch not taken -- and the leaf count of the last record on top of it.)
// PLAIN: no leaf carries the cut-out bit (rl_plan.cc), so the walk does not test it.
template <bool ANYHIT, bool PLAIN = false>
__device__ __forceinline__ bool TraverseLeafList(const DSceneView& S, V3 o, V3 d, float tMin, HitRec& best, Counters& c, const float4* sm)
{
	c.rays++;
	const V3 invb = ExactInv(d);
	const bool nx = invb.x < 0.0f, ny = invb.y < 0.0f, nz = invb.z < 0.0f;
	best.t = INFINITY; best.tri = -1; best.a = 0.0f; best.b = 0.0f;
	uint32_t key[4 * RL_LEAFLIST_RECORDS];
	// The box test of the list is a filter, not the reference's test (that one is the candidate rule of the triangle test, on the
	// triangle's own box): it only has to let through every leaf the exact test would.  So the planes are one fma each,
	// t = plane * inv + c with c = -(o * inv), instead of (plane - o) * inv; c's rounding error, |c| * 2^-24, which the exact form does not
	// have when plane ~ o, is covered four times over by moving c outwards by |c| * 2^-22 (near planes down, far planes up), and the
	// relative errors by the same "tf * widen < tn" as every other box test here.  An infinite inv (a zero in d) turns the axis's terms
	// into NaN or into the harmless infinity, which max / min ignore: the axis then simply does not cull.  And the near / far plane of
	// an axis is picked by ADDRESS (the record holds lo.x lo.y lo.z hi.x hi.y hi.z, 16 bytes each) instead of by 24 selects per record.
	const V3 cc = v3(-(o.x * invb.x), -(o.y * invb.y), -(o.z * invb.z));
	const V3 ce = v3(fabsf(cc.x) * 2.3841858e-7f, fabsf(cc.y) * 2.3841858e-7f, fabsf(cc.z) * 2.3841858e-7f);
	const V3 cn = cc - ce, cf = cc + ce;
	const char* recs = (const char*)(sm + LdsAt<2>::NODES);
	const uint32_t oNX = nx ? 48u : 0u, oFX = 48u - oNX, oNY = ny ? 64u : 16u, oFY = 80u - oNY, oNZ = nz ? 80u : 32u, oFZ = 112u - oNZ;
	#pragma unroll
	for (int g = 0; g < RL_LEAFLIST_RECORDS; ++g) {
		key[4 * g] = key[4 * g + 1] = key[4 * g + 2] = key[4 * g + 3] = 0xffffffffu;
		if (g < S.numLeafRecords) {   // the same for every lane
			c.nodes += 2;             // 64-byte records fetched
			RL_WSTEP(4);
			const char* rec = recs + g * (RL_LDS_NSTRIDE * 16);
			const float4 nX = *(const float4*)(rec + oNX), fX = *(const float4*)(rec + oFX);
			const float4 nY = *(const float4*)(rec + oNY), fY = *(const float4*)(rec + oFY);
			const float4 nZ = *(const float4*)(rec + oNZ), fZ = *(const float4*)(rec + oFZ);
			// (This form -- 34 issue cycles per box for 46 by the cost table of tools/valu_calib.hip -- ran SLOWER twice in the first half of round 3, 14.80 ms for 14.31, while
			// the kernel still parked its arguments in VGPR lanes; with those reloads gone (RL_ARGS) it is 13.25 ms for 13.52.)
			// One box: six fma, max + max3, min3, and the key.  The exit needs no clamp to FLT_MAX (an axis without a constraint gives +inf or NaN, which min3 skips;
			// "NaN * widen < tn" is false: the box counts as met), and the entry no clamp to 0: this kernel only runs with rayTMin >= 0 (rl_plan.cc picks the
			// tree walk otherwise), so tn >= tMin >= 0 is a sortable key as it is.  RL_LL_SMEAR: "culled" as the sign of fma(exit, widen, -entry) smeared over the key.
			#ifndef RL_LL_SMEAR
			#define RL_LL_SMEAR 1
			#endif
			// (The smeared form works on the NEGATED entry distance, ntn = min(-tMin, -planes): the sign test is then fma(tf, widen, ntn) with the constant as the
			//  instruction's literal -- v_fmamk, 2 issue cycles; with "- tn" the compiler needs the three-operand encoding, which takes no literal, parks the
			//  constant in an SGPR and pays the 4 cycles of an SGPR operand -- and the key drops ntn's sign bit with the mask it applies anyway.)
			#define RL_LSLAB(k, slot) { \
				float tn = tMin, tf; \
				if (RL_LL_SMEAR) { \
					float ntn = -tMin; \
					ntn = fminf(ntn, -__builtin_fmaf(nX.k, invb.x, cn.x)); tf = __builtin_fmaf(fX.k, invb.x, cf.x); \
					ntn = fminf(ntn, -__builtin_fmaf(nY.k, invb.y, cn.y)); tf = fminf(tf, __builtin_fmaf(fY.k, invb.y, cf.y)); \
					ntn = fminf(ntn, -__builtin_fmaf(nZ.k, invb.z, cn.z)); tf = fminf(tf, __builtin_fmaf(fZ.k, invb.z, cf.z)); \
					key[slot] = ((__float_as_uint(ntn) & 0x7fffffe0u) | (uint32_t)(slot)) | (uint32_t)((int32_t)__float_as_uint(__builtin_fmaf(tf, RL_BOX_WIDEN, ntn)) >> 31); \
				} else { \
					tn = fmaxf(tn, __builtin_fmaf(nX.k, invb.x, cn.x)); tf = __builtin_fmaf(fX.k, invb.x, cf.x); \
					tn = fmaxf(tn, __builtin_fmaf(nY.k, invb.y, cn.y)); tf = fminf(tf, __builtin_fmaf(fY.k, invb.y, cf.y)); \
					tn = fmaxf(tn, __builtin_fmaf(nZ.k, invb.z, cn.z)); tf = fminf(tf, __builtin_fmaf(fZ.k, invb.z, cf.z)); \
					if (!(tf * RL_BOX_WIDEN < tn)) key[slot] = (__float_as_uint(tn) & ~31u) | (uint32_t)(slot); } }
			RL_LSLAB(x, 4 * g) RL_LSLAB(y, 4 * g + 1) RL_LSLAB(z, 4 * g + 2) RL_LSLAB(w, 4 * g + 3)
			#undef RL_LSLAB
		}
	}
	uint32_t from = 0u;   // keys below this one are done (keys are distinct: the slot is part of the key)
	// (One triangle per turn of ONE loop -- a lane picks its next leaf while its neighbours test their next triangle -- was measured too: 9.8
	// triangle steps per wave and bounce instead of 12 on 16 leaves, but 19.81 ms against 19.42: the pick costs more per turn than it saves.  Again on the
	// final kernel of round 3: 13.33 ms against 12.50.)
#ifdef RL_WATCHDOG
	int guardSel = 0;
#endif
	// the smallest key >= from, as the smallest (key - from) in unsigned arithmetic: an unused key (0xffffffff) lands on 0xffffffff - from and
	// a key below `from` (a leaf already visited) wraps around to more than that -- so "nothing left" is "the smallest is not below
	// 0xffffffff - from".  (Comparing the re-based minimum with 0xffffffff instead is wrong exactly when all 24 slots are candidates and
	// all have been visited: the minimum is then a wrapped one, never equals 0xffffffff, and the loop does not end.  tools/gpu_fuzz.py found it.)
	// The first pick (from == 0) needs no subtractions; the next one is made at the end of the loop's body.
	uint32_t m = 0xffffffffu;
	#pragma unroll
	for (int j = 0; j < 4 * RL_LEAFLIST_RECORDS; ++j) m = min(m, key[j]);
	for (;;) {
#ifdef RL_WATCHDOG
		if (++guardSel > 200) { printf("leaf-list pick stuck: lane %u from %u tMin %g best %g keys %u %u %u %u\n", threadIdx.x, from, tMin, best.t, key[0], key[1], key[2], key[3]); break; }
#endif
		if (m >= 0xffffffffu - from) break;
		m += from;
		// the nearest leaf left starts behind the hit (the slab test's own cut: tf * widen < tn; the keys are entry distances, rayTMin >= 0 here)
		if (best.t * RL_BOX_WIDEN < __uint_as_float(m & ~31u)) break;
		from = m + 1u;
		RL_WSTEP(6);
		const uint32_t j = m & 31u;
		const LeafRef L = DecodeLeaf(((const int*)(sm + LdsAt<2>::NODES + (j >> 2) * RL_LDS_NSTRIDE + 6))[j & 3u]);
#if defined(RL_DIAG_STAMPS) && RL_DIAG_STAMPS >= 2
		// diagnostic build: what regrouping the (ray, triangle) pairs of this round across the wave could save at best.  The lanes that visit a leaf in this
		// round test `count` triangles each; dealt evenly to 64 lanes the round's pairs would take ceil(pairs / 64) wave steps instead of max(count) -- and no
		// fewer than one, because a ray's next leaf depends on what this one yields (the nearest-first cut).  Summed in slot 7 next to the steps taken (slot 5).
		{
			uint32_t pairs = 0;
			for (int cc = 1; cc <= 8; ++cc) pairs += (uint32_t)cc * (uint32_t)__popcll(Ballot(L.count == cc));
			const unsigned long long em_ = Ballot(true);
			if (c.diag && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)em_) - 1u) atomicAdd(&c.diag[CNT_COUNT + 7], (unsigned long long)((pairs + 63u) / 64u));
		}
#endif
		for (int i = 0; i < L.count; ++i) {
			const float4* tr = sm + LdsAt<2>::ISECT + (L.first + i) * 6;
			const float4 q0 = tr[0], q1 = tr[1], q2 = tr[2], q3 = tr[3];
			struct { V3 v0, n, u, v; float uv, uu, vv, denom, rden; } T;
			T.v0 = v3(q0.x, q0.y, q0.z); T.n = v3(q0.w, q1.x, q1.y); T.u = v3(q1.z, q1.w, q2.x); T.v = v3(q2.y, q2.z, q2.w);
			T.uv = q3.x; T.uu = q3.y; T.vv = q3.z; T.denom = q3.w; T.rden = tr[5].z;
			c.tris++;
			RL_WSTEP(5);
			RL_TRIANGLE_TEST(S, T, L.first + i, o, d, tMin, best, !PLAIN && L.alpha, OwnBoxPassMnMx(tr, o, invb, tMin, t), ANYHIT, c, RL_ELSE_CONTINUE)
		}
		m = 0xffffffffu;
		#pragma unroll
		for (int j = 0; j < 4 * RL_LEAFLIST_RECORDS; ++j) m = min(m, key[j] - from);
	}
	return best.tri >= 0;
}

// The same closest-hit search on the BVH4 (DNode4): four slab tests per step, hit children ordered by entry distance.
// FULL: float boxes (S.nodes4f), else the grid nodes (S.nodes4)
template <int STACK, bool ANYHIT, bool PRIMS, bool FULL, int LDS = 0, bool PLAIN = false>
__device__ __forceinline__ bool Traverse4(const DSceneView& S, V3 o, V3 d, float rayTime, float tMin, HitRec& best, int* stk, Counters& c, const float4* sm = nullptr,
                                          const float tBound = INFINITY)
{
	if constexpr (LDS == 2) return TraverseLeafList<ANYHIT, PLAIN>(S, o, d, tMin, best, c, sm);
	c.rays++;
	V3 invb = ExactInv(d);   // for the box tests (the candidate rule divides again: exact, and rare)
	if (!FULL) invb = ClampInv(invb);
	const bool nx = invb.x < 0.0f, ny = invb.y < 0.0f, nz = invb.z < 0.0f;
	best.t = tBound; best.tri = -1; best.a = 0.0f; best.b = 0.0f;
	int sp = 0, cur = 0;
	const int DONE = 0x7fffffff;
	for (;;) {
		while (cur >= 0 && cur != DONE) {
			c.nodes += FULL ? 2 : 1;   // 64-byte records fetched
			RL_WSTEP(4);
			const float tmx = fminf(best.t, FLT_MAX);
			float t0, t1, t2, t3; int r0, r1, r2, r3;
			if (FULL) { RL_WIDE_STEP_F((LDS ? sm + RL_LDS_NODES + cur * RL_LDS_NSTRIDE : (const float4*)(S.nodes4f + cur)), o, invb, nx, ny, nz, tMin, tmx, RL_BOX_WIDEN, a0, a1, a2, a3, ch) t0 = a0; t1 = a1; t2 = a2; t3 = a3; r0 = ch.x; r1 = ch.y; r2 = ch.z; r3 = ch.w; }
			else { RL_WIDE_STEP_Q(S, cur, o, invb, nx, ny, nz, tMin, tmx, RL_BOX_WIDEN, a0, a1, a2, a3, ch) t0 = a0; t1 = a1; t2 = a2; t3 = a3; r0 = ch.x; r1 = ch.y; r2 = ch.z; r3 = ch.w; }
			if (r0 == DNODE_EMPTY) t0 = INFINITY;
			if (r1 == DNODE_EMPTY) t1 = INFINITY;
			if (r2 == DNODE_EMPTY) t2 = INFINITY;
			if (r3 == DNODE_EMPTY) t3 = INFINITY;
			RL_SORT4(t0, r0, t1, r1, t2, r2, t3, r3)
			if (!(t0 < INFINITY)) { if (sp == 0) cur = DONE; else { --sp; cur = stk[sp * RL_BLOCK]; } continue; }
			if (t3 < INFINITY && sp < STACK) { stk[sp * RL_BLOCK] = r3; ++sp; }
			if (t2 < INFINITY && sp < STACK) { stk[sp * RL_BLOCK] = r2; ++sp; }
			if (t1 < INFINITY && sp < STACK) { stk[sp * RL_BLOCK] = r1; ++sp; }
			cur = r0;
		}
		if (cur == DONE) break;
		{
			const LeafRef L = DecodeLeaf(cur);
			RL_WSTEP(6);
			for (int i = 0; i < L.count; ++i) {
				const Tri T = LDS ? TriFrom(sm + RL_LDS_ISECT + (L.first + i) * RL_LDS_TSTRIDE) : LoadTri(S, L.first + i);
				c.tris++;
				RL_WSTEP(5);
				RL_TRIANGLE_TEST(S, T, L.first + i, o, d, tMin, best, L.alpha, OwnBoxPass(T.v0, T.v1, T.v2, o, ExactInv(d), tMin, t), ANYHIT, c, RL_ELSE_CONTINUE)
			}
		}
		if (sp == 0) break;
		--sp;
		cur = stk[sp * RL_BLOCK];
	}
	(void)rayTime;
	return best.tri >= 0;
}

} // namespace rl
