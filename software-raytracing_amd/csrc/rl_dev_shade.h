// Device library, part 4 of 6: shading -- the surface interaction, the microfacet BRDF and its sampler, the material lookups, Scatter, and the
// miss shaders.
#pragma once

#include "rl_dev_walk.h"

namespace rl {

// ---------------------------------------------------------------------------
// Surface interaction (reference geom/hit.h:16-36)
struct Surf { float t; V3 p, n; float U, V; V3 tangent, bitangent; };

// the tangent frame of s.n (geom/hit.cc:6-18), for BuildSurface under RL_NORMALIZE_RANGED bit 1 (rl_dev_core.h).  RANGED: s.n is a unit vector to a few ulps (the caller's to guarantee), and neither normalisation needs a test:
// T is the axis with |s.n.axis| <= 0.9, so |cross(T, n)|^2 = 1 - n.axis^2 lies in [0.18, 1.01], and B is then a unit vector orthogonal to s.n to a few ulps:
// |cross(n, B)|^2 lies in [0.98, 1.02].  Both far inside NormalizeInRange's [2^-101, FLT_MAX].
template <bool RANGED>
__device__ __forceinline__ void BuildFrame(Surf& s)
{
	V3 T = (fabsf(s.n.x) > 0.9f) ? v3(0.0f, 1.0f, 0.0f) : v3(1.0f, 0.0f, 0.0f);
	V3 B = RANGED ? normalize_ranged_(cross(T, s.n)) : normalize(cross(T, s.n));
	T = RANGED ? normalize_ranged_(cross(s.n, B)) : normalize(cross(s.n, B));
	s.tangent = T; s.bitangent = B;
}
// HitResult for the winning primitive (reference geom/triangle.cc:43-47, geom/sphere.cc:19-41, geom/cube.cc:24-38)
// + the tangent frame (geom/hit.cc:6-18).  Returns the material index.
template <bool PRIMS, int LDS = 0>
__device__ __forceinline__ int BuildSurface(const DSceneView& S, V3 o, V3 d, const HitRec& h, Surf& s, bool basis, Counters& c, const float4* sm = nullptr)
{
	int material;
	s.t = h.t;
	s.p = o + h.t * d;
	const uint32_t kind = PRIMS ? (((uint32_t)h.tri) >> 28) : 0u;
	if (kind == 0u) {
		const Shade sh = LDS ? ShadeFrom(sm + LdsAt<LDS>::SHADE + h.tri * RL_LDS_TSTRIDE) : LoadShade(S, h.tri);
		c.shaded++;
		const float a = h.a, b = h.b;
#if RL_NORMALIZE_RANGED & 1
		// The interpolated normal is the scene's: a zero or NaN one must still give the reference's NaN, so its length is voted on.  Where the vote passes every
		// lane's s.n is a unit vector and the frame takes the ranged forms untested (BuildFrame); where it fails all three run the general form.
		const V3 nv = (1 - a - b) * sh.n0 + a * sh.n1 + b * sh.n2;
		if (rtm::wave_any_(!NormalizeInRange(nv.x * nv.x + nv.y * nv.y + nv.z * nv.z))) {
			s.n = normalize(nv);
			if (basis) BuildFrame<false>(s);
		} else {
			s.n = normalize_ranged_(nv);
			if (basis) BuildFrame<true>(s);
		}
#else
		s.n = normalize((1 - a - b) * sh.n0 + a * sh.n1 + b * sh.n2);
#endif
		s.U = (1 - a - b) * sh.s0 + a * sh.s1 + b * sh.s2;
		s.V = (1 - a - b) * sh.t0 + a * sh.t1 + b * sh.t2;
		material = sh.material;
	} else if (kind == 1u) {
		const float4* p = (const float4*)(S.spheres + (h.tri & 0x0fffffff));
		const float4 q = p[0];
		material = __float_as_int(p[1].x);
		c.shaded++;
		const V3 center = v3(q.x, q.y, q.z);
		s.n = (s.p - center) / q.w;
		const V3 op = s.p - center;
		s.U = rtm::atan_(op.y / op.x);
		s.V = rtm::acos_(op.z / q.w);
	} else {
		const float4* p = (const float4*)(S.cubes + (h.tri & 0x0fffffff));
		material = __float_as_int(p[1].w);
		c.shaded++;
		const int face = __float_as_int(h.a);
		s.n = (face == 0) ? v3(-1.0f, 0.0f, 0.0f) : (face == 1) ? v3(1.0f, 0.0f, 0.0f) : (face == 2) ? v3(0.0f, -1.0f, 0.0f)
		    : (face == 3) ? v3(0.0f, 1.0f, 0.0f) : (face == 4) ? v3(0.0f, 0.0f, -1.0f) : (face == 5) ? v3(0.0f, 0.0f, 1.0f) : v3s(0.0f);
		s.U = 0.0f; s.V = 0.0f;   // the reference leaves paramU / paramV unset for cubes
	}
#if RL_NORMALIZE_RANGED & 1
	if (basis && kind != 0u) BuildFrame<false>(s);   // (a triangle's frame was made beside its normal, above)
#else
	if (basis) {
		V3 T = (fabsf(s.n.x) > 0.9f) ? v3(0.0f, 1.0f, 0.0f) : v3(1.0f, 0.0f, 0.0f);
		V3 B = normalize(cross(T, s.n));
		T = normalize(cross(s.n, B));
		s.tangent = T; s.bitangent = B;
	}
#endif
	return material;
}
__device__ __forceinline__ V3 LocalToWorld(const Surf& s, V3 v)
{
	float wx = dot(v3(s.tangent.x, s.bitangent.x, s.n.x), v);
	float wy = dot(v3(s.tangent.y, s.bitangent.y, s.n.y), v);
	float wz = dot(v3(s.tangent.z, s.bitangent.z, s.n.z), v);
	return v3(wx, wy, wz);
}
__device__ __forceinline__ V3 WorldToLocal(const Surf& s, V3 v) { return v3(dot(v, s.tangent), dot(v, s.bitangent), dot(v, s.n)); }

// ---- microfacet BRDF pieces (reference render/brdf.h, render/material.cc:16-190) ----
__device__ __forceinline__ float Clampf(float val, float lo, float hi) { return fmaxf(lo, fminf(hi, val)); }

// (Inline since the end of round 3: as calls they measured better in round 2 (ErfInv / Erf inline 20.25 ms against 19.9), when the kernel had 400 SGPR reloads
//  to place around every call; with the arguments re-read per part of the loop, ErfInv + Erf + acosf inline are 12.26 ms against 12.45, 36.9 against 37.2 ms
//  on the 298 k frame.  powf stays a call: inline 12.65.)
#ifndef RL_ERFINV_ATTR
#define RL_ERFINV_ATTR __forceinline__
#endif
#ifndef RL_ERF_ATTR
#define RL_ERF_ATTR __forceinline__
#endif
__device__ RL_ERFINV_ATTR float ErfInv(float x)
{
	float w, p;
	x = Clampf(x, -.99999f, .99999f);
	w = -rtm::log_((1 - x) * (1 + x));
	if (w < 5) {
		w = w - 2.5f;
		p = 2.81022636e-08f;
		p = 3.43273939e-07f + p * w;
		p = -3.5233877e-06f + p * w;
		p = -4.39150654e-06f + p * w;
		p = 0.00021858087f + p * w;
		p = -0.00125372503f + p * w;
		p = -0.00417768164f + p * w;
		p = 0.246640727f + p * w;
		p = 1.50140941f + p * w;
	} else {
		w = rtm::sqrt_(w) - 3;
		p = -0.000200214257f;
		p = 0.000100950558f + p * w;
		p = 0.00134934322f + p * w;
		p = -0.00367342844f + p * w;
		p = 0.00573950773f + p * w;
		p = -0.0076224613f + p * w;
		p = 0.00943887047f + p * w;
		p = 1.00167406f + p * w;
		p = 2.83297682f + p * w;
	}
	return p * x;
}
__device__ RL_ERF_ATTR float Erf(float x)
{
	const float a1 = 0.254829592f, a2 = -0.284496736f, a3 = 1.421413741f, a4 = -1.453152027f, a5 = 1.061405429f;
	const float p = 0.3275911f;
	int sign = 1;
	if (x < 0) sign = -1;
	x = fabsf(x);
	float t = rtm::rcp1_(1 + p * x);
	float y = 1 - (((((a5 * t + a4) * t) + a3) * t + a2) * t + a1) * t * rtm::exp_(-x * x);
	return sign * y;
}
#if RL_NORMALIZE_RANGED & 8
// (voted: 1 - z z is an exact 0 for a direction along the normal, and NaN for a NaN one)
__device__ __forceinline__ float SinThetaL(V3 w) { return sqrt_voted_(fmaxf(0.0f, 1.0f - w.z * w.z)); }
#else
__device__ __forceinline__ float SinThetaL(V3 w) { return rtm::sqrt_(fmaxf(0.0f, 1.0f - w.z * w.z)); }
#endif

// ---- the scattering event's divisions in the short form (RL_EXACT_DIV bits 1 and 2, rl_glibc_math.h) ----
// (RL_EXACT_DIV is a translation unit's setting, made before its includes: the pool schedule's unit sets it to 0 and keeps every IEEE division, rl_render_pool.hip)
// An IEEE division is 36 VALU issue cycles; y = RN(1 / b) without rcp1_'s guard is 13 and each quotient rtm::div_by_(a, b, y) 7 more, a compare 4.4 (tools/valu_calib.hip).
// div_by_ is exact only under its conditions (rl_math.h): 2^-126 <= |b| < 2^126 here, |a| >= 2^-102 and a normal quotient.  The sites below take the short form where
// the divisor's range is known and test what is not with compares that fail on NaN; if any lane fails, the whole wave takes the IEEE divisions in a branch on the
// ballot (rarely taken: zero or tiny numerators, degenerate directions).  A site with nothing known about its divisor would pay two compares for it plus the
// numerator's and the quotient's (>= 20 cycles of guard, 41 in all): DistributionBeckmann, the pdf and the Newton step keep their divisions.
// |q| in [2^-91, 2^126): for a divisor in [2^-10, 8] this proves |a| >= 2^-102 and a normal quotient; a q computed from a zero, tiny, huge, infinite or NaN
// numerator or a NaN divisor falls outside (those stay within a few ulps of, or as far out as, the true quotient)
__device__ __forceinline__ bool QuotientInRange(float q) { return fabsf(q) >= 0x1p-91f && fabsf(q) < 0x1p126f; }
// the specular term's vec3 / float: b = 4 |N.Wi| |N.Wo| + 0.001 lies in [0.001, 4.001] (unit vectors) -- or is NaN
__device__ __forceinline__ V3 DivSpecular(V3 a, float b)
{
#if RL_EXACT_DIV & 1
	const float y = rlm::rcp1_in_range_(b);
	const V3 q = v3(rtm::div_by_(a.x, b, y), rtm::div_by_(a.y, b, y), rtm::div_by_(a.z, b, y));
	if (rtm::wave_any_(!(QuotientInRange(q.x) && QuotientInRange(q.y) && QuotientInRange(q.z)))) return a / b;
	return q;
#else
	return a / b;
#endif
}
__device__ __forceinline__ float CosPhi(V3 w) { float s = SinThetaL(w); return (s == 0) ? 1 : Clampf(w.x / s, -1, 1); }
__device__ __forceinline__ float SinPhi(V3 w) { float s = SinThetaL(w); return (s == 0) ? 0 : Clampf(w.y / s, -1, 1); }
#if RL_EXACT_DIV & 1
// CosPhi(w) and SinPhi(w) of one vector, sharing the divisor
__device__ __forceinline__ void CosSinPhi(V3 w, float& cosPhi, float& sinPhi)
{
	const float s = SinThetaL(w);
	// s is 0 or in [2^-12, 1] (1 - z z >= 2^-24 when it is positive), and |w.x|, |w.y| <= 1 + 2^-22: with numerators of at least 2^-102 every condition holds.  A zero
	// numerator (its sign would come out wrong), a tiny one or NaN sends the wave to the divisions; lanes with s = 0 take the constants and do not count.
	const float y = rlm::rcp1_in_range_(s);
	float qx = rtm::div_by_(w.x, s, y), qy = rtm::div_by_(w.y, s, y);
	if (rtm::wave_any_(!(s == 0 || (fabsf(w.x) >= 0x1p-102f && fabsf(w.y) >= 0x1p-102f)))) { qx = w.x / s; qy = w.y / s; }
	cosPhi = (s == 0) ? 1 : Clampf(qx, -1, 1);
	sinPhi = (s == 0) ? 0 : Clampf(qy, -1, 1);
}
#endif
// dot(V, H) / dot(V, N) <= 0 (RL_EXACT_DIV bit 2).  n / d <= 0 holds exactly when the quotient is a zero, a negative number or -inf:
//   n = +-0 with d neither zero nor NaN (+-0; 0 / 0 is NaN),
//   n nonzero, neither NaN, with opposite sign bits (-inf when d = +-0, a negative number otherwise) --
// except for a quotient that underflows to zero and d = +-inf, neither of which can happen here: d is the dot product of two unit vectors, |d| <= 1 + 2^-21, so it is
// finite, and |n / d| > 2^-150 for every n != 0 (denormals included), which rounds to a nonzero quotient.
__device__ __forceinline__ bool QuotientNotPositive(float n, float d)
{
#if RL_EXACT_DIV & 2
	const bool opposite = (int32_t)(__float_as_uint(n) ^ __float_as_uint(d)) < 0;
	return (n == 0.0f) ? __builtin_islessgreater(d, 0.0f) : (!__builtin_isunordered(n, d) && opposite);
#else
	return n / d <= 0.0f;
#endif
}

// k_trace's PLAIN instance has fewer registers to place around a call (no texture, cut-out or sky code): there the tan_ of GeometryBeckmann and the pow_ of
// the Fresnel term may be inlined, measured in DESIGN.md section 2.  Every other kernel keeps the calls.  (The sampler's pow_ stays a call everywhere: a template
// parameter on BeckmannSample would change how the compiler inlines it into every other kernel.)
#ifndef RL_PLAIN_INLINE_TAN
#define RL_PLAIN_INLINE_TAN 0
#endif
#ifndef RL_PLAIN_INLINE_POW
#define RL_PLAIN_INLINE_POW 0
#endif
template <bool INL> __device__ __forceinline__ float TanSel(float x) { return INL ? rtm::tan_inline_(x) : rtm::tan_(x); }
template <bool INL> __device__ __forceinline__ float PowSel(float x, float y) { return INL ? rtm::pow_inline_(x, y) : rtm::pow_(x, y); }

// ---- the ranged sampler (RL_SAMPLER_RANGED) ----
// A translation unit's setting, made before its includes as RL_EXACT_DIV is; off by default, and only the lazy instance's unit turns it on (rl_render_lazy.hip).
// BeckmannSample11 calls logf, expf, sqrtf and 1 / x with arguments that cannot reach those functions' special cases; with the setting on it calls their
// guard-free forms (rl_glibc_math.h *_in_range_) there.  Nothing is argued on paper: every piece is a function of ONE float, and RaylibAMD_VerifySamplerRanged
// (k_verify_sampler_ranged, rl_render_lazy.hip) compares it with the general form on all 2^32 bit patterns of that float.
//   the loop body, a function of b:  ErfInv clamps its argument to +-0.99999 (a NaN too: fminf and fmaxf drop it), so log_ sees (1 - x)(1 + x) in [2e-5, 1],
//       the tail's sqrt_ w in [5, 10.9], and exp_(-invErf invErf) an exponent in [-9.8, 0];
//   the prologue, a function of cosThetaI on [RL_SAMPLER_C_MIN, 0.9999]:  sinThetaI in [0.014, 1], tanThetaI in [0.014, 2^126], cotThetaI in [2^-126, 71],
//       1 + p cot >= 1, the normalization's argument in [1, 2^126): sqrt_, the tan division, both reciprocals and Erf's reciprocal lose their guards.  cotThetaI >= 0
//       there, so Erf takes no sign and its exp_(-x x) is the normalization's exp_(-cot cot): evaluated once.  That exp_ KEEPS its guard (its argument passes -88
//       at cotThetaI = 9.4, cosThetaI = 0.994, well inside the interval), and so does acos_.  Below C_MIN, at zero, negative or NaN the whole wave takes the
//       general prologue behind one vote (DivSpecular's form);
//   the branch on cosThetaI:  (double)cosThetaI > .9999 is cosThetaI >= RL_SAMPLER_COS_NEAR_ONE, the smallest float whose double exceeds .9999 (float(.9999)
//       itself rounds below it), for every bit pattern.
// pow_ (two inputs) and the Newton step's division (a divisor of unknown range) stay as they are.
#ifndef RL_SAMPLER_RANGED
#define RL_SAMPLER_RANGED 0
#endif
#define RL_SAMPLER_COS_NEAR_ONE 0x1.fff2e6p-1f   /* bits 0x3f7ff973; float(.9999) is 0x3f7ff972 = 0x1.fff2e4p-1 < .9999 */
// What the sweep yields: the two prologues agree on every float of [2^-126, 0x1.fff2e4p-1] and differ at the largest subnormal (the short reciprocal of cosThetaI
// leaves its range there) -- the bound the general form's tan division votes on already.
#define RL_SAMPLER_C_MIN 0x1p-126f
__device__ __forceinline__ float ErfInvRanged(float x)
{
	float w, p;
	x = Clampf(x, -.99999f, .99999f);
	w = -rtm::log_in_range_((1 - x) * (1 + x));
	if (w < 5) {
		w = w - 2.5f;
		p = 2.81022636e-08f;
		p = 3.43273939e-07f + p * w;
		p = -3.5233877e-06f + p * w;
		p = -4.39150654e-06f + p * w;
		p = 0.00021858087f + p * w;
		p = -0.00125372503f + p * w;
		p = -0.00417768164f + p * w;
		p = 0.246640727f + p * w;
		p = 1.50140941f + p * w;
	} else {
		w = rtm::sqrt_in_range_(w) - 3;
		p = -0.000200214257f;
		p = 0.000100950558f + p * w;
		p = 0.00134934322f + p * w;
		p = -0.00367342844f + p * w;
		p = 0.00573950773f + p * w;
		p = -0.0076224613f + p * w;
		p = 0.00943887047f + p * w;
		p = 1.00167406f + p * w;
		p = 2.83297682f + p * w;
	}
	return p * x;
}
// the Newton loop's two transcendentals of b: invErf = ErfInv(b) and exp_(-invErf invErf)
__device__ __forceinline__ void SamplerLoopTerms(float b, float& invErf, float& expTerm)
{
	invErf = ErfInv(b);
	expTerm = rtm::exp_(-invErf * invErf);
}
__device__ __forceinline__ void SamplerLoopTermsRanged(float b, float& invErf, float& expTerm)
{
	invErf = ErfInvRanged(b);
	expTerm = rtm::exp_in_range_(-invErf * invErf);
}
// the sampler's prologue below the .9999 branch, a function of cosThetaI: BeckmannSample11's statements (those of a unit without the setting)
__device__ __forceinline__ void SamplerPrologue(float cosThetaI, float& tanThetaI, float& c, float& fit, float& normalization)
{
	const float SQRT_PI_INV = 1.f / sqrtf(RL_PI);
	float sinThetaI = rtm::sqrt_(fmaxf((float)0, (float)1 - cosThetaI * cosThetaI));
#if RL_EXACT_DIV & 1
	tanThetaI = rtm::div_by_(sinThetaI, cosThetaI, rlm::rcp1_in_range_(cosThetaI));
	if (rtm::wave_any_(!(cosThetaI >= 0x1p-126f))) tanThetaI = sinThetaI / cosThetaI;
#else
	tanThetaI = sinThetaI / cosThetaI;
#endif
	float cotThetaI = rtm::rcp1_(tanThetaI);
	c = Erf(cotThetaI);
	float thetaI = rtm::acos_(cosThetaI);
	fit = 1 + thetaI * (-0.876f + thetaI * (0.4265f - 0.0594f * thetaI));
	normalization = rtm::rcp1_(1 + c + SQRT_PI_INV * tanThetaI * rtm::exp_(-cotThetaI * cotThetaI));
}
// ... and for RL_SAMPLER_C_MIN <= cosThetaI <= .9999 (the caller's to guarantee): the same bits
__device__ __forceinline__ void SamplerPrologueRanged(float cosThetaI, float& tanThetaI, float& c, float& fit, float& normalization)
{
	const float SQRT_PI_INV = 1.f / sqrtf(RL_PI);
	float sinThetaI = rtm::sqrt_in_range_((float)1 - cosThetaI * cosThetaI);   // (fmaxf(0, .) of a value >= 0.0002 is the value)
	tanThetaI = rtm::div_by_(sinThetaI, cosThetaI, rlm::rcp1_in_range_(cosThetaI));
	float cotThetaI = rlm::rcp1_in_range_(tanThetaI);
	const float expCot = rtm::exp_(-cotThetaI * cotThetaI);   // guarded: it underflows from cotThetaI = 9.4 on
	{	// Erf(cotThetaI) for cotThetaI >= 0
		const float a1 = 0.254829592f, a2 = -0.284496736f, a3 = 1.421413741f, a4 = -1.453152027f, a5 = 1.061405429f;
		const float p = 0.3275911f;
		float t = rlm::rcp1_in_range_(1 + p * cotThetaI);
		c = 1 - (((((a5 * t + a4) * t) + a3) * t + a2) * t + a1) * t * expCot;
	}
#if RL_NORMALIZE_RANGED & 8
	float thetaI = rtm::acos_in_range_(cosThetaI);   // (RaylibAMD_VerifyNormalizeRanged mode 1: every float of the interval)
#else
	float thetaI = rtm::acos_(cosThetaI);
#endif
	fit = 1 + thetaI * (-0.876f + thetaI * (0.4265f - 0.0594f * thetaI));
	normalization = rlm::rcp1_in_range_(1 + c + SQRT_PI_INV * tanThetaI * expCot);
}

// reference render/material.cc:83-165
// (__forceinline__ on the sampler and its caller below: the compiler inlined both into every kernel of its own accord until k_trace's PLAIN instance added
//  one more call site, after which it kept BeckmannSample out of line in all of them)
__device__ __forceinline__ void BeckmannSample11(float cosThetaI, float U1, float U2, float* slope_x, float* slope_y, Counters& cn)
{
	(void)cn;   // diagnostic builds count Newton iterations
	const float Pi = RL_PI;
#if RL_SAMPLER_RANGED
	if (cosThetaI >= RL_SAMPLER_COS_NEAR_ONE) {
#else
	if ((double)cosThetaI > .9999) {
#endif
		float r = rtm::sqrt_(-rtm::log_(1.0f - U1));
		float sinPhi, cosPhi; rtm::sincos_(2 * Pi * U2, &sinPhi, &cosPhi);
		*slope_x = r * cosPhi;
		*slope_y = r * sinPhi;
		return;
	}
#if RL_SAMPLER_RANGED
	// the ranged prologue for the wave; a lane outside its interval (tiny, zero, negative, NaN) sends the whole wave through the general one
	float tanThetaI, c, fit, normalization;
	SamplerPrologueRanged(cosThetaI, tanThetaI, c, fit, normalization);
	if (rtm::wave_any_(!(cosThetaI >= RL_SAMPLER_C_MIN))) SamplerPrologue(cosThetaI, tanThetaI, c, fit, normalization);
	float a = -1;
	float sample_x = fmaxf(U1, (float)1e-6f);
	float b = c - (1 + c) * rtm::pow_(1 - sample_x, fit);
	const float SQRT_PI_INV = 1.f / sqrtf(Pi);
#else
	float sinThetaI = rtm::sqrt_(fmaxf((float)0, (float)1 - cosThetaI * cosThetaI));
#if RL_EXACT_DIV & 1
	// cosThetaI <= .9999 here, so sinThetaI is in [0.014, 1]; with 2^-126 <= cosThetaI < 1 the quotient is in [0.014, 2^126] and div_by_'s conditions hold.
	// cosThetaI = +-0, tiny or NaN sends the wave to the division.
	float tanThetaI = rtm::div_by_(sinThetaI, cosThetaI, rlm::rcp1_in_range_(cosThetaI));
	if (rtm::wave_any_(!(cosThetaI >= 0x1p-126f))) tanThetaI = sinThetaI / cosThetaI;
#else
	float tanThetaI = sinThetaI / cosThetaI;
#endif
	float cotThetaI = rtm::rcp1_(tanThetaI);

	float a = -1, c = Erf(cotThetaI);
	float sample_x = fmaxf(U1, (float)1e-6f);

	float thetaI = rtm::acos_(cosThetaI);
	float fit = 1 + thetaI * (-0.876f + thetaI * (0.4265f - 0.0594f * thetaI));
	float b = c - (1 + c) * rtm::pow_(1 - sample_x, fit);

	const float SQRT_PI_INV = 1.f / sqrtf(Pi);
	float normalization = rtm::rcp1_(1 + c + SQRT_PI_INV * tanThetaI * rtm::exp_(-cotThetaI * cotThetaI));
#endif

	int it = 0;
	float invErf = 0.0f;
	bool converged = false;
	// The compiler unrolls this loop nine times whatever `#pragma nounroll` says (its trip count is a constant): 12 KB of code of which two or three copies ever
	// run.  Kept: with the limit hidden from the compiler (-DRL_NEWTON_ROLLED, round 5) the pool kernel is 10 KB shorter and every frame 0.6 - 1.1 % SLOWER
	// (298 k room from inside 89.3 against 88.4 ms, from outside 35.4 against 35.1, Cornell 12.39 against 12.30: profiles/r05_newton_rolled_ab.log).
	int newtonLimit = 10;
#ifdef RL_NEWTON_ROLLED
	asm volatile("" : "+s"(newtonLimit));
	#pragma nounroll
#endif
	while (++it < newtonLimit) {
		RL_WLSTEP(cn, 16, 17);
		if (!(b >= a && b <= c)) b = 0.5f * (a + c);
#if RL_SAMPLER_RANGED
		float expTerm; SamplerLoopTermsRanged(b, invErf, expTerm);
		float value = normalization * (1 + b + SQRT_PI_INV * tanThetaI * expTerm) - sample_x;
#else
		invErf = ErfInv(b);
		float value = normalization * (1 + b + SQRT_PI_INV * tanThetaI * rtm::exp_(-invErf * invErf)) - sample_x;
#endif
		float derivative = normalization * (1 - invErf * tanThetaI);
		if (fabsf(value) < 1e-5f) { converged = true; break; }
		if (value > 0) c = b; else a = b;
		b -= value / derivative;
	}
	// the reference evaluates ErfInv(b) once more here (material.cc:163); after the break b is still the argument invErf was computed from,
	// so the value is in hand -- only a lane that used up its nine iterations has moved b since (a whole ErfInv per scattering event less)
#if RL_SAMPLER_RANGED
	*slope_x = converged ? invErf : ErfInvRanged(b);
	*slope_y = ErfInvRanged(2.0f * fmaxf(U2, (float)1e-6f) - 1.0f);
#else
	*slope_x = converged ? invErf : ErfInv(b);
	*slope_y = ErfInv(2.0f * fmaxf(U2, (float)1e-6f) - 1.0f);
#endif
}
// reference render/material.cc:166-190
__device__ __forceinline__ V3 BeckmannSample(V3 wi, float alpha_x, float alpha_y, float U1, float U2, Counters& cn)
{
#if RL_NORMALIZE_RANGED & 2
	V3 wiStretched = normalize_voted_(v3(alpha_x * wi.x, alpha_y * wi.y, wi.z));   // (a grazing wi under a small alpha is arbitrarily short)
#else
	V3 wiStretched = normalize(v3(alpha_x * wi.x, alpha_y * wi.y, wi.z));
#endif
	float slope_x, slope_y;
	BeckmannSample11(wiStretched.z, U1, U2, &slope_x, &slope_y, cn);
#if RL_EXACT_DIV & 1
	float cosPhi, sinPhi; CosSinPhi(wiStretched, cosPhi, sinPhi);
	float tmp = cosPhi * slope_x - sinPhi * slope_y;
	slope_y = sinPhi * slope_x + cosPhi * slope_y;
#else
	float tmp = CosPhi(wiStretched) * slope_x - SinPhi(wiStretched) * slope_y;
	slope_y = SinPhi(wiStretched) * slope_x + CosPhi(wiStretched) * slope_y;
#endif
	slope_x = tmp;
	slope_x = alpha_x * slope_x;
	slope_y = alpha_y * slope_y;
#if RL_NORMALIZE_RANGED & 2
	// len2 = (sx sx + sy sy) + 1 is at least 1 and finite when the slopes are.  Voted all the same, and not proved from ErfInvRanged's clamp: the .9999 branch's
	// slopes are r cos, r sin with r = sqrt_(-log_(1 - U1)), infinite at U1 = 1, and the alphas are the caller's; the vote is one compare and a scalar branch.
	return normalize_voted_(v3(-slope_x, -slope_y, 1.f));
#else
	return normalize(v3(-slope_x, -slope_y, 1.f));
#endif
}
// reference render/brdf.h:39-58
__device__ __forceinline__ float DistributionBeckmann(V3 N, V3 H, float roughness)
{
	float cosH = dot(N, H);
	if (roughness == 0.0f) return 1.0f;
	if (H.z < 0.0f) cosH = -cosH;
	float cosH2 = cosH * cosH;
	float rr = roughness * roughness;
	float exp_x = (1.0f - cosH2) / (rr * cosH);
	float num = (cosH > 0.0f ? 1.0f : 0.0f) * rtm::exp_(-exp_x);
	float denom = RL_PI * rr * cosH2 * cosH2;
	return num / denom;
}
// reference render/brdf.h:74-93
template <bool ITAN = false>
__device__ __forceinline__ float GeometryBeckmann(V3 N, V3 H, V3 V, float roughness)
{
	float thetaV = rtm::acos_(dot(N, V));
	float tanThetaV = TanSel<ITAN>(thetaV);
	float a = rtm::rcp1_(roughness * tanThetaV);
	float aa = a * a;
	if (QuotientNotPositive(dot(V, H), dot(V, N))) return 0.0f;
	if (a < 1.6f) {
		float num = 3.535f * a + 2.181f * aa;
		float denom = 1.0f + 2.276f * a + 2.577f * aa;
		return num / denom;
	}
	return 1.0f;
}

// ---- the reflectance of one microfacet scattering event (reference render/material.cc:306-333) ----
// Its arithmetic is written once, here: from baseColor, roughness, metallic, N, Wo, Wh, Wi and NdotWi in scope, RL_REFLECTANCE_TERMS declares the terms in the
// reference's statement order and RL_REFLECTANCE_VALUE is the reflectance.  ReflFromRecord is that arithmetic as a function of what a vertex record of k_trace's lazy
// instance holds (FoldLazyVertex).  Scatter expands the same two macros in place and not through the function: the compiler simplifies an inlined callee on its own
// first, where kD and diffuse sink below DivSpecular's branch, and every kernel that scatters eagerly would come out as a different instruction sequence
// (tools/isa_equivalence.py: 19 kernels of the main unit alone).  The values are the same either way: no operation is reassociated or contracted.
#define RL_REFLECTANCE_TERMS(PLAIN_) \
	V3 F0 = v3s(0.04f); \
	F0 = mix(F0, baseColor, metallic); \
	V3 F = F0 + (1.0f - F0) * PowSel<PLAIN_ && RL_PLAIN_INLINE_POW>(1.0f - absDot(Wh, Wo), 5.0f); \
	float ggx2 = GeometryBeckmann<PLAIN_ && RL_PLAIN_INLINE_TAN>(N, Wh, Wo, roughness); \
	float ggx1 = GeometryBeckmann<PLAIN_ && RL_PLAIN_INLINE_TAN>(N, Wh, Wi, roughness); \
	float G = rtm::rcp1_(1.0f + ggx1 * ggx2); \
	float NDF = DistributionBeckmann(N, Wh, roughness); \
	\
	V3 kS = F; \
	V3 kD = 1.0f - kS; \
	V3 diffuse = baseColor * (1.0f - metallic); \
	V3 specular = DivSpecular(F * G * NDF, 4.0f * NdotWi * absDot(N, Wo) + 0.001f)
#define RL_REFLECTANCE_VALUE ((kD * diffuse + kS * specular) * NdotWi)
template <bool PLAIN = false>
__device__ __forceinline__ V3 ReflFromRecord(V3 baseColor, float roughness, float metallic, V3 N, V3 Wo, V3 Wh, V3 Wi, float NdotWi)
{
	RL_REFLECTANCE_TERMS(PLAIN);
	return RL_REFLECTANCE_VALUE;
}

// material texture lookups (reference render/material.cc:297-303,378-395,406-415)
__device__ __forceinline__ V3 GetAlbedo(const DSceneView& S, const Mat& m, float U, float V, Counters& c)
{
	if (m.type == MAT_LAMBERTIAN || m.type == MAT_METAL) return m.albedo;
	if (m.type == MAT_MICROFACET) {
		V3 albedo = m.albedo;
		if (m.tex0 >= 0) { float4 px = TexSample(S, m.tex0, false, U, V, c); albedo = v3(px.x, px.y, px.z) * px.w; }   // tex0: the pow(2.2) copy made at upload
		return albedo;
	}
	return v3s(0.0f);
}
__device__ __forceinline__ float GetRoughness(const DSceneView& S, const Mat& m, float U, float V, Counters& c)
{
	float roughness = m.roughness;
	if (m.tex2 >= 0) roughness = TexSample(S, m.tex2, false, U, V, c).x;
	return roughness;
}
__device__ __forceinline__ V3 GetMicrosurfaceNormal(const DSceneView& S, const Mat& m, const Surf& s, Counters& c)
{
	if (m.type == MAT_MICROFACET && m.tex1 >= 0) {
		float4 px = TexSample(S, m.tex1, false, s.U, s.V, c);
		V3 N = v3(px.x, px.y, px.z);
		N = normalize(2.0f * N - 1.0f);
		return N;
	}
	return v3(0.0f, 0.0f, 1.0f);
}
__device__ __forceinline__ bool IsMirrorLike(const DSceneView& S, const Mat& m, float U, float V, Counters& c)
{
	if (m.type == MAT_DIELECTRIC || m.type == MAT_MIRROR) return true;
	if (m.type == MAT_MICROFACET) return GetRoughness(S, m, U, V, c) < 0.1f;
	return false;
}
// reference render/material.cc:342-350, material.h:67-69
__device__ __forceinline__ V3 Emitted(const DSceneView& S, const Mat& m, const Surf& s, Counters& c)
{
	if (m.type == MAT_DIFFUSE_LIGHT) return m.albedo;
	if (m.type == MAT_MICROFACET) {
		V3 emit = m.emissive;
		if (m.tex4 >= 0) { float4 px = TexSample(S, m.tex4, false, s.U, s.U, c); emit = v3s(px.z); }  // (U,U) and vec3(b): reference bugs kept
		return emit;
	}
	return v3s(0.0f);
}

// One scattering event.  Returns false when the material does not scatter.
// Outputs reflectance, new direction, pdf and ScatteringPdf (the value the
// reference recomputes at renderer.cc:144).
// PLAIN: k_trace's instance for plain scenes (MatFrom<true>), which takes the inlining choices above.
template <bool PLAIN = false>
__device__ __forceinline__ bool Scatter(const DSceneView& S, const Mat& m, V3 inD, const Surf& s, Rng& g, Counters& c,
                                        V3& refl, V3& outD, float& pdf, float& sp)
{
	switch (m.type) {
		case MAT_DIFFUSE_LIGHT: return false;
		case MAT_LAMBERTIAN: {   // material.cc:195-219
			V3 N = s.n;
			V3 r = RandomInUnitSphere(g);
			if ((double)dot(r, N) < 0.0) r = -r;
			V3 Wi = normalize(r);
			outD = Wi;
			refl = m.albedo;
			pdf = absDot(N, Wi) / RL_PI;
			sp = fmaxf(0.0f, dot(s.n, Wi)) / RL_PI;
			return true;
		}
		case MAT_METAL: {        // material.cc:225-239
			V3 ud = normalize(inD);
			V3 reflected = reflect(ud, s.n);
			outD = reflected + m.fuzz * RandomInUnitSphere(g);
			refl = m.albedo;
			pdf = 1.0f;
			sp = 1.0f / RL_PI;
			return dot(outD, s.n) > 0.0f;
		}
		case MAT_MIRROR: {       // material.h:149-162
			refl = m.albedo;
			outD = reflect(inD, s.n);
			pdf = 1.0f;
			sp = 1.0f;
			return true;
		}
		case MAT_DIELECTRIC: {   // material.cc:244-285
			V3 outward_normal;
			V3 reflected = reflect(inD, s.n);
			float ni_over_nt;
			refl = m.transmission;
			V3 refracted = v3s(0.0f);
			float reflect_prob, cosine;
			if (dot(inD, s.n) > 0.0f) {
				outward_normal = -s.n;
				ni_over_nt = m.ior;
				cosine = m.ior * dot(inD, s.n) / length(inD);
			} else {
				outward_normal = s.n;
				ni_over_nt = rtm::rcp1_(m.ior);
				cosine = -dot(inD, s.n) / length(inD);
			}
			bool bRefract;
			{   // vec3.h:136-145
				V3 uv = normalize(inD);
				float dt = dot(uv, outward_normal);
				float D = 1.0f - ni_over_nt * ni_over_nt * (1.0f - dt * dt);
				bRefract = D > 0.0f;
				if (bRefract) refracted = ni_over_nt * (uv - outward_normal * dt) - outward_normal * rtm::sqrt_(D);
			}
			if (bRefract) {
				float r0 = (1.0f - m.ior) / (1.0f + m.ior);
				r0 = r0 * r0;
				reflect_prob = r0 + (1.0f - r0) * rtm::pow_((1.0f - cosine), 5.0f);
			} else {
				reflect_prob = 1.0f;
			}
			outD = (Next(g) < reflect_prob) ? reflected : refracted;
			pdf = 1.0f;
			sp = 1.0f / RL_PI;
			return true;
		}
		default: {               // MicrofacetMaterial, material.cc:290-340,352-376,417-431
			RL_CSTAMP_BEGIN(c);
			RL_WLSTEP(c, 18, 19);
			V3 baseColor = GetAlbedo(S, m, s.U, s.V, c);
			float roughness = GetRoughness(S, m, s.U, s.V, c);
			float metallic = m.metallic;
			if (m.tex3 >= 0) metallic = TexSample(S, m.tex3, false, s.U, s.V, c).x;

			V3 N = GetMicrosurfaceNormal(S, m, s, c);
			V3 Wo = WorldToLocal(s, -inD);
			float u0 = Next(g);
			float u1 = Next(g);
			bool bFlip = Wo.z < 0.0f;
			RL_CSTAMP(c, 0);
			V3 Wh = BeckmannSample(bFlip ? -Wo : Wo, roughness, roughness, u0, u1, c);
			RL_CSTAMP(c, 1);
			if (bFlip) Wh = -Wh;
			V3 Wi = reflect(-Wo, Wh);
			float NdotWi = absDot(N, Wi);

			RL_REFLECTANCE_TERMS(PLAIN);

			V3 WiW = LocalToWorld(s, Wi);
			outD = WiW;
			refl = RL_REFLECTANCE_VALUE;

			// ScatteringPdf(hit, -inD, WiW), material.cc:352-376
			V3 wo = WorldToLocal(s, -inD);
			V3 wi = WorldToLocal(s, WiW);
			V3 wh = normalize(wo + wi);
			if (wh.z < 0.0f) wh.z = -wh.z;
			float D = DistributionBeckmann(N, wh, roughness);
			sp = D * absDot(wh, N);
			pdf = sp / (4.0f * dot(Wo, Wh));
			RL_CSTAMP(c, 2);
			return true;
		}
	}
}

// ---- the ScatteringPdf part of a lazy event, decided without evaluating it ----
// Scatter ends with D = DistributionBeckmann(N, wh, r), sp = D |wh.z|, pdf = sp / (4 Wo.Wh) of the recomputed half vector wh.  On an unlit path (98 % of the headline
// frame's) the kernel reads two predicates of them and no value: pdf > 0 (does the path go on?) and |sp| < inf (LazyVertexSafe).  LazyPdfQuick decides both from the
// floats DistributionBeckmann would divide -- c = wh.z (flipped: >= 0), A = 1 - c c, B = r r c -- and from w = Wo.Wh.  Every compare is false on NaN.
// Why LazyPdfQuick, with r in [2^-10, 1] (SceneLazyRefl), implies 0 < pdf and 0 < sp < inf as Scatter computes them:
//   wh:  wh = v rcp1_(|v|) with c = v.z k in [2^-10, 1 + 2^-20]: |v| is finite and not zero (k = 0 or k = inf leaves c a zero or NaN, a NaN length a NaN) and
//        then every component of v is finite and at most |v| (1 + 2^-22) in magnitude: wh.x and wh.y are finite, within a few ulps of [-1, 1].  So dot(N, wh) with
//        N = (0, 0, 1) is 0 wh.x + 0 wh.y + c = c exactly (c is not a zero), cosH = c, cosH2 = fl(c c), and DistributionBeckmann's operands are A and B.
//   exp_x = fl(A / B): B = fl(rr c) >= 2^-30 is a positive normal number and 32 B is exact; A <= 32 B gives exp_x <= 32 (division is monotone, 32 a float).
//        A < 0 needs c > 1, where c <= 1 + 2^-20 gives A >= -(2^-19 + 2^-40) and B >= rr >= 2^-20: exp_x >= -2.000002.  exp_x in [-2.1, 32].
//   num = 1 * exp_(-exp_x) in [1.2e-14, 8.2]: a positive normal number (exp_ is within an ulp of e^x).
//   denom = pi rr c^4 in [pi 2^-60, pi (1 + 2^-20)^4] = [2.7e-18, 3.2], positive and normal at every step (rr >= 2^-20, cosH2 >= 2^-20).
//   D = num / denom in [3.9e-15, 3.1e18]; sp = D c in [3.8e-18, 3.1e18]: both positive, finite and far from the subnormals, whatever the last-bit roundings
//        are.  4 w lies in (0, 8] (or is flushed to +0), and pdf = sp / (4 w) >= 4.7e-19: positive, +inf where w is tiny, never NaN or a zero.
//   w:   only w > 0 is asked, not LazyVertexSafe's w >= 2^-10: an event between the two continues with the pdf's sign decided here, and fails that guard
//        behind it as it always did.  (Of the device sweep's events 9.1 % have w <= 0 -- its Wo.z = 0 inputs, the event's pdf is not positive and the path ends --
//        and 11.3 % lie in between; with w >= 2^-10 here every one of those would evaluate the pdf for nothing.)
// A quick event therefore continues (pdf > 0) and passes LazyVertexSafe's sp compare without D, sp or pdf being computed; the record's sp slot holds c, and the
// fold computes sp = DistributionBeckmann(N, (0, 0, c), r) |c| and pdf = sp / (4 Wo.Wh) -- the same operations on the same floats, dot(N, (0, 0, c)) being c as
// above -- for the lit paths alone (LazyRecordPdf).  An event that is not quick (a grazing half vector, a sampled D below e^-32, Wo in or behind the microfacet's
// plane, any NaN) evaluates the three as Scatter does and its record says so (RL_LAZY_REC_EXACT_SP).  RaylibAMD_VerifyLazyPdf sweeps the claim on the device.
__device__ __forceinline__ bool LazyPdfQuick(float c, float roughness, float w)
{
	const float rr = roughness * roughness, A = 1.0f - c * c, B = rr * c;
	return c >= 0x1p-10f && c <= 1.0f + 0x1p-20f && A <= 32.0f * B && w > 0.0f && w <= 2.0f;
}
// wh: the recomputed half vector, flipped to wh.z >= 0.  Returns whether sp and pdf are the event's values (false: sp holds wh.z, and pdf a stand-in that is
// positive as the event's is).  The slow side is entered by the whole wave when one lane needs it (DivSpecular's form: no divergent region around the division
// sequences), and changes nothing in a quick lane.
__device__ __forceinline__ bool LazyScatterPdf(V3 N, V3 Wo, V3 Wh, V3 wh, float roughness, float& sp, float& pdf)
{
	const float w = dot(Wo, Wh);
	const bool quick = LazyPdfQuick(wh.z, roughness, w);
	sp = wh.z;
	pdf = 1.0f;
	if (rtm::wave_any_(!quick)) {
		const float D = DistributionBeckmann(N, wh, roughness);
		const float spExact = D * absDot(wh, N);
		const float pdfExact = spExact / (4.0f * dot(Wo, Wh));
		if (!quick) { sp = spExact; pdf = pdfExact; }
	}
	return !quick;
}
// sp and pdf of a recorded microfacet vertex (r0 = Wo, sp slot; r1 = Wh, material index and RL_LAZY_REC_EXACT_SP), bit for bit what Scatter computes at the event
__device__ __forceinline__ void LazyRecordPdf(float4 r0, float4 r1, float roughness, float& sp, float& pdf)
{
	const V3 Wo = v3(r0.x, r0.y, r0.z), Wh = v3(r1.x, r1.y, r1.z);
	sp = r0.w;
	if ((__float_as_int(r1.w) & RL_LAZY_REC_EXACT_SP) == 0) {
		const V3 N = v3(0.0f, 0.0f, 1.0f), wh = v3(0.0f, 0.0f, r0.w);
		const float D = DistributionBeckmann(N, wh, roughness);
		sp = D * absDot(wh, N);
	}
	pdf = sp / (4.0f * dot(Wo, Wh));
}
// ---- k_trace's lazy-reflectance instance (rl_k_trace.inl RL_LAZY_REFL; rl_plan.cc TracePlan::lazy) ----
// A sample is the fold L_k = (0 + refl_k * L_{k+1} * sp_k / pdf_k) + E_k back to the camera.  On a path whose terminal L and every E are +0 each refl_k is
// multiplied by an exact zero: the sample is (+0, +0, +0) whatever the reflectances are -- as long as they and sp are finite (below).  The instance therefore
// scatters without the reflectance (ScatterLazy: everything the continuation needs), records what the reflectance is a function of, and evaluates it
// (FoldLazyVertex) for the paths with light in them alone.  Plain scenes whose triangles carry microfacet and mirror materials only (SceneLazyRefl): no
// texture lookups, N = (0, 0, 1).  A mirror's reflectance is its albedo, a constant there is nothing to skip of; its record holds the material alone.
// Scatter's mirror arm, or its microfacet arm without the reflectance: the same draws, the same statements, the same bits in Wo, Wh, outD, pdf and sp.
// pdf and sp are what LazyScatterPdf (above) leaves: exactSp says which.
__device__ __forceinline__ void ScatterLazy(const DSceneView& S, const Mat& m, V3 inD, const Surf& s, Rng& g, Counters& c, V3& Wo, V3& Wh, V3& outD, float& pdf, float& sp, bool& exactSp)
{
	if (m.type == MAT_MIRROR) {   // material.h:149-162
		outD = reflect(inD, s.n);
		pdf = 1.0f;
		sp = 1.0f;
		exactSp = false;                      // (a mirror's record is the material alone: FoldLazyVertex reads neither slot nor flag)
		Wo = v3(0.0f, 0.0f, 1.0f); Wh = Wo;   // (LazyVertexSafe passes: the albedo is finite, SceneLazyRefl)
		return;
	}
	RL_WLSTEP(c, 18, 19);
	float roughness = GetRoughness(S, m, s.U, s.V, c);
	V3 N = GetMicrosurfaceNormal(S, m, s, c);
	Wo = WorldToLocal(s, -inD);
	float u0 = Next(g);
	float u1 = Next(g);
	bool bFlip = Wo.z < 0.0f;
	Wh = BeckmannSample(bFlip ? -Wo : Wo, roughness, roughness, u0, u1, c);
	if (bFlip) Wh = -Wh;
	V3 Wi = reflect(-Wo, Wh);
	V3 WiW = LocalToWorld(s, Wi);
	outD = WiW;

	// ScatteringPdf(hit, -inD, WiW), material.cc:352-376
	V3 wo = WorldToLocal(s, -inD);
	V3 wi = WorldToLocal(s, WiW);
#if RL_NORMALIZE_RANGED & 4
	V3 wh = normalize_voted_(wo + wi);   // (arbitrarily short when Wo.Wh is small)
#else
	V3 wh = normalize(wo + wi);
#endif
	if (wh.z < 0.0f) wh.z = -wh.z;
	exactSp = LazyScatterPdf(N, Wo, Wh, wh, roughness, sp, pdf);
}
// May the vertex's reflectance go unevaluated on an unlit path?  refl * 0 * sp / pdf is a zero, and (0 + that) + 0 is +0, only if every component of refl
// and sp are finite (pdf > 0 is the caller's condition for a recorded vertex; a NaN or an infinity in refl makes the reference's sample NaN).  A vertex that
// fails only marks its path lit: the exact evaluation then reproduces whatever the reference does.  All three compares fail on NaN.
// Why passing, with roughness r in [2^-10, 1] and |albedo|, |metallic| <= 16 (SceneLazyRefl), implies a finite ReflFromRecord(Wo, Wh):
//   Wo: camera directions are normalised, a reflection about a unit Wh and the orthonormal frames keep a length to a few ulps, so over at most RL_LAZY_MAX_PATH
//       vertices |Wo|, |Wi| are within 2^-8 of 1.  Wh = +-normalize(-sx, -sy, 1): an infinite, NaN or overflowing slope leaves Wh.z = 0 or NaN and fails the first
//       compare; otherwise Wh is a unit vector to a few ulps, all components finite.
//   F:  |F0| = |0.04 (1 - metallic) + metallic albedo| < 2^9; 1 - |Wh.Wo| lies in [-2^-7, 1] and pow_(x, 5) is defined there, |.| <= 1: |F| < 2^11.
//   G:  GeometryBeckmann is 0, 1 or num / denom with a = rcp1_(r tan(acos(V.z))) < 1.6 (a NaN a compares false and yields 1).  acos_ is 0 or at least 2^-12, and the
//       floats next to pi / 2 and pi keep |tan| within [2^-24, 2^25], so r tan is +0 (a = +inf: 1 is returned) or at least 2^-34 in magnitude: a is finite or +inf,
//       never -inf or the quotient of a -0 (what roughness 0 would give: num = -inf + inf), and aa <= 2^68 does not overflow.  denom = 1 + 2.276 a + 2.577 aa has a
//       negative discriminant: >= 0.49 for every a, so the quotient lies in [-2.5, 1.1].  It is negative only for a < 0, that is V.z <= 0 together with V.Wh > 0
//       (QuotientNotPositive returns 0 first otherwise) -- and then, unless V.z is a zero or rounds to pi / 2's tangent (a = -1 / (r 2.3e7): a quotient within 2^-12 of 0), V.Wh and
//       V.z differ in sign and 0 was returned.  V = Wo: Wo.Wh >= 2^-10, the third compare.  V = Wi: Wi.Wh = Wo.Wh (2 |Wh|^2 - 1) >= 2^-11 as computed.  So both
//       factors lie in [-2^-12, 1.1], 1 + ggx1 ggx2 in [0.99, 2.3], and G = rcp1_ of it in (0.4, 1.02).  (Without the third compare a product of exactly -1 and with it
//       G = inf could not be excluded.)
//   NDF: cosH = |Wh.z| in [2^-10, 1 + 2^-20]; rr in [2^-20, 1]; exp_x in [-2^-19, 2^30], exp_(-exp_x) in [0, 1.01]; denom = pi rr cosH^4 >= 2^-59 is a
//       normal number: 0 <= NDF < 2^60.
//   specular = F G NDF / b with b = 4 |Wi.z| |Wo.z| + 0.001 in [0.001, 4.1]: below 2^11 2^0.1 2^60 2^10 < 2^82; kS specular < 2^93; kD diffuse = (1 - F) albedo
//       (1 - metallic) < 2^21; the sum times |Wi.z| <= 1.01 is finite.
__device__ __forceinline__ bool LazyVertexSafe(V3 Wo, V3 Wh, float sp)
{
	return fabsf(Wh.z) >= 0x1p-10f && fabsf(sp) < INFINITY && dot(Wo, Wh) >= 0x1p-10f;
}
__device__ __forceinline__ bool AnyBitSet(V3 a) { return (__float_as_uint(a.x) | __float_as_uint(a.y) | __float_as_uint(a.z)) != 0u; }
// One step of the fold at a recorded vertex (r0 = Wo, sp slot; r1 = Wh, material index and flag; m = that material): the reflectance, sp and the pdf as Scatter
// computes them from the same values (LazyRecordPdf), the emission (plain scenes: the material's), and the fold's statement exactly as k_trace writes it.
__device__ __forceinline__ V3 FoldLazyVertex(const Mat& m, float4 r0, float4 r1, V3 L)
{
	if (m.type == MAT_MIRROR) {   // refl = albedo, sp = pdf = 1, nothing emitted
		V3 radiance = v3s(0.0f);
		radiance = radiance + m.albedo * L * 1.0f / 1.0f;
		radiance = radiance + v3s(0.0f);
		return radiance;
	}
	const V3 Wo = v3(r0.x, r0.y, r0.z), Wh = v3(r1.x, r1.y, r1.z);
	const V3 N = v3(0.0f, 0.0f, 1.0f);
	const V3 Wi = reflect(-Wo, Wh);
	const float NdotWi = absDot(N, Wi);
	const V3 refl = ReflFromRecord<true>(m.albedo, m.roughness, m.metallic, N, Wo, Wh, Wi, NdotWi);
	float sp, pdf;
	LazyRecordPdf(r0, r1, m.roughness, sp, pdf);
	const V3 E = m.emissive;
	V3 radiance = v3s(0.0f);
	radiance = radiance + refl * L * sp / pdf;
	radiance = radiance + E;
	return radiance;
}

// Miss shader: sky panorama + sun (reference render/renderer.cc:155-199)
// PLAIN: the launch has no sky image (rl_plan.cc), and the panorama lookup is compiled out
template <int STACK, bool PRIMS, bool FULL, int LDS = 0, bool PLAIN = false>
__device__ __forceinline__ V3 MissShader(const DSceneView& S, const SkyRot& R, V3 o, V3 d, float rayTime, float rayTMin, int* stk, Counters& c, const float4* sm = nullptr)
{
	V3 missResult = v3s(0.0f);
	if (!PLAIN && S.sky) {
		V3 dir = normalize(d);
		V3 D = v3(dot(ld3(R.m0), dir), dot(ld3(R.m1), dir), dot(ld3(R.m2), dir));
		float u = rtm::atan2_(D.z, D.x), v = rtm::asin_(D.y);
		u *= 0.1591f; v *= 0.3183f;
		u += 0.5f; v += 0.5f;
		int x = (int)(u * (float)(uint32_t)(S.skyWidth - 1));
		int y = (int)(v * (float)(uint32_t)(S.skyHeight - 1));
		float4 px = ((const float4*)S.sky)[(uint32_t)(y * S.skyWidth + x)];
		c.texels++;
		missResult = missResult + v3(px.x, px.y, px.z);
	}
	if (S.hasSun) {
		HitRec tmp;
		bool occluded;
		if constexpr (LDS != 0) occluded = Traverse4<STACK, true, PRIMS, FULL, LDS, PLAIN>(S, o, -ld3(S.sunDirection), rayTime, rayTMin, tmp, stk, c, sm);
		else occluded = (!PRIMS && (FULL ? (const void*)S.nodes4f : (const void*)S.nodes4)) ? Traverse4<STACK, true, PRIMS, FULL, LDS>(S, o, -ld3(S.sunDirection), rayTime, rayTMin, tmp, stk, c, sm)
		                                           : Traverse<STACK, true, PRIMS>(S, o, -ld3(S.sunDirection), rayTime, rayTMin, tmp, stk, c);
		if (!occluded) missResult = missResult + ld3(S.sunIlluminance);
	}
	return missResult;
}

// sky part of the miss shader (reference render/renderer.cc:155-181)
__device__ __forceinline__ V3 MissSky(const DSceneView& S, const SkyRot& R, V3 d, Counters& c)
{
	V3 missResult = v3s(0.0f);
	if (S.sky) {
		V3 dir = normalize(d);
		V3 D = v3(dot(ld3(R.m0), dir), dot(ld3(R.m1), dir), dot(ld3(R.m2), dir));
		float u = rtm::atan2_(D.z, D.x), v = rtm::asin_(D.y);
		u *= 0.1591f; v *= 0.3183f;
		u += 0.5f; v += 0.5f;
		int x = (int)(u * (float)(uint32_t)(S.skyWidth - 1));
		int y = (int)(v * (float)(uint32_t)(S.skyHeight - 1));
		float4 px = ((const float4*)S.sky)[(uint32_t)(y * S.skyWidth + x)];
		c.texels++;
		missResult = missResult + v3(px.x, px.y, px.z);
	}
	return missResult;
}

} // namespace rl
