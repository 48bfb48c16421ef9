// Device library, part 1 of 6: what every kernel starts from -- the exact-libm tables in LDS, the tunables both megakernels share, the wave vote,
// the device float3, the diagnostic builds' macros, the counters and the RNG.  (Parts: rl_dev_core.h, rl_dev_scene.h, rl_dev_walk.h, rl_dev_shade.h,
// rl_dev_jobs.h, rl_dev_pool.h; each includes what it needs.  The kernels' declarations and instance lists: rl_kernels.h.)
#pragma once

#include <hip/hip_runtime.h>

#include "rl_host.h"
// the exact-libm tables (rl_glibc_math.h) in LDS: 640 B per workgroup, filled by rlm_fill_lds_tables() at the top of every kernel that
// evaluates expf / logf / powf.  A microfacet scattering event makes ~16 such look-ups; from constant memory each one is a gather through
// the vector memory pipeline with a full s_waitcnt behind it.
#ifndef RL_MATH_TABLES_GLOBAL
#define RLM_LDS_TABLES 1
__shared__ double rlm_lds_tab[80];
#define RL_MATH_PROLOGUE() rlm::rlm_fill_lds_tables()
#else
#define RL_MATH_PROLOGUE()
#endif
#include "rl_math.h"
#include "rl_progressive.h"
#include "raylib_amd_rng.h"

#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace rl {

#ifndef RL_POOL_NODEPTR_VGPR
#define RL_POOL_NODEPTR_VGPR 1   /* 298 k-triangle frame 43.0 -> 42.6 ms */
#endif
#ifndef RL_ROOTMISS_RCP
#define RL_ROOTMISS_RCP 1
#endif
#ifndef RL_REFILL_ROUNDS
#define RL_REFILL_ROUNDS 4
#endif
// paths of up to this many vertices fetch all their vertex records before the fold's dependent chain (0: one fetch per step)
#ifndef RL_FOLD_PREFETCH
#define RL_FOLD_PREFETCH 5
#endif
#define RL_LIT_STRIDE (2 * RL_FOLD_PREFETCH + 2)   /* float4 per entry of the lit list (rl_device.h DLitList) */
#ifndef RL_FOLD_PREFETCH_POOL
#define RL_FOLD_PREFETCH_POOL RL_FOLD_PREFETCH
#endif

// The wave's lane mask of a predicate, as the exec-masked compare it is.  HIP's __ballot(int) reaches the same builtin through an int: the compiler
// then materialises the bool as 0 / 1 in a VGPR and compares it with zero again (v_cndmask + v_cmp_ne, 8 issue cycles per ballot on kernels that vote
// several times per traversal step).
__device__ __forceinline__ unsigned long long Ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// ---------------------------------------------------------------------------
// device float3 (reference core/vec3.h conventions; see rl_host.h f3)
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 v3s(float s) { return v3(s, s, s); }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ V3 operator*(V3 a, float t) { return v3(a.x * t, a.y * t, a.z * t); }
__device__ __forceinline__ V3 operator*(float t, V3 a) { return v3(a.x * t, a.y * t, a.z * t); }
__device__ __forceinline__ V3 operator/(V3 a, float t) { return v3(a.x / t, a.y / t, a.z / t); }
__device__ __forceinline__ V3 operator-(V3 a, float t) { return v3(a.x - t, a.y - t, a.z - t); }
__device__ __forceinline__ V3 operator-(float t, V3 a) { return v3(t - a.x, t - a.y, t - a.z); }
__device__ __forceinline__ V3 operator+(V3 a, float t) { return v3(a.x + t, a.y + t, a.z + t); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float absDot(V3 a, V3 b) { return fabsf(a.x * b.x + a.y * b.y + a.z * b.z); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, -(a.x * b.z - a.z * b.x), a.x * b.y - a.y * b.x); }
// (rtm::sqrt_ and rtm::rcp1_ are sqrtf and 1.0f / x bit for bit: rl_math.h)
__device__ __forceinline__ float length(V3 a) { return rtm::sqrt_(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ V3 normalize(V3 a) { float k = rtm::rcp1_(length(a)); return v3(a.x * k, a.y * k, a.z * k); }
// ---- normalize without the two range guards (RL_NORMALIZE_RANGED) ----
// A translation unit's setting, made before its includes as RL_SAMPLER_RANGED is; off by default, and only the lazy instance's unit turns it on
// (rl_render_lazy.hip).  normalize pays sqrt_'s guard and rcp1_'s for one fact about one float, len2.  Bits, so that the groups can be built apart:
//   1: the surface frame (BuildSurface), 2: the sampler's two normalisations (BeckmannSample), 4: the recomputed half vector (ScatterLazy),
//   8: the single-float sites -- SinThetaL's root and the root inside the ranged prologue's acos_ (rl_dev_shade.h).
// (A definition on the compiler's command line reaches every unit: that is for `make variant` experiments, whose other kernels are then not the product's.)
#ifndef RL_NORMALIZE_RANGED
#define RL_NORMALIZE_RANGED 0
#endif
// 2^-101 <= len2 <= FLT_MAX: sqrt_in_range_'s domain.  The root then lies in [2^-50.5, 2^64], inside rcp1_in_range_'s [2^-126, 2^126): one condition for both.
// False on a zero, a subnormal, a negative number, an infinity and NaN.
__device__ __forceinline__ bool NormalizeInRange(float len2) { return (__float_as_uint(len2) - 0x0d000000u) < (0x7f800000u - 0x0d000000u); }
// normalize's statements with neither guard: the same bits for NormalizeInRange(dot(a, a)), the caller's to guarantee
__device__ __forceinline__ V3 normalize_ranged_(V3 a)
{
	float k = rlm::rcp1_in_range_(rtm::sqrt_in_range_(a.x * a.x + a.y * a.y + a.z * a.z));
	return v3(a.x * k, a.y * k, a.z * k);
}
// normalize for a length of unknown range: if any lane's len2 is out of range the whole wave runs normalize, otherwise the ranged form (DivSpecular's pattern: one
// scalar branch, no exec-mask region).  Nothing to prove about the bits: both short sequences equal sqrtf and 1.0f / x on their domains for every bit pattern
// (RaylibAMD_VerifyExactMath, RaylibAMD_VerifyNormalizeRanged mode 0), so an in-range lane gets the same value from either side.
__device__ __forceinline__ V3 normalize_voted_(V3 a)
{
	if (rtm::wave_any_(!NormalizeInRange(a.x * a.x + a.y * a.y + a.z * a.z))) return normalize(a);
	return normalize_ranged_(a);
}
// sqrt_ of one float, voted the same way
__device__ __forceinline__ float sqrt_voted_(float x)
{
	if (rtm::wave_any_(!NormalizeInRange(x))) return rtm::sqrt_(x);
	return rtm::sqrt_in_range_(x);
}
__device__ __forceinline__ V3 reflect(V3 v, V3 n) { return v - 2.0f * dot(v, n) * n; }
__device__ __forceinline__ V3 mix(V3 a, V3 b, float t) { return (1.0f - t) * a + t * b; }
__device__ __forceinline__ V3 ld3(const float* p) { return v3(p[0], p[1], p[2]); }
__device__ __forceinline__ bool isZero(V3 a) { return a.x == 0.0f && a.y == 0.0f && a.z == 0.0f; }

#define RL_PI 3.14159265359f   /* BRDF::PI, reference render/brdf.h:8 */

// diagnostic build (-DRL_DIAG_TIMELINE=1, RAYLIB_PRINT_STAMPS=1): k_trace's waves record when they start, when they first find the
// job queue empty and when they end (s_memrealtime, 100 MHz), three arrays of 8192 slots behind the counters
#ifdef RL_DIAG_TIMELINE
#define RL_TIMELINE_SLOTS (4 * 8192)   /* start | job list seen empty | end | XCC id */
#define RL_TIMELINE(which) { if (lane == 0 && (gtid >> 6) < 8192u) { countersK[CNT_COUNT + 24 + (which) * 8192 + (gtid >> 6)] = __builtin_amdgcn_s_memrealtime(); if ((which) == 0) countersK[CNT_COUNT + 24 + 3 * 8192 + (gtid >> 6)] = XccId(); } }
#else
#define RL_TIMELINE_SLOTS 0
#define RL_TIMELINE(which)
#endif
// behind everything else in the counter block: the lazy instance's lit paths (list entries + folds in place) and, of them, the folds in place
#define RL_CNT_LIT (CNT_COUNT + 24 + RL_TIMELINE_SLOTS)
#define RL_CNT_BLOCK (RL_CNT_LIT + 2)   /* counters in the block */
#ifdef RL_DIAG_STAMPS
#define RL_DIAG_BIND(c) { (c).diag = nullptr; (c).tLast = 0; (c).tAcc[0] = (c).tAcc[1] = (c).tAcc[2] = (c).tAcc[3] = 0; }
#else
#define RL_DIAG_BIND(c)
#endif
struct Counters {
	uint32_t rays, nodes, tris, shaded, texels, samples, trips;
#ifdef RL_DIAG_STAMPS
	unsigned long long* diag;   // diagnostic build: the global counter array (slots CNT_COUNT + k)
	unsigned long long tLast, tAcc[4];
#endif
};
#ifdef RL_DIAG_STAMPS
#define RL_CSTAMP_BEGIN(c) { __builtin_amdgcn_sched_barrier(0); (c).tLast = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#define RL_CSTAMP(c, k) { __builtin_amdgcn_sched_barrier(0); const unsigned long long now_ = __builtin_amdgcn_s_memtime(); (c).tAcc[k] += now_ - (c).tLast; (c).tLast = now_; __builtin_amdgcn_sched_barrier(0); }
#if RL_DIAG_STAMPS >= 2   /* wave-step against lane-step counts: global atomics in the inner loops, they distort the clock shares */
#define RL_WLSTEP(c, kw, kl) { const unsigned long long em_ = Ballot(1); if ((c).diag && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)em_) - 1u) { atomicAdd(&(c).diag[CNT_COUNT + kw], 1ull); atomicAdd(&(c).diag[CNT_COUNT + kl], (unsigned long long)__popcll(em_)); } }
#else
#define RL_WLSTEP(c, kw, kl)
#endif
#else
#define RL_WLSTEP(c, kw, kl)
#define RL_CSTAMP_BEGIN(c)
#define RL_CSTAMP(c, k)
#endif

// ---------------------------------------------------------------------------
// RNG (include/raylib_amd_rng.h); draws in the reference's program order.
struct Rng { RaylibRngStream s; };
__device__ __forceinline__ float Next(Rng& g) { return raylib_rng_next_float(&g.s); }

// reference core/random.cc:3-23
__device__ __forceinline__ V3 RandomInUnitSphere(Rng& g)
{
	float u1 = Next(g);
	float u2 = Next(g);
	float z = 1.0f - 2.0f * u1;
	float r = rtm::sqrt_(fmaxf(0.0f, 1.0f - z * z));
	float phi = 2.0f * 3.141592f * u2;
	float sn, cs; rtm::sincos_(phi, &sn, &cs);
	return v3(r * cs, r * sn, z);
}
// reference core/random.cc:42-50
__device__ __forceinline__ V3 RandomInUnitDisk(Rng& g)
{
	float u1 = Next(g);
	float u2 = Next(g);
	float r = rtm::sqrt_(u1);
	float theta = 2.0f * 3.14159265358979323846f * u2;
	float sn, cs; rtm::sincos_(theta, &sn, &cs);
	return v3(r * cs, r * sn, 0.0f);
}

} // namespace rl
