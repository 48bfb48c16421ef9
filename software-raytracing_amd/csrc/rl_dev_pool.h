// Device library, part 6 of 6: the pool schedule's resumable walk -- the slot states, Trav, single node and leaf steps on the three trees, the
// path fold and the pool kernel's occupancy.  k_trace_pool (rl_k_trace_pool.inl) and the 8-wide ray query (rl_k_query.inl) are built from these.
#pragma once

#include "rl_dev_walk.h"

namespace rl {

// ---------------------------------------------------------------------------
// The pool megakernel.  Same job queue, same per-path arithmetic and the same outputs as k_trace, but a wave
// no longer runs "one ray per lane per trip".  Each wave owns a POOL of 64*K paths:
//   - the per-ray data the traversal needs (origin, direction, time) and gives back (t, primitive, barycentrics)
//     sit in LDS, one column per pool slot;
//   - the rest of a path (RNG state, output index, depth) stays in the registers of the slot's HOME lane
//     (slot = p*64 + lane), its vertex records in the global path stack.
// A trip is: refill the free slots (wave64 ballot + prefix ranks, compacted: up to 64 new camera rays are generated
// by the low lanes and dealt to the free slots through LDS), then ONE traversal phase over the whole pool, then K
// shading passes.  In the traversal phase a lane takes the next un-traced slot from the pool whenever it has
// finished its ray ("dynamic fetch"; the ray's home lane is irrelevant), so a wave's traversal time is the
// SUM of its rays' steps / 64 plus a tail, instead of the MAX over lanes per bounce.  The sun query of the miss
// shader (renderer.cc:192-197) goes through the pool like any other ray instead of being traced inline by the few
// lanes that missed.
enum { F_OX = 0, F_OY, F_OZ, F_DX, F_DY, F_DZ, F_T, F_TRI, F_A, F_B, F_TIME, F_COUNT };   // F_TIME only exists in scenes with moving primitives (PRIMS)
#define Q_CLOSEST  (-1)   /* F_TRI before traversal: closest-hit query; after: missed everything */
#define Q_SHADOW   (-2)   /* before: occlusion query towards the sun (sky part parked in F_D*); after: not occluded */
#define Q_EMPTY    (-3)   /* no path in this slot */
#define Q_OCCLUDED (-4)   /* after a Q_SHADOW query: something is in the way */
#define Q_PENDING  (-5)   /* a lane is tracing this slot's closest-hit query (it may take more than one trip) */
#define Q_PENDING_SHADOW (-6)
#define Q_MISS     (-7)   /* result of a closest-hit query that hit nothing (distinct from Q_CLOSEST: a straggler may deliver it while the next phase is handing out slots) */
#define Q_CLEAR    (-8)   /* result of a sun query: nothing in the way */
#define RL_POOL_WIDEN RL_BOX_WIDEN
#ifndef RL_POOL_MAXBLOCKS
#define RL_POOL_MAXBLOCKS 4   /* workgroups per CU the pool kernel is compiled for (register budget 512 / (4 * blocks) per lane) */
#endif
// Re-tuned in round 2 on the grid nodes (tools/gpu_variants.py, tools/gpu_scenes_time.py; 40 / 40 / 52 before): 298 k scene 51.9 ->
// 50.9 ms, colonnade 481 -> 471 ms, 2.36 M 156 -> 154 ms, 10.1 M 463 -> 460 ms.  (Cut 24: colonnade 458 but 2.36 M 159; cut 16: 459 / 163.)
#ifndef RL_POOL_CUT_EXH
#define RL_POOL_CUT_EXH 32   /* the same once the job queue is empty */
#endif
#ifndef RL_POOL_CUT
#define RL_POOL_CUT 32    /* with the pool handed out: shade once no more than this many lanes still traverse */
#endif
#ifndef RL_POOL_WNODE
#define RL_POOL_WNODE 4   /* relative cost of a node step and a primitive step in the vote */
#define RL_POOL_WLEAF 5
#endif
#ifndef RL_POOL_WNODE4
#define RL_POOL_WNODE4 4  /* the same for a BVH4 step */
#endif
#ifndef RL_POOL_WNODE8
#define RL_POOL_WNODE8 4  /* ... and for a step on the 8-wide tree */
#endif
#ifndef RL_POOL_BOTH8
#define RL_POOL_BOTH8 0
#endif
#ifndef RL_POOL_SHADE_MIN
// Hits wait in their pool slots until a shading round is worth running.  Until round 5 that meant a full wave of 64: the material code then always ran with every lane, and on
// average half a round's worth of finished hits -- a quarter of the pool's 128 slots -- sat parked instead of holding rays for the traversal phase, whose lanes run
// dry towards its end.  From 32 waiting hits on a round runs at once: 298 k room from inside 88.3 -> 85.5 ms, from outside 34.9 -> 33.8, colonnade 375.6 -> 363.6,
// 2.36 M 97.4 -> 94.5, 10.1 M 271.1 -> 267.2, textured room 102.0 -> 98.1 (thresholds 8 ... 48 are within 0.5 % of each other; profiles/r05_shade_min_ab.log).
#define RL_POOL_SHADE_MIN 32
#endif
#ifndef RL_POOL_WLEAF8
#define RL_POOL_WLEAF8 12   /* 298 k-triangle room from inside: 6 -> 365.7 ms, 9 -> 358.9, 12 -> 357.8, 16 -> 360.9 (the 4-wide tree: 381.4) */
#endif
#ifndef RL_POOL_WLEAF4
// Re-tuned at the end of round 3 (the leaf step is a third cheaper than it was -- two divisions gone, the own-box rule on v_max / v_min -- but above all the lanes at
// leaves are the ones about to FINISH: serving them first frees lanes for the next fetch).  298 k frame / colonnade / 2.36 M triangles at 4K, ms: 5 -> 36.85 / 373.7 /
// 114.2; 7 -> 36.0 / 372.9 / --; 8 -> 35.87 / 374.1 / 109.9; 10 -> 35.64 / 377.4 / 108.5; 12 -> 35.6 / -- / --; 16 -> 35.85 / 390.4 / 107.5.
#define RL_POOL_WLEAF4 8
#endif
#ifndef RL_POOL_KEEP
#define RL_POOL_KEEP 58   /* leave the traversal loop to fetch new rays when no more than this many lanes still traverse */
#endif


struct Trav {
	V3 o, d, inv; float rayTime; bool nx, ny, nz, anyhit; HitRec best; int cur, sp, leafI;
	// the 8-wide tree's walk (NodeStep8 / LeafStep8): the hit inner children of a node still to be visited, as ONE group -- gx the node's childBase, gy = their bits
	// in VISITING order (bit 24 + (slot XOR oct), highest first) | the node's alphaMask << 8 | its imask --; the triangles of its hit leaf children still to be tested:
	// tx the node's triBase, tz its leafMask, ty the bits of tz that are left; oct: bit 0 / 1 / 2 set when the ray travels towards +x / +y / +z
	uint32_t gx, gy, tx, ty, tz, oct;
	// ... and per axis all ones where the ray travels in the negative direction (NodeStep8 selects a node's near / far planes with them)
	uint32_t m8x, m8y, m8z;
};

// Single steps on the resumable state, for the vote-driven loop of k_trace_pool: a lane is either at an inner node
// (cur >= 0), at a leaf (cur < 0, leafI = next primitive of it), or finished (both return true then).
// LSTACK entries of the traversal stack live in LDS (stk), deeper ones in the lane's private overflow array (scratch):
// with a 19-entry LDS part a 32-deep stack fits 4 workgroups per CU; trees rarely need the overflow.
// (Round 3, measured and not kept: a 16-bit entry distance beside every stack entry, so that a pop drops the entries that start behind the best hit without
// fetching their node.  It drops next to nothing -- 6.8 node records per ray instead of 6.9 on the 298 k-triangle scene: the near-first walk with its
// shrinking t leaves little behind -- and the column costs LDS stack depth (12 entries instead of 18): 51.6 ms against 44.7.)
template <int LSTACK, int STACK>
__device__ __forceinline__ void StackPush(Trav& T, int* stk, int* ovf, int v)
{
	if (T.sp < LSTACK) { stk[T.sp * RL_BLOCK] = v; ++T.sp; }
	else if (LSTACK < STACK && T.sp < STACK) { ovf[T.sp - LSTACK] = v; ++T.sp; }
}
#ifndef RL_POP_SPLIT
#define RL_POP_SPLIT 0
#endif
template <int LSTACK, int STACK>
__device__ __forceinline__ bool PopOrFinish(Trav& T, int* stk, int* ovf)
{
	if (T.sp == 0) return true;
	--T.sp;
	// (The compiler sinks the two loads, one from scratch and one from LDS, into ONE flat_load through a selected pointer.  RL_POP_SPLIT keeps them apart --
	//  measured: the colonnade hall, whose rays live above the LDS part of the stack, 402 ms against 377: two divergent arms cost more than the flat load.)
#if RL_POP_SPLIT
	int v;
	if (LSTACK < STACK && T.sp >= LSTACK) { v = ovf[T.sp - LSTACK]; asm volatile("" : "+v"(v)); }
	else v = stk[T.sp * RL_BLOCK];
	T.cur = v;
#else
	T.cur = (LSTACK < STACK && T.sp >= LSTACK) ? ovf[T.sp - LSTACK] : stk[T.sp * RL_BLOCK];
#endif
	T.leafI = 0;
	return false;
}
// min(t, FLT_MAX) for a t that is never NaN (a hit distance, or +inf): one integer minimum on the bit patterns -- floats below FLT_MAX, negative ones
// included, are below 0x7f7fffff as signed integers too -- where fminf costs the compiler's canonicalising v_max t, t in front of the v_min
__device__ __forceinline__ float ClampToFltMax(float t) { return __int_as_float(min(__float_as_int(t), 0x7f7fffff)); }
template <int LSTACK, int STACK>
__device__ __forceinline__ bool NodeStep(const DSceneView& S, Trav& T, float tMin, int* stk, int* ovf, Counters& c)
{
	RL_WSTEP(4);
	const float4* np = (const float4*)(S.nodes + T.cur);
	const float4 q0 = np[0], q1 = np[1], q2 = np[2];
	const int4 k = ((const int4*)np)[3];
	c.nodes++;
	float tl, tr;
	const float tmx = ClampToFltMax(T.best.t);
	bool hl = Slab(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, T.o, T.inv, T.nx, T.ny, T.nz, tMin, tmx, tl, RL_POOL_WIDEN);
	bool hr = Slab(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, T.o, T.inv, T.nx, T.ny, T.nz, tMin, tmx, tr, RL_POOL_WIDEN);
	hl = hl && (k.x != DNODE_EMPTY);
	hr = hr && (k.y != DNODE_EMPTY);
	T.leafI = 0;
	if (hl && hr) {
		const bool leftFirst = tl <= tr;
		const int nearC = leftFirst ? k.x : k.y, farC = leftFirst ? k.y : k.x;
		StackPush<LSTACK, STACK>(T, stk, ovf, farC);
		T.cur = nearC;
		return false;
	}
	if (hl) { T.cur = k.x; return false; }
	if (hr) { T.cur = k.y; return false; }
	return PopOrFinish<LSTACK, STACK>(T, stk, ovf);
}
// One step on the BVH4 (grid nodes, DNode4Q, 64 B): four slab tests, the hit children ordered by entry distance (5-comparator network),
// the nearest followed, the others pushed far-to-near.
template <int LSTACK, int STACK>
__device__ __forceinline__ bool NodeStep4(const DSceneView& S, Trav& T, float tMin, int* stk, int* ovf, Counters& c)
{
	RL_WSTEP(4);
	c.nodes += 1;   // 64-byte records fetched
	const float tmx = ClampToFltMax(T.best.t);
	RL_WIDE_STEP_Q(S, T.cur, T.o, T.inv, T.nx, T.ny, T.nz, tMin, tmx, RL_POOL_WIDEN, t0, t1, t2, t3, ch)   // T.inv was clamped when the ray was fetched
	int r0 = ch.x, r1 = ch.y, r2 = ch.z, r3 = ch.w;
	if (r0 == DNODE_EMPTY) t0 = INFINITY;
	if (r1 == DNODE_EMPTY) t1 = INFINITY;
	if (r2 == DNODE_EMPTY) t2 = INFINITY;
	if (r3 == DNODE_EMPTY) t3 = INFINITY;
	RL_SORT4(t0, r0, t1, r1, t2, r2, t3, r3)
	T.leafI = 0;
	if (!(t0 < INFINITY)) return PopOrFinish<LSTACK, STACK>(T, stk, ovf);
	if (t3 < INFINITY) StackPush<LSTACK, STACK>(T, stk, ovf, r3);
	if (t2 < INFINITY) StackPush<LSTACK, STACK>(T, stk, ovf, r2);
	if (t1 < INFINITY) StackPush<LSTACK, STACK>(T, stk, ovf, r1);
	T.cur = r0;
	return false;
}

template <int LSTACK, int STACK, bool PRIMS>
__device__ __forceinline__ bool LeafStep(const DSceneView& S, Trav& T, float tMin, int* stk, int* ovf, Counters& c)
{
	RL_WSTEP(5);
	const LeafRef L = DecodeLeaf(T.cur);
	const V3 o = T.o, d = T.d;
	c.tris++;
	if (!PRIMS || L.kind == 0u) {
		const int i = L.first + T.leafI;
		const Tri TT = LoadTri(S, i);
		RL_TRIANGLE_TEST(S, TT, i, o, d, tMin, T.best, L.alpha, OwnBoxPass(TT.v0, TT.v1, TT.v2, o, ExactInv(d), tMin, t), T.anyhit, c, RL_NESTED)
	} else RL_PRIMITIVE_LEAF(S, L.kind, L.first, o, d, T.rayTime, tMin, T.best, T.anyhit, false, FLT_MAX)
	if (++T.leafI < L.count) return false;
	return PopOrFinish<LSTACK, STACK>(T, stk, ovf);
}

// ---- the 8-wide tree (DNode8, rl_device.h) in the vote-driven loop --------------------------------------------------------------------------------
// A lane's state is (T.gx, T.gy): the group of hit inner children it is working through, (T.tx, T.ty, T.tz): the triangles of hit leaf children it still has
// to test, and a stack of groups (two words each: the LDS stack's entries pairwise, then the private overflow).  T.cur only says which party of the vote the
// lane belongs to: 0 at a node (a group with a child left), -1 at a leaf (a triangle left), TRAV-idle without a ray.  One node step = take the group's next
// child in visiting order, push the rest of the group (ONE entry however many children it holds), fetch the child (five 16-byte loads), test its eight boxes,
// and turn the hits into the next group and the next triangles -- no sort, no per-child pushes.  The triangles of a node's leaf children are tested before any
// of its inner children is entered (they are the geometry nearest to hand); the order of two candidates never decides a hit (candidate rule, tie rule).
// T.gy = the group's bits in VISITING order (bit 24 + (slot XOR oct), highest first) | the node's imask; T.ty = the hit leaf children (bits 0 - 7, slot order) |
// the next triangle of the lowest of them (bits 8 - 9) | the node's alphaMask << 16; T.tx / T.tz = the node's triBase / leafMask.
__device__ __forceinline__ void Push8(Trav& T, int* stk, int* ovf, const int G, const int GMAX)
{
	if (T.sp < G) { stk[(2 * T.sp) * RL_BLOCK] = (int)T.gx; stk[(2 * T.sp + 1) * RL_BLOCK] = (int)T.gy; ++T.sp; }
	else if (T.sp < GMAX) { ovf[2 * (T.sp - G)] = (int)T.gx; ovf[2 * (T.sp - G) + 1] = (int)T.gy; ++T.sp; }   // (GMAX = RL_POOL8_MAXLEVELS: the host selects this walk only for trees of at most that many levels, rl_plan.cc)
}
// what comes next for a lane whose triangles are done: the rest of its group, else the stack's top group, else nothing (true: the ray is finished)
__device__ __forceinline__ bool Next8(Trav& T, int* stk, int* ovf, const int G)
{
	if ((T.ty & 0xffu) != 0u) { T.cur = -1; return false; }
	if ((T.gy >> 24) != 0u) { T.cur = 0; return false; }
	if (T.sp == 0) return true;
	--T.sp;
	if (T.sp < G) { T.gx = (uint32_t)stk[(2 * T.sp) * RL_BLOCK]; T.gy = (uint32_t)stk[(2 * T.sp + 1) * RL_BLOCK]; }
	else { T.gx = (uint32_t)ovf[2 * (T.sp - G)]; T.gy = (uint32_t)ovf[2 * (T.sp - G) + 1]; }
	T.cur = 0;
	return false;
}
// a ray's constants for this walk: the octant (visiting order = slot XOR oct) and, per axis, all ones where the ray travels in the negative direction -- the
// near planes of a node are then (upper & m) | (lower & ~m): one v_bitop3_b32, 2 issue clocks, where a v_cndmask on a lane mask in SGPRs takes 4
__device__ __forceinline__ void RaySetup8(Trav& T)
{
	T.m8x = T.inv.x < 0.0f ? 0xffffffffu : 0u; T.m8y = T.inv.y < 0.0f ? 0xffffffffu : 0u; T.m8z = T.inv.z < 0.0f ? 0xffffffffu : 0u;
	T.oct = (T.inv.x < 0.0f ? 0u : 1u) | (T.inv.y < 0.0f ? 0u : 2u) | (T.inv.z < 0.0f ? 0u : 4u);
}
// One child: six planes, the NEGATED entry distance = min of the negated near distances (fma(q, -A, -(B - E)): the modifier is free), exit = min of the far ones,
// and "culled" (exit * widen < entry in real arithmetic) as the SIGN of fma(exit, widen, -entry) -- with the entry negated the widening is the instruction's literal
// (v_fmac with a constant: 2 issue clocks; round 4's fma(exit, widen, -entry) held the constant in an SGPR: 4) -- shifted into a mask with one v_alignbit.
#define RL_QSLAB8(wn, wf, sh) { \
	const float nx_ = __builtin_fmaf((float)((nX##wn >> sh) & 0xffu), -Ax_, nBx_), fx_ = __builtin_fmaf((float)((fX##wf >> sh) & 0xffu), Ax_, Bfx_); \
	const float ny_ = __builtin_fmaf((float)((nY##wn >> sh) & 0xffu), -Ay_, nBy_), fy_ = __builtin_fmaf((float)((fY##wf >> sh) & 0xffu), Ay_, Bfy_); \
	const float nz_ = __builtin_fmaf((float)((nZ##wn >> sh) & 0xffu), -Az_, nBz_), fz_ = __builtin_fmaf((float)((fZ##wf >> sh) & 0xffu), Az_, Bfz_); \
	const float ntn_ = fminf(ntMin_, __builtin_fminf(__builtin_fminf(nx_, ny_), nz_)), tf_ = fminf(tmxL_, __builtin_fminf(__builtin_fminf(fx_, fy_), fz_)); \
	culled = __builtin_amdgcn_alignbit(culled, __float_as_uint(__builtin_fmaf(tf_, RL_POOL_WIDEN, ntn_)), 31u); }
#define RL_SEL8(hi_, lo_, m_) __builtin_amdgcn_bitop3_b32((hi_), (lo_), (m_), 0xE4)   /* (hi & m) | (lo & ~m): truth table over (hi, lo, m) */
__device__ __forceinline__ bool NodeStep8(const DSceneView& S, Trav& T, float tMin, int* stk, int* ovf, Counters& c, const unsigned char* perm, const uint4* top, const int G, const int GMAX)
{
	RL_WSTEP(4);
	c.nodes++;   // one 80-byte record
	// the group's next child in visiting order; the rest of the group, if any, is one stack entry
	const uint32_t pos = 31u - (uint32_t)__clz((int)T.gy);
	T.gy &= ~(1u << pos);
	const uint32_t slot = (pos - 24u) ^ T.oct;
	const uint32_t node = T.gx + (uint32_t)__popc(T.gy & 0xffu & ((1u << slot) - 1u));
	if ((T.gy >> 24) != 0u) Push8(T, stk, ovf, G, GMAX);
#ifdef RL_DIAG_TOPN   /* which nodes the steps go to (breadth-first numbers: a prefix is the top of the tree) and how many groups the stack holds: what an LDS copy of the top serves */
	if (c.diag) {
		const uint32_t lim_[8] = { 9u, 22u, 53u, 73u, 128u, 256u, 1024u, 0xffffffffu };
		uint32_t lo_ = 0;
		for (int b_ = 0; b_ < 8; ++b_) { const unsigned long long m_ = Ballot(node >= lo_ && node < lim_[b_]); if (m_ && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)Ballot(1)) - 1u) atomicAdd(&c.diag[CNT_COUNT + 4 + b_], (unsigned long long)__popcll(m_)); lo_ = lim_[b_]; }
		const uint32_t dl_[8] = { 1u, 2u, 3u, 4u, 5u, 6u, 8u, 0xffffffffu };
		lo_ = 0;
		for (int b_ = 0; b_ < 8; ++b_) { const unsigned long long m_ = Ballot((uint32_t)T.sp >= lo_ && (uint32_t)T.sp < dl_[b_]); if (m_ && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)Ballot(1)) - 1u) atomicAdd(&c.diag[CNT_COUNT + 16 + b_], (unsigned long long)__popcll(m_)); lo_ = dl_[b_]; }
	}
#endif
	// five 16-byte rows from global memory: the base is the kernel's (uniform), the offset 32-bit -- global_load with an SGPR base.  (RL_TOP8_NODES > 0, an
	// experiment: the first nodes -- breadth first, the top of the tree -- from the workgroup's LDS copy: rl_device.h.)
	const uint32_t at_ = node * 80u;
	uint4 h_, k_, p0_, p1_, p2_;
#if RL_TOP8_NODES > 0
	if (node < (uint32_t)RL_TOP8_NODES) {
		const char* lp_ = (const char*)top + at_;
		h_ = *(const uint4*)(lp_); k_ = *(const uint4*)(lp_ + 16); p0_ = *(const uint4*)(lp_ + 32); p1_ = *(const uint4*)(lp_ + 48); p2_ = *(const uint4*)(lp_ + 64);
	} else
#endif
	{
		(void)top;
		const char* np_ = (const char*)S.nodes8 + at_;
		h_ = GLoadU4(np_, 0); k_ = GLoadU4(np_, 1); p0_ = GLoadU4(np_, 2); p1_ = GLoadU4(np_, 3); p2_ = GLoadU4(np_, 4);
	}
	const float Ax_ = __uint_as_float((h_.w & 0xffu) << 23) * T.inv.x, Ay_ = __uint_as_float(((h_.w >> 8) & 0xffu) << 23) * T.inv.y, Az_ = __uint_as_float(((h_.w >> 16) & 0xffu) << 23) * T.inv.z;
	const float Bx_ = (__uint_as_float(h_.x) - T.o.x) * T.inv.x, By_ = (__uint_as_float(h_.y) - T.o.y) * T.inv.y, Bz_ = (__uint_as_float(h_.z) - T.o.z) * T.inv.z;
	const float Ex_ = RL_GRID_ERR(Ax_, Bx_), Ey_ = RL_GRID_ERR(Ay_, By_), Ez_ = RL_GRID_ERR(Az_, Bz_);   // -(B - E) and B + E below
	const float nBx_ = Ex_ - Bx_, Bfx_ = Bx_ + Ex_, nBy_ = Ey_ - By_, Bfy_ = By_ + Ey_, nBz_ = Ez_ - Bz_, Bfz_ = Bz_ + Ez_;
	// planes: p0 = qlo x (children 0-3, 4-7), qlo y (0-3, 4-7); p1 = qlo z (0-3, 4-7), qhi x (0-3, 4-7); p2 = qhi y (0-3, 4-7), qhi z (0-3, 4-7)
	const uint32_t nX0 = RL_SEL8(p1_.z, p0_.x, T.m8x), fX0 = RL_SEL8(p0_.x, p1_.z, T.m8x), nX1 = RL_SEL8(p1_.w, p0_.y, T.m8x), fX1 = RL_SEL8(p0_.y, p1_.w, T.m8x);
	const uint32_t nY0 = RL_SEL8(p2_.x, p0_.z, T.m8y), fY0 = RL_SEL8(p0_.z, p2_.x, T.m8y), nY1 = RL_SEL8(p2_.y, p0_.w, T.m8y), fY1 = RL_SEL8(p0_.w, p2_.y, T.m8y);
	const uint32_t nZ0 = RL_SEL8(p2_.z, p1_.x, T.m8z), fZ0 = RL_SEL8(p1_.x, p2_.z, T.m8z), nZ1 = RL_SEL8(p2_.w, p1_.y, T.m8z), fZ1 = RL_SEL8(p1_.y, p2_.w, T.m8z);
	const float ntMin_ = -tMin, tmxL_ = ClampToFltMax(T.best.t);
	uint32_t culled = 0u;   // child 7 first: child c ends up in bit c
	RL_QSLAB8(1, 1, 24) RL_QSLAB8(1, 1, 16) RL_QSLAB8(1, 1, 8) RL_QSLAB8(1, 1, 0)
	RL_QSLAB8(0, 0, 24) RL_QSLAB8(0, 0, 16) RL_QSLAB8(0, 0, 8) RL_QSLAB8(0, 0, 0)
	const uint32_t hitSlot = ~culled & 0xffu;
	// hits -> the next group (inner children, bits moved to visiting order by the workgroup's 8 x 256 table) and the next triangles (leaf children: their bits as
	// they are -- LeafStep8 works out which triangle a bit stands for; round 4 spread every bit into a nibble here, ten instructions on every node step)
	const uint32_t imask = h_.w >> 24;
	const uint32_t innerP = (uint32_t)perm[T.oct * 256u + (hitSlot & imask)];
	T.gx = k_.x; T.gy = (innerP << 24) | imask;
	T.tx = k_.y; T.tz = k_.z; T.ty = (hitSlot & ~imask) | ((k_.w & 0xffu) << 16);
	return Next8(T, stk, ovf, G);
}
template <bool PRIMS>
__device__ __forceinline__ bool LeafStep8(const DSceneView& S, Trav& T, float tMin, int* stk, int* ovf, Counters& c, const int G)
{
	RL_WSTEP(5);
	// the lowest hit leaf child, its next triangle (the children's triangles are consecutive slots: triBase + the bits of leafMask below)
	const uint32_t lc = (uint32_t)__ffs((int)(T.ty & 0xffu)) - 1u;
	const uint32_t k = (T.ty >> 8) & 3u;
	const uint32_t nib = (T.tz >> (4u * lc)) & 15u;
	const int i = (int)(T.tx + (uint32_t)__popc(T.tz & ((1u << (4u * lc)) - 1u)) + k);
	const bool alpha = ((T.ty >> (16u + lc)) & 1u) != 0u;
	if ((nib >> (k + 1u)) != 0u) T.ty += 0x100u;                       // the child has another triangle
	else { T.ty &= ~0x300u; T.ty &= T.ty - 1u; }                       // next child (the lowest set bit is a child's: bits 8 - 9 are clear)
	const V3 o = T.o, d = T.d;
	c.tris++;
	const Tri TT = LoadTri(S, i);
	RL_TRIANGLE_TEST(S, TT, i, o, d, tMin, T.best, alpha, OwnBoxPass(TT.v0, TT.v1, TT.v2, o, ExactInv(d), tMin, t), T.anyhit, c, RL_NESTED)
	return Next8(T, stk, ovf, G);
}

// Radiance folded from the last vertex back to the camera: radiance = (0 + refl*Li*sp/pdf) + E at every vertex,
// in the reference's operation order (renderer.cc:139-151).
__device__ __forceinline__ V3 FoldPath(const float* __restrict__ pathStack, uint32_t stackStride, uint32_t home, int depth, V3 L)
{
#if RL_FOLD_PREFETCH_POOL > 0
	if (depth <= RL_FOLD_PREFETCH_POOL) {
		float4 q0[RL_FOLD_PREFETCH_POOL], q1[RL_FOLD_PREFETCH_POOL];
		#pragma unroll
		for (int k = 0; k < RL_FOLD_PREFETCH_POOL; ++k) {
			const int kk = k < depth ? k : 0;
			const float4* rec = (const float4*)pathStack + ((size_t)kk * stackStride + home) * 2u;
			q0[k] = rec[0]; q1[k] = rec[1];
		}
		#pragma unroll
		for (int k = RL_FOLD_PREFETCH_POOL - 1; k >= 0; --k) {
			if (k < depth) {
				const V3 refl = v3(q0[k].x, q0[k].y, q0[k].z);
				const float sp = q0[k].w, pdf = q1[k].x;
				const V3 E = v3(q1[k].y, q1[k].z, q1[k].w);
				V3 radiance = v3s(0.0f);
				radiance = radiance + refl * L * sp / pdf;
				radiance = radiance + E;
				L = radiance;
			}
		}
		return L;
	}
#endif
	for (int k = depth - 1; k >= 0; --k) {
		const float4* rec = (const float4*)pathStack + ((size_t)k * stackStride + home) * 2u;
		const float4 r0 = rec[0], r1 = rec[1];
		const V3 refl = v3(r0.x, r0.y, r0.z);
		const float sp = r0.w, pdf = r1.x;
		const V3 E = v3(r1.y, r1.z, r1.w);
		V3 radiance = v3s(0.0f);
		radiance = radiance + refl * L * sp / pdf;
		radiance = radiance + E;
		L = radiance;
	}
	return L;
}

template <int LSTACK, bool PRIMS, int K> struct PoolOcc {
	static constexpr int kFields = PRIMS ? F_COUNT : F_COUNT - 1;
	static constexpr int kLdsPerBlock = LSTACK * RL_BLOCK * 4 + (RL_BLOCK / 64) * (kFields * 64 * K * 4 + 64 * K);
	static constexpr int kFit = (160 * 1024) / kLdsPerBlock;
	static constexpr int kBlocks = kFit < 1 ? 1 : (kFit > RL_POOL_MAXBLOCKS ? RL_POOL_MAXBLOCKS : kFit);
};

} // namespace rl
