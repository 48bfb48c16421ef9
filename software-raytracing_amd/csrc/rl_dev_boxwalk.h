// The point walk of k_nearest, k_nearest_all and k_sdf_dist -- a walk that the distance from a point to a box drives, not a ray -- written once, with the pieces
// that the box-driven kernels share: the isect record's vertices, the grid node's decode, the packed distance of the point walk's stack, the chunk claim and
// the counter fold.  rl_nearest.hip, rl_overlap.hip, rl_overlap_box.hip, rl_sdf.hip and rl_sweep.hip include this file; no other unit does (the ray kernels keep their own claim and fold).
// k_sweep takes the pieces from here and keeps its walk -- the point walk's shape with a time bound in the distance's place -- in rl_k_sweep.inl.
// k_overlap and k_overlap_contacts take the vertices and the claim from here and keep their box walk, its grid decode and their fold in rl_k_overlap.inl:
// on the shared walk the 4-wide ANY instance ran 1 % longer than the parent's in every job (profiles/box_walk_ab.log).
// k_overlap_box keeps that walk's text a second time (rl_k_overlap_box.inl) and takes the vertices, the claim, the grid node's decode and the fold from here.
//
// The walk: one point per lane, the stack is this lane's column of an LDS array (entry k at stk[k * RL_BLOCK]), the root is an inner node, a leaf holds <= 4
// triangles stored back to back.  It pushes at most (children - 1) references per level, as the ray walks do, so the planner's bounds hold: the binary
// tree's depth and the 4-wide tree's BVH::stackNeed4.  A push beyond STACK is dropped.
#pragma once

#include "rl_kernels.h"
#include "rl_nearest.h"

namespace rl {

// ---- the pieces ----
// the vertices of isect slot `slot`: three 16-byte loads of its 64-byte record
__device__ __forceinline__ void IsectVertices(const DSceneView& S, int slot, float v0[3], float v1[3], float v2[3])
{
	const float4* tp = (const float4*)(S.isect + slot);
	const float4 q0 = GLoadF4(tp, 0), q1 = GLoadF4(tp, 1), q2 = GLoadF4(tp, 2);
	v0[0] = q0.x; v0[1] = q0.y; v0[2] = q0.z;
	v1[0] = q1.z; v1[1] = q1.w; v1[2] = q2.x;
	v2[0] = q2.y; v2[1] = q2.z; v2[2] = q2.w;
}

// The 64-byte grid node, and child c's box and reference.  The planes are decoded as origin + (float)q * step -- the product is exact (q <= 255, step a
// power of two), the sum rounds once, monotonically, so the decoded box still contains the float box the planes were rounded outwards from (rl_grid.h).
struct GridNode { float4 h0; uint4 l, u, ch; };
__device__ __forceinline__ GridNode LoadGridNode(const DNode4Q* np) { GridNode N; N.h0 = GLoadF4(np, 0); N.l = GLoadU4(np, 1); N.u = GLoadU4(np, 2); N.ch = GLoadU4(np, 3); return N; }
__device__ __forceinline__ int GridChild(const GridNode& N, int c, float lo[3], float hi[3])
{
	const int sh = 8 * c;
	const float sx = N.h0.w, sy = __uint_as_float(N.l.w), sz = __uint_as_float(N.u.w);
	lo[0] = N.h0.x + (float)((N.l.x >> sh) & 0xffu) * sx; hi[0] = N.h0.x + (float)((N.u.x >> sh) & 0xffu) * sx;
	lo[1] = N.h0.y + (float)((N.l.y >> sh) & 0xffu) * sy; hi[1] = N.h0.y + (float)((N.u.y >> sh) & 0xffu) * sy;
	lo[2] = N.h0.z + (float)((N.l.z >> sh) & 0xffu) * sz; hi[2] = N.h0.z + (float)((N.u.z >> sh) & 0xffu) * sz;
	return (int)(c == 0 ? N.ch.x : c == 1 ? N.ch.y : c == 2 ? N.ch.z : N.ch.w);
}

// The box distance that rides beside a reference on the point walk's stack, in BYTES bytes: 0 none, 4 the float, 2 its upper half (a distance is >= +0, so
// dropping mantissa bits rounds it down: the pop's re-test then culls a little less, never more).  No choice changes a result.
template <int BYTES> struct NearestDist;
template <> struct NearestDist<0> { typedef float T; static __device__ __forceinline__ T Pack(float) { return 0.0f; } static __device__ __forceinline__ float Unpack(T) { return 0.0f; } };
template <> struct NearestDist<4> { typedef float T; static __device__ __forceinline__ T Pack(float d) { return d; } static __device__ __forceinline__ float Unpack(T v) { return v; } };
template <> struct NearestDist<2> {
	typedef unsigned short T;
	static __device__ __forceinline__ T Pack(float d) { return (T)(__float_as_uint(d) >> 16); }
	static __device__ __forceinline__ float Unpack(T v) { return __uint_as_float((uint32_t)v << 16); }
};

// a wave's next `amount` items of the launch's counter: one atomic by lane 0, the same base in every lane
__device__ __forceinline__ uint32_t ClaimChunk(unsigned int* __restrict__ counter, uint32_t amount, uint32_t lane)
{
	uint32_t base = 0u;
	if (lane == 0u) base = atomicAdd(counter, amount);
	return (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
}

// the lanes' items, nodes and triangles into counters[CNT_RAYS ..]: wave reduction, one atomic per wave and counter
__device__ __forceinline__ void FoldWaveCounters(unsigned long long* __restrict__ counters, uint32_t items, uint32_t nodes, uint32_t tris, uint32_t lane)
{
	if (!counters) return;
	const uint32_t vals[3] = { items, nodes, tris };
	for (int k = 0; k < 3; ++k) {
		unsigned long long v = vals[k];
		for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
		if (lane == 0u && v) atomicAdd(&counters[CNT_RAYS + k], v);
	}
}

constexpr int RL_WALK_DONE = 0x7fffffff;   // a walk's "nothing left": not a node index, not negative

// ---- the point walk ----
// Point p descends the tree TREE (2: S.nodes, 4: S.nodes4).  Children are ordered and culled by the distance from the point to their box (rl_nearest.h
// NearestBoxDist2), not by a parametric distance, and nothing is widened: a child is dropped when its box distance is > bound, kept when it is == bound (a
// tie may still win on the export index).  leaf(first, count) tests a leaf's triangles; it may lower `bound`, and the walk ends, returning true, when it
// returns true.  A popped reference is re-tested against the current bound when the stack keeps its box distance beside it (DBYTES != 0, dstk this lane's
// column of them); otherwise the popped node's children's tests (a leaf's own-box tests) do the culling, one fetch later.
template <int TREE, int STACK, int DBYTES, class LEAF>
__device__ __forceinline__ bool PointWalk(const DSceneView& S, const float p[3], float& bound, int* stk, typename NearestDist<DBYTES>::T* dstk, uint32_t& nodes, LEAF&& leaf)
{
	static_assert(TREE == 2 || TREE == 4, "tree");
	typedef NearestDist<DBYTES> Dist;
	const int DONE = RL_WALK_DONE;
	int sp = 0, cur = 0;
	// (push and pop as macros: written as lambdas, the pop's loop comes out of the compiler with a branch more per entry, and the kernels whose bound moves
	// run 5 to 10 % longer -- profiles/box_walk_ab.log)
#define RL_WALK_PUSH(ref_, d_) { if (sp < STACK) { stk[sp * RL_BLOCK] = (ref_); if constexpr (DBYTES != 0) dstk[sp * RL_BLOCK] = Dist::Pack(d_); ++sp; } }
	// the stack's next entry that the bound has not passed since it was pushed
#define RL_WALK_POP() while (cur == DONE && sp > 0) { --sp; if constexpr (DBYTES != 0) if (Dist::Unpack(dstk[sp * RL_BLOCK]) > bound) continue; cur = stk[sp * RL_BLOCK]; }
	for (;;) {
		// ---- descend: inner nodes until this lane holds a leaf or has nothing left ----
		while (cur >= 0 && cur != DONE) {
			++nodes;
			if constexpr (TREE == 2) {
				const float4* np = (const float4*)(S.nodes + cur);
				const float4 q0 = GLoadF4(np, 0), q1 = GLoadF4(np, 1), q2 = GLoadF4(np, 2);
				const uint4 ku = GLoadU4(np, 3);
				const int kl = (int)ku.x, kr = (int)ku.y;
				const float dl = NearestBoxDist2(p[0], p[1], p[2], q0.x, q0.y, q0.z, q0.w, q1.x, q1.y);
				const float dr = NearestBoxDist2(p[0], p[1], p[2], q1.z, q1.w, q2.x, q2.y, q2.z, q2.w);
				const bool hl = kl != DNODE_EMPTY && !(dl > bound), hr = kr != DNODE_EMPTY && !(dr > bound);
				if (hl && hr) {
					const bool leftFirst = dl <= dr;
					RL_WALK_PUSH(leftFirst ? kr : kl, leftFirst ? dr : dl)
					cur = leftFirst ? kl : kr;
				} else if (hl) cur = kl;
				else if (hr) cur = kr;
				else cur = DONE;
			} else {
				const GridNode N = LoadGridNode(S.nodes4 + cur);
				float t[4]; int r[4];
#pragma unroll
				for (int c = 0; c < 4; ++c) {
					float lo[3], hi[3];
					r[c] = GridChild(N, c, lo, hi);
					t[c] = NearestBoxDist2(p[0], p[1], p[2], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
					// a dropped child: no reference, behind every kept one (a kept child's distance may be +inf too: the reference tells them apart)
					if (r[c] == DNODE_EMPTY || t[c] > bound) { r[c] = DNODE_EMPTY; t[c] = INFINITY; }
				}
				RL_SORT4(t[0], r[0], t[1], r[1], t[2], r[2], t[3], r[3])
				// from the farthest to the nearest: the nearest kept child is walked next, the others are pushed farthest first
				int nr = r[3]; float nt = t[3];
#pragma unroll
				for (int c = 2; c >= 0; --c) if (r[c] != DNODE_EMPTY) { if (nr != DNODE_EMPTY) RL_WALK_PUSH(nr, nt) nr = r[c]; nt = t[c]; }
				cur = nr != DNODE_EMPTY ? nr : DONE;
			}
			RL_WALK_POP()   // nothing kept
		}
		if (cur == DONE) return false;
		// ---- leaf ----
		const LeafRef L = DecodeLeaf(cur);
		if (leaf(L.first, L.count)) return true;
		cur = DONE;
		RL_WALK_POP()
		if (cur == DONE) return false;
	}
}

#undef RL_WALK_POP
#undef RL_WALK_PUSH

// the walk's state of one point of a closest-triangle query: the least D so far, its slot and its barycentrics
struct NearestBest { float d; int slot; float b1, b2; };

// One leaf of a WITHIN or CLOSEST query (rl_kernels.h RL_NK_*): `count` triangles from slot `first`.  True: a WITHIN query has found its candidate.  A
// triangle replaces the best when its D is smaller, or equal with a lower export index (slotIndex, read on a tie only).
template <int KIND>
__device__ __forceinline__ bool NearestLeaf(const DSceneView& S, const float p[3], int first, int count, NearestBest& best, const int32_t* __restrict__ slotIndex, uint32_t& tris)
{
	for (int i = 0; i < count; ++i) {
		const int slot = first + i;
		float v0[3], v1[3], v2[3];
		IsectVertices(S, slot, v0, v1, v2);
		++tris;
		const float B = NearestOwnBoxDist2(p, v0, v1, v2);
		if (B > best.d) continue;   // D >= B: not a candidate, and E need not be known
		float b1, b2;
		const float D = NearestTriangleD(NearestTriangleE(p, v0, v1, v2, b1, b2), B);
		if (D > best.d) continue;
		if (KIND == RL_NK_WITHIN) return true;   // D <= R2 (best.d never moves)
		if (D == best.d && best.slot >= 0) {
			const int mine = slotIndex ? slotIndex[slot] : slot, theirs = slotIndex ? slotIndex[best.slot] : best.slot;
			if (mine > theirs) continue;
		}
		best.d = D; best.slot = slot; best.b1 = b1; best.b2 = b2;
	}
	return false;
}

} // namespace rl
