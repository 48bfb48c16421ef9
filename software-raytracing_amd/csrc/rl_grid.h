// The 8-bit grid of the wide nodes (rl_device.h DNode4Q, DNode8) and the re-derivation of every wide format from the binary tree's boxes, one statement
// for the host and the device: the builder (rl_bvh.cc QuantizeWide, EmitWide8) quantises with it, the refit behind a move of the scene's triangles
// (rl_refit.hip, rl_rt_move.hip) re-derives with it.  Every decision is made in double, where origin + q * step is exact, with IEEE operations only
// (+ - * /, floor, ceil, bit patterns), so "the grid box contains the float box" holds exactly and the host and the device agree.
#pragma once

#include "rl_device.h"

#if defined(__HIPCC__)
#define RL_GRID_HD __host__ __device__ inline
#else
#define RL_GRID_HD inline
#endif

namespace rl {

#define RL_BOX_MAX 3.40282347e+38f   /* FLT_MAX: an unused child's float box is [FLT_MAX, -FLT_MAX] */

// One axis of a node's grid: anchored at the least lower bound of the node's children, the step the smallest power of two whose 255 steps span them.
struct GridAxis { float origin; int exp; double step; };   // exp: the step's biased exponent, step = 2^(exp - 127), 1 <= exp <= 254
RL_GRID_HD double GridPow2(int biased) { return __builtin_bit_cast(double, (uint64_t)(biased - 127 + 1023) << 52); }
RL_GRID_HD GridAxis GridAxisOf(float lo, float hi)   // the least lower and the greatest upper bound over the children; lo > hi: the node has none
{
	if (!(lo <= hi)) { lo = hi = 0.0f; }
	GridAxis G; G.origin = lo;
	const double extent = (double)hi - (double)lo;
	int e = 1;   // 2^-126, the smallest normal
	if (extent > 0.0) {
		// frexp(extent / 255): the x with extent / 255 = m 2^x, 0.5 <= m < 1 (the quotient is a normal double: extent >= 2^-149)
		const int x = (int)((__builtin_bit_cast(uint64_t, extent / 255.0) >> 52) & 0x7ffu) - 1022;
		e = x + 127 < 1 ? 1 : (x + 127 > 254 ? 254 : x + 127);
	}
	double step = GridPow2(e);
	while (255.0 * step < extent && e < 254) { ++e; step *= 2.0; }
	G.exp = e; G.step = step;
	return G;
}
// a child's planes on that axis: the lower one rounded down, the upper one up
RL_GRID_HD void GridPlanes(const GridAxis& G, float blo, float bhi, uint32_t& ql, uint32_t& qh)
{
	const double lo = (double)G.origin, step = G.step;
	double l = __builtin_floor(((double)blo - lo) / step), h = __builtin_ceil(((double)bhi - lo) / step);
	l = l < 0.0 ? 0.0 : (l > 255.0 ? 255.0 : l); h = h < 0.0 ? 0.0 : (h > 255.0 ? 255.0 : h);
	while (l > 0.0 && lo + l * step > (double)blo) l -= 1.0;
	while (h < 255.0 && lo + h * step < (double)bhi) h += 1.0;
	ql = (uint32_t)l; qh = (uint32_t)h;
}

// DNode4 -> DNode4Q: same children; an unused child (DNODE_EMPTY) keeps the inverted grid box, lower 255 / upper 0
RL_GRID_HD DNode4Q QuantizeNode4(const DNode4& n)
{
	DNode4Q q;
	float steps[3];
	for (int a = 0; a < 3; ++a) {
		float lo = RL_BOX_MAX, hi = -RL_BOX_MAX;
		for (int k = 0; k < 4; ++k) if (n.child[k] != DNODE_EMPTY) { lo = n.lo[a][k] < lo ? n.lo[a][k] : lo; hi = hi < n.hi[a][k] ? n.hi[a][k] : hi; }
		const GridAxis G = GridAxisOf(lo, hi);
		q.origin[a] = G.origin; steps[a] = (float)G.step;   // a power of two between 2^-126 and 2^127: exact
		q.qlo[a] = 0u; q.qhi[a] = 0u;
		for (int k = 0; k < 4; ++k) {
			if (n.child[k] == DNODE_EMPTY) { q.qlo[a] |= 255u << (8 * k); continue; }
			uint32_t l, h; GridPlanes(G, n.lo[a][k], n.hi[a][k], l, h);
			q.qlo[a] |= l << (8 * k); q.qhi[a] |= h << (8 * k);
		}
	}
	q.stepX = steps[0]; q.stepY = steps[1]; q.stepZ = steps[2];
	for (int k = 0; k < 4; ++k) q.child[k] = n.child[k];
	return q;
}

// The boxes of an 8-wide node's children (used: bit c = slot c holds a child) into n: origin, the steps' exponents (meta's low 24 bits; its imask stays)
// and the planes.  Everything else of n is topology and is not touched.
RL_GRID_HD void QuantizeNode8(const float lo[3][8], const float hi[3][8], uint32_t used, DNode8& n)
{
	uint32_t exps = 0u;
	for (int a = 0; a < 3; ++a) {
		float mn = RL_BOX_MAX, mx = -RL_BOX_MAX;
		for (int c = 0; c < 8; ++c) if ((used >> c) & 1u) { mn = lo[a][c] < mn ? lo[a][c] : mn; mx = mx < hi[a][c] ? hi[a][c] : mx; }
		const GridAxis G = GridAxisOf(mn, mx);
		n.origin[a] = G.origin; exps |= (uint32_t)G.exp << (8 * a);
		n.qlo[a][0] = n.qlo[a][1] = n.qhi[a][0] = n.qhi[a][1] = 0u;
		for (int c = 0; c < 8; ++c) {
			if (!((used >> c) & 1u)) { n.qlo[a][c >> 2] |= 255u << (8 * (c & 3)); continue; }
			uint32_t l, h; GridPlanes(G, lo[a][c], hi[a][c], l, h);
			n.qlo[a][c >> 2] |= l << (8 * (c & 3)); n.qhi[a][c >> 2] |= h << (8 * (c & 3));
		}
	}
	n.meta = (n.meta & 0xff000000u) | exps;
}

// ---- the wide formats again from the binary tree's boxes (a refit) ----
// A box id names one child box of the binary tree, 2 * (node index) + (0: left, 1: right): the builder records, per child of every wide record, the id of
// the binary node's box it emitted that child from (rl_host.h BVH::boxOf4 / boxOf8 / boxOfLeafList; -1: the slot is unused).
RL_GRID_HD void BoxOfId(const DNode* nodes, int32_t id, float mn[3], float mx[3])
{
	const DNode& nd = nodes[id >> 1];
	const float* a = (id & 1) ? nd.rmin : nd.lmin; const float* b = (id & 1) ? nd.rmax : nd.lmax;
	for (int k = 0; k < 3; ++k) { mn[k] = a[k]; mx[k] = b[k]; }
}
// the float boxes of wide node n's used children (its child references are in place and stay)
RL_GRID_HD void RefitNode4(const DNode* nodes, const int32_t ids[4], DNode4& n)
{
	for (int k = 0; k < 4; ++k) {
		if (ids[k] < 0) continue;
		float mn[3], mx[3]; BoxOfId(nodes, ids[k], mn, mx);
		for (int a = 0; a < 3; ++a) { n.lo[a][k] = mn[a]; n.hi[a][k] = mx[a]; }
	}
}
RL_GRID_HD void RefitNode8(const DNode* nodes, const int32_t ids[8], DNode8& n)
{
	float lo[3][8], hi[3][8]; uint32_t used = 0u;
	for (int c = 0; c < 8; ++c) {
		if (ids[c] < 0) continue;
		used |= 1u << c;
		float mn[3], mx[3]; BoxOfId(nodes, ids[c], mn, mx);
		for (int a = 0; a < 3; ++a) { lo[a][c] = mn[a]; hi[a][c] = mx[a]; }
	}
	QuantizeNode8(lo, hi, used, n);
}

} // namespace rl
