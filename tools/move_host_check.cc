// Stand-alone check of the host side of RaylibAMD_SceneMoveTriangles (tools/host_check.sh move runs it under ASan + UBSan; tests/test_move_host.py runs it plain):
// the box ids the builder records per child of every wide record (csrc/rl_host.h BVH::boxOf4 / boxOf8 / boxOfLeafList), the grid rule shared with the device
// (csrc/rl_grid.h) against the builder's former quantiser restated here, the leaf order as a permutation, and the host half of a moved scene's refresh (csrc/rl_bvh.cc
// RefitWideFromBinary) behind a refit of the binary tree's boxes restated here.  Linked with rl_bvh.cc and rl_log.cc only; never part of libraylib.so.
#include "rl_host.h"
#include "rl_grid.h"
#include <algorithm>
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace rl;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "move_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static uint32_t Mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
static float Unit(uint32_t k) { return (float)(Mix(k) & 0xffffu) / 65536.0f; }

static std::vector<HostTriangle> Soup(int n, uint32_t seed)
{
	std::vector<HostTriangle> tris((size_t)n);
	for (int i = 0; i < n; ++i) {
		HostTriangle t; memset(&t, 0, sizeof(t));
		const uint32_t k = seed + 16u * (uint32_t)i;
		const f3 c = F3(4.0f * Unit(k) - 2.0f, 4.0f * Unit(k + 1) - 2.0f, 4.0f * Unit(k + 2) - 2.0f);
		t.v0 = c + F3(0.3f * Unit(k + 3), 0.3f * Unit(k + 4), 0.3f * Unit(k + 5));
		t.v1 = c + F3(0.3f * Unit(k + 6), 0.3f * Unit(k + 7), 0.3f * Unit(k + 8));
		t.v2 = c + F3(0.3f * Unit(k + 9), 0.3f * Unit(k + 10), 0.3f * Unit(k + 11));
		tris[(size_t)i] = t;
	}
	return tris;
}
static void Build(const std::vector<HostTriangle>& tris, BVH& out)
{
	std::vector<PrimRef> prims;
	for (size_t i = 0; i < tris.size(); ++i) {
		const HostTriangle& t = tris[i];
		PrimRef p; p.mn = fmin3(fmin3(t.v0, t.v1), t.v2); p.mx = fmax3(fmax3(t.v0, t.v1), t.v2); p.kind = PRIM_TRIANGLE; p.index = (uint32_t)i;
		prims.push_back(p);
	}
	BuildBVH(prims, out);
}
// the device's k_refit_level on the host: children follow their parent in `nodes`, so a reverse sweep is bottom-up
static void RefitBinary(BVH& B, const std::vector<HostTriangle>& tris)
{
	for (size_t i = B.nodes.size(); i-- > 0;) {
		DNode& nd = B.nodes[i];
		for (int side = 0; side < 2; ++side) {
			const int32_t ref = side ? nd.right : nd.left;
			float* mn = side ? nd.rmin : nd.lmin; float* mx = side ? nd.rmax : nd.lmax;
			if (ref == DNODE_EMPTY) continue;
			f3 lo = F3(FLT_MAX, FLT_MAX, FLT_MAX), hi = F3(-FLT_MAX, -FLT_MAX, -FLT_MAX);
			if (ref >= 0) {
				const DNode& c = B.nodes[(size_t)ref];
				lo = fmin3(F3(c.lmin[0], c.lmin[1], c.lmin[2]), F3(c.rmin[0], c.rmin[1], c.rmin[2]));
				hi = fmax3(F3(c.lmax[0], c.lmax[1], c.lmax[2]), F3(c.rmax[0], c.rmax[1], c.rmax[2]));
			} else {
				const uint32_t code = (uint32_t)~ref, first = code >> LEAF_FIRST_SHIFT, count = (code & LEAF_COUNT_MASK) + 1u;
				for (uint32_t k = 0; k < count; ++k) {
					const HostTriangle& t = tris[B.triOrder[first + k]];
					lo = fmin3(fmin3(fmin3(lo, t.v0), t.v1), t.v2); hi = fmax3(fmax3(fmax3(hi, t.v0), t.v1), t.v2);
				}
			}
			mn[0] = lo.x; mn[1] = lo.y; mn[2] = lo.z; mx[0] = hi.x; mx[1] = hi.y; mx[2] = hi.z;
		}
	}
}
// The builder's quantiser as it stood before rl_grid.h (frexp / ldexp, division by the step), restated: what rl_grid.h's rule must reproduce bit for bit.
// lo / hi: the planes' inputs of one axis; returns the origin, the biased exponent, and the planes of n children (unused: lower 255, upper 0).
struct FormerAxis { float origin; int e; uint32_t ql[8], qh[8]; };
static FormerAxis FormerGrid(const float* blo, const float* bhi, const bool* used, int n)
{
	FormerAxis A;
	float lo = FLT_MAX, hi = -FLT_MAX;
	for (int k = 0; k < n; ++k) if (used[k]) { lo = std::min(lo, blo[k]); hi = std::max(hi, bhi[k]); }
	if (!(lo <= hi)) { lo = hi = 0.0f; }
	A.origin = lo;
	const double extent = (double)hi - (double)lo;
	int e = 1;
	if (extent > 0.0) { int x; (void)frexp(extent / 255.0, &x); e = std::max(1, std::min(254, x + 127)); }
	double step = ldexp(1.0, e - 127);
	while (255.0 * step < extent && e < 254) { ++e; step *= 2.0; }
	A.e = e;
	for (int k = 0; k < n; ++k) {
		if (!used[k]) { A.ql[k] = 255u; A.qh[k] = 0u; continue; }
		double l = floor(((double)blo[k] - (double)lo) / step), h = ceil(((double)bhi[k] - (double)lo) / step);
		l = std::max(0.0, std::min(255.0, l)); h = std::max(0.0, std::min(255.0, h));
		while (l > 0.0 && (double)lo + l * step > (double)blo[k]) l -= 1.0;
		while (h < 255.0 && (double)lo + h * step < (double)bhi[k]) h += 1.0;
		A.ql[k] = (uint32_t)l; A.qh[k] = (uint32_t)h;
	}
	return A;
}
template <typename T> static bool SameBytes(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

static int CheckScene(int n, bool wantLeafList, bool wantWide8)
{
	const std::vector<HostTriangle> tris = Soup(n, 77u + (uint32_t)n);
	BVH B; Build(tris, B);
	CHECK(ValidateBVH(B, tris) && ValidateBVH4(B, tris) && ValidateBVH8(B, tris));
	CHECK(B.leafList.empty() != wantLeafList && B.nodes8.empty() != wantWide8);
	// the leaf order is a permutation of the triangles: its inverse (triangle -> slot) exists
	std::vector<int> seen((size_t)n, 0);
	CHECK(B.triOrder.size() == (size_t)n);
	for (uint32_t t : B.triOrder) { CHECK(t < (uint32_t)n && !seen[t]); seen[t] = 1; }
	// every wide child names the binary tree's box it was emitted from
	CHECK(B.boxOf4.size() == 4 * B.nodes4.size() && B.boxOf8.size() == 8 * B.nodes8.size() && B.boxOfLeafList.size() == 4 * B.leafList.size());
	auto sameBox = [&](int32_t id, const DNode4& nd, int k) {
		float mn[3], mx[3]; BoxOfId(B.nodes.data(), id, mn, mx);
		for (int a = 0; a < 3; ++a) if (memcmp(&mn[a], &nd.lo[a][k], 4) != 0 || memcmp(&mx[a], &nd.hi[a][k], 4) != 0) return false;
		return true;
	};
	for (size_t i = 0; i < B.nodes4.size(); ++i) for (int k = 0; k < 4; ++k) {
		const int32_t id = B.boxOf4[4 * i + (size_t)k];
		CHECK((id < 0) == (B.nodes4[i].child[k] == DNODE_EMPTY) && (id < 0 || ((size_t)(id >> 1) < B.nodes.size() && sameBox(id, B.nodes4[i], k))));
	}
	for (size_t i = 0; i < B.leafList.size(); ++i) for (int k = 0; k < 4; ++k) {
		const int32_t id = B.boxOfLeafList[4 * i + (size_t)k];
		CHECK((id < 0) == (B.leafList[i].child[k] == DNODE_EMPTY) && (id < 0 || ((size_t)(id >> 1) < B.nodes.size() && sameBox(id, B.leafList[i], k))));
	}
	for (size_t i = 0; i < B.nodes8.size(); ++i) for (int c = 0; c < 8; ++c) {
		const DNode8& nd = B.nodes8[i];
		const bool used = ((nd.meta >> 24) >> c & 1u) || ((nd.leafMask >> (4 * c)) & 15u);
		const int32_t id = B.boxOf8[8 * i + (size_t)c];
		CHECK((id >= 0) == used && (id < 0 || (size_t)(id >> 1) < B.nodes.size()));
	}
	// the builder's grid records (made by rl_grid.h's rule) are what the former quantiser made of the same float boxes
	for (size_t i = 0; i < B.nodes4.size(); ++i) for (int a = 0; a < 3; ++a) {
		const DNode4& nd = B.nodes4[i]; const DNode4Q& q = B.nodes4q[i];
		bool used[4]; for (int k = 0; k < 4; ++k) used[k] = nd.child[k] != DNODE_EMPTY;
		const FormerAxis A = FormerGrid(nd.lo[a], nd.hi[a], used, 4);
		const float step = a == 0 ? q.stepX : (a == 1 ? q.stepY : q.stepZ), want = (float)ldexp(1.0, A.e - 127);
		CHECK(memcmp(&q.origin[a], &A.origin, 4) == 0 && memcmp(&step, &want, 4) == 0);
		for (int k = 0; k < 4; ++k) CHECK(((q.qlo[a] >> (8 * k)) & 255u) == A.ql[k] && ((q.qhi[a] >> (8 * k)) & 255u) == A.qh[k] && q.child[k] == nd.child[k]);
	}
	for (size_t i = 0; i < B.nodes8.size(); ++i) for (int a = 0; a < 3; ++a) {
		const DNode8& nd = B.nodes8[i];
		float blo[8], bhi[8]; bool used[8];
		for (int c = 0; c < 8; ++c) {
			used[c] = B.boxOf8[8 * i + (size_t)c] >= 0; blo[c] = bhi[c] = 0.0f;
			if (used[c]) { float mn[3], mx[3]; BoxOfId(B.nodes.data(), B.boxOf8[8 * i + (size_t)c], mn, mx); blo[c] = mn[a]; bhi[c] = mx[a]; }
		}
		const FormerAxis A = FormerGrid(blo, bhi, used, 8);
		CHECK(memcmp(&nd.origin[a], &A.origin, 4) == 0 && ((nd.meta >> (8 * a)) & 255u) == (uint32_t)A.e);
		for (int c = 0; c < 8; ++c) CHECK(((nd.qlo[a][c >> 2] >> (8 * (c & 3))) & 255u) == A.ql[c] && ((nd.qhi[a][c >> 2] >> (8 * (c & 3))) & 255u) == A.qh[c]);
	}
	// the re-derivation from the binary tree's boxes through the recorded ids gives the builder's records and cost back, byte for byte
	{
		BVH R = B;
		for (DNode4& nd : R.nodes4) for (int k = 0; k < 4; ++k) if (nd.child[k] != DNODE_EMPTY) for (int a = 0; a < 3; ++a) nd.lo[a][k] = nd.hi[a][k] = 12345.0f;
		for (DNode4& nd : R.leafList) for (int k = 0; k < 4; ++k) if (nd.child[k] != DNODE_EMPTY) for (int a = 0; a < 3; ++a) nd.lo[a][k] = nd.hi[a][k] = 12345.0f;
		for (DNode4Q& q : R.nodes4q) { q.origin[0] = q.origin[1] = q.origin[2] = -1.0f; q.qlo[0] = q.qhi[1] = 0x01020304u; q.stepX = q.stepY = q.stepZ = 3.0f; }
		for (DNode8& nd : R.nodes8) { nd.origin[0] = nd.origin[2] = 9.0f; nd.meta ^= 0x00123456u; nd.qlo[0][0] = nd.qhi[2][1] = 0x0a0b0c0du; }
		R.sahCost = -1.0f;
		RefitWideFromBinary(R);
		CHECK(SameBytes(R.nodes4, B.nodes4) && SameBytes(R.nodes4q, B.nodes4q) && SameBytes(R.nodes8, B.nodes8) && SameBytes(R.leafList, B.leafList));
		CHECK(memcmp(&R.sahCost, &B.sahCost, 4) == 0);
	}
	// a third of the triangles moved: the refitted trees hold the moved scene, and cost at least what a fresh build of it costs
	{
		std::vector<HostTriangle> moved = tris;
		for (int i = n / 3; i < 2 * (n / 3); ++i) { HostTriangle& t = moved[(size_t)i]; const f3 d = F3(1.25f, -0.5f, 2.0f); t.v0 = t.v0 + d; t.v1 = t.v1 + d; t.v2 = t.v2 + d; }
		BVH R = B;
		CHECK(!ValidateBVH(R, moved));
		RefitBinary(R, moved);
		RefitWideFromBinary(R);
		CHECK(ValidateBVH(R, moved) && ValidateBVH4(R, moved) && ValidateBVH8(R, moved));
		BVH F; Build(moved, F);
		CHECK(R.sahCost == R.sahCost && R.sahCost < FLT_MAX && R.sahCost >= F.sahCost);
		// ... and moved back: the trees the builder made
		RefitBinary(R, tris);
		RefitWideFromBinary(R);
		CHECK(SameBytes(R.nodes, B.nodes) && SameBytes(R.nodes4, B.nodes4) && SameBytes(R.nodes4q, B.nodes4q) && SameBytes(R.nodes8, B.nodes8) && SameBytes(R.leafList, B.leafList));
		CHECK(memcmp(&R.sahCost, &B.sahCost, 4) == 0);
	}
	return 0;
}

int main(int argc, char** argv)
{
	if (CheckScene(60, true, false)) return 1;      // the leaf list's class
	if (CheckScene(700, false, true)) return 1;     // the wide trees, the 8-wide one included
	if (argc > 1 && !strcmp(argv[1], "big") && CheckScene(70000, false, true)) return 1;   // ... with the grid copy's threaded stage (the sanitizer run)
	printf("move_host_check: ok\n");
	return 0;
}
