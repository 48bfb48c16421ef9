// Sanitizer harness only (tools/host_check.sh box): a stand-alone program over the host side of RaylibAMD_OverlapBoxes -- the statements of csrc/rl_box.h called
// directly on the special values, the host oracle RaylibAMD_OverlapBoxesHost on heap arrays of exactly the sizes the contract names (the specials and a random
// set, all three kinds), every refusal, and the planner -- linked with tools/nodevice_stub.cc in place of the device units, so every accepted call of the plain
// and the device entry ends at "no device" (0).  Never part of libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include "rl_box.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "box_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static float Rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); }

static RaylibAMDBoxQuery Box(const float c[3], float hx, float hy, float hz)
{
	RaylibAMDBoxQuery Q;
	memset(&Q, 0xff, sizeof(Q));   // (the reserved word is not read)
	for (int a = 0; a < 3; ++a) { Q.center[a] = c[a]; for (int k = 0; k < 3; ++k) Q.axis[a].dir[k] = a == k ? 1.0f : 0.0f; }
	Q.axis[0].half = hx; Q.axis[1].half = hy; Q.axis[2].half = hz;
	return Q;
}
// the axes turned about z by `angle`, then about x by half of it
static void Turn(RaylibAMDBoxQuery& Q, float angle)
{
	const float c = cosf(angle), s = sinf(angle), c2 = cosf(0.5f * angle), s2 = sinf(0.5f * angle);
	const float R[3][3] = { { c, s, 0 }, { -s * c2, c * c2, s2 }, { s * s2, -c * s2, c2 } };
	for (int a = 0; a < 3; ++a) for (int k = 0; k < 3; ++k) Q.axis[a].dir[k] = R[a][k];
}
static rl::BoxQ Statement(const RaylibAMDBoxQuery& q)
{
	rl::BoxQ Q;
	for (int a = 0; a < 3; ++a) { Q.c[a] = q.center[a]; Q.h[a] = q.axis[a].half; for (int k = 0; k < 3; ++k) Q.a[a][k] = q.axis[a].dir[k]; }
	return Q;
}

int main()
{
	const float grey[3] = { 0.5f, 0.5f, 0.5f }, zero[3] = { 0, 0, 0 }, one[3] = { 1, 1, 1 }, up[3] = { 0, 1, 0 };
	MaterialHandle m = RaylibAMD_CreateMaterial(0, grey, 1.0f, 0.0f, zero, 1.5f, one, 0.0f);
	CHECK(m);
	// a soup of 300 triangles (the elements live as long as the program); triangle 0 lies in the plane x = 1
	const int numTris = 300, words = (numTris + 31) / 32;
	std::vector<float> verts;
	SceneHandle scene = Raylib_CreateScene(), unfinished = Raylib_CreateScene();
	CHECK(scene && unfinished);
	{
		uint32_t s = 12345u;
		for (int k = 0; k < numTris; ++k) {
			const float c[3] = { Rnd(s) * 8 - 4, Rnd(s) * 8 - 4, Rnd(s) * 8 - 4 };
			float p[9];
			for (int a = 0; a < 9; ++a) p[a] = c[a % 3] + Rnd(s) * 1.6f - 0.8f;
			if (k == 0) { const float flat[9] = { 1, 0, 0, 1, 1, 0, 1, 0, 1 }; memcpy(p, flat, sizeof(p)); }
			for (int a = 0; a < 9; ++a) verts.push_back(p[a]);
			SceneElementHandle e = RaylibAMD_CreateTriangle(p, p + 3, p + 6, up, up, up, NULL, m);
			CHECK(e);
			Raylib_AddSceneElement(scene, e);
		}
	}
	Raylib_FinalizeScene(scene);
	CHECK(RaylibAMD_SceneNumTriangles(scene) == numTris);

	SceneElementHandle sphere = RaylibAMD_CreateSphere(0, 0, 0, 0.5f, m);
	SceneHandle prims = Raylib_CreateScene();
	CHECK(sphere && prims);
	Raylib_AddSceneElement(prims, sphere);
	Raylib_FinalizeScene(prims);

	// ---- the statements, called directly ----
	{
		const float* t0 = &verts[0];
		const float c[3] = { 1.5f, 0.25f, 0.25f };
		rl::BoxQ Q = Statement(Box(c, 0.5f, 1.0f, 1.0f));   // its face x = 1 lies exactly on triangle 0's plane
		CHECK(rl::BoxTakesPart(Q));
		rl::BoxEnclosing(Q);
		CHECK(Q.lo[0] == 1.0f && Q.hi[0] == 2.0f && rl::BoxAccepts(Q, t0, t0 + 3, t0 + 6));
		Q = Statement(Box(c, 0.25f, 1.0f, 1.0f)); rl::BoxEnclosing(Q);
		CHECK(!rl::BoxAccepts(Q, t0, t0 + 3, t0 + 6));
		const float corner[3] = { 1.5f, 1.5f, -0.5f };   // its corner (1, 1, 0) is triangle 0's second vertex
		Q = Statement(Box(corner, 0.5f, 0.5f, 0.5f)); rl::BoxEnclosing(Q);
		CHECK(rl::BoxAccepts(Q, t0, t0 + 3, t0 + 6));
		const float inside[3] = { 1.0f, 0.25f, 0.25f };   // a point in the triangle's interior, a rectangle through it, a box with a -0.0 half extent
		Q = Statement(Box(inside, 0.0f, 0.0f, 0.0f)); rl::BoxEnclosing(Q);
		CHECK(rl::BoxTakesPart(Q) && rl::BoxAccepts(Q, t0, t0 + 3, t0 + 6));
		Q = Statement(Box(inside, 0.125f, -0.0f, 0.0f)); rl::BoxEnclosing(Q);
		CHECK(rl::BoxTakesPart(Q) && rl::BoxAccepts(Q, t0, t0 + 3, t0 + 6));
		for (float bad : { NAN, INFINITY, -INFINITY }) {
			RaylibAMDBoxQuery q = Box(c, 0.5f, 0.5f, 0.5f); q.center[1] = bad; CHECK(!rl::BoxTakesPart(Statement(q)));
			q = Box(c, 0.5f, 0.5f, 0.5f); q.axis[2].dir[0] = bad; CHECK(!rl::BoxTakesPart(Statement(q)));
			q = Box(c, 0.5f, 0.5f, 0.5f); q.axis[1].half = bad; CHECK(!rl::BoxTakesPart(Statement(q)));
		}
		CHECK(!rl::BoxTakesPart(Statement(Box(c, 0.5f, -1e-3f, 0.5f))));
		Q = Statement(Box(c, 1e30f, 1e30f, 1e30f)); rl::BoxEnclosing(Q);
		CHECK(rl::BoxTakesPart(Q) && rl::BoxAccepts(Q, t0, t0 + 3, t0 + 6));
		RaylibAMDBoxQuery huge = Box(c, 3e38f, 3e38f, 3e38f); Turn(huge, 0.7f);   // B2 overflows to infinity: fine, and no NaN
		Q = Statement(huge); rl::BoxEnclosing(Q);
		CHECK(rl::BoxTakesPart(Q) && Q.lo[0] == -INFINITY && Q.hi[0] == INFINITY && rl::BoxAccepts(Q, t0, t0 + 3, t0 + 6));
	}

	// ---- the oracle ----
	for (int n : { 0, 1, 7, 300 }) {
		// exactly n records, n * maxHits words, n counts and the mask's words, on the heap: the oracle may read and write nothing past them
		std::vector<RaylibAMDBoxQuery> q((size_t)n);
		uint32_t s = 99u + (uint32_t)n;
		for (int i = 0; i < n; ++i) {
			const float c[3] = { Rnd(s) * 8 - 4, Rnd(s) * 8 - 4, Rnd(s) * 8 - 4 };
			const float size = i % 3 == 1 ? 0.1f : i % 3 == 2 ? 2.0f : 12.0f;
			RaylibAMDBoxQuery& Q = q[(size_t)i];
			Q = Box(c, Rnd(s) * size, Rnd(s) * size, Rnd(s) * size);
			if (i % 2) Turn(Q, Rnd(s) * 6.0f);
			if (i % 3 == 0) for (int a = 0; a < 3; ++a) Q.center[a] = verts[(size_t)(i % numTris) * 9 + a];   // about a scene vertex
			if (i == 5) Q.center[1] = NAN;
			if (i == 6) Q.axis[0].half = Q.axis[1].half = Q.axis[2].half = 1e30f;
			if (i == 8) Q.axis[1].half = -1.0f;
			if (i == 9) memset(Q.axis, 0, sizeof(Q.axis));
		}
		RaylibAMDBoxQuery* qp = n ? q.data() : NULL;
		std::vector<uint32_t> any((size_t)n, 7u), mask((size_t)words, 0xffffffffu), ored((size_t)words, 0u);
		CHECK(RaylibAMD_OverlapBoxesHost(scene, RAYLIB_AMD_BOX_ANY, qp, n, 12345, n ? any.data() : NULL, NULL) == 1);
		CHECK(RaylibAMD_OverlapBoxesHost(scene, RAYLIB_AMD_BOX_MARK, qp, n, -7, mask.data(), NULL) == 1);
		CHECK((mask[(size_t)words - 1] >> (numTris % 32)) == 0u);
		if (n == 0) for (uint32_t w : mask) CHECK(w == 0u);
		for (int maxHits : { 1, 4, RAYLIB_AMD_MAX_OVERLAPS }) {
			std::vector<int32_t> rows((size_t)n * (size_t)maxHits, 7);
			std::vector<uint32_t> cnt((size_t)n, 7u);
			CHECK(RaylibAMD_OverlapBoxesHost(scene, RAYLIB_AMD_BOX_LIST, qp, n, maxHits, n ? rows.data() : NULL, n ? cnt.data() : NULL) == 1);
			std::vector<int32_t> rows2((size_t)n * (size_t)maxHits, 7);
			CHECK(RaylibAMD_OverlapBoxesHost(scene, RAYLIB_AMD_BOX_LIST, qp, n, maxHits, n ? rows2.data() : NULL, NULL) == 1);
			CHECK(rows == rows2);
			for (int i = 0; i < n; ++i) {
				const int32_t* row = &rows[(size_t)i * (size_t)maxHits];
				const uint32_t listed = cnt[(size_t)i] < (uint32_t)maxHits ? cnt[(size_t)i] : (uint32_t)maxHits;
				for (uint32_t e = 0; e < (uint32_t)maxHits; ++e) {
					if (e < listed) {
						CHECK(row[e] >= 0 && row[e] < numTris && (e == 0 || row[e - 1] < row[e]));
						CHECK((mask[(size_t)row[e] >> 5] >> (row[e] & 31)) & 1u);
					} else CHECK(row[e] == -1);
				}
				CHECK(any[(size_t)i] == (cnt[(size_t)i] ? 1u : 0u));
				if (i == 5 || i == 8) CHECK(cnt[(size_t)i] == 0);
				if (i == 6) CHECK(cnt[(size_t)i] == (uint32_t)numTris);
				if (i % 3 == 0 && i != 5 && i != 8 && i != 9) CHECK(cnt[(size_t)i] >= 1);
			}
			// accepted by the checks, then "no device" -- but no queries are a success without one
			CHECK(RaylibAMD_OverlapBoxes(scene, RAYLIB_AMD_BOX_LIST, qp, n, maxHits, n ? rows.data() : NULL, n ? cnt.data() : NULL) == 0);
			CHECK(RaylibAMD_OverlapBoxesDevice(scene, RAYLIB_AMD_BOX_LIST, qp, n, maxHits, n ? rows.data() : NULL, n ? cnt.data() : NULL, NULL) == 0);
		}
		// one call's mask is the OR of the calls of one
		for (int i = 0; i < n; ++i) {
			std::vector<uint32_t> one((size_t)words, 0xffffffffu);
			CHECK(RaylibAMD_OverlapBoxesHost(scene, RAYLIB_AMD_BOX_MARK, &q[(size_t)i], 1, 0, one.data(), NULL) == 1);
			for (int w = 0; w < words; ++w) ored[(size_t)w] |= one[(size_t)w];
		}
		CHECK(ored == mask);
		// the refusals write nothing
		std::vector<int32_t> out((size_t)(n * 4 > words ? n * 4 : words) + 1, 7);
		std::vector<uint32_t> cnt((size_t)n + 1, 7u);
		typedef int32_t (*Entry)(SceneHandle, int32_t, const RaylibAMDBoxQuery*, int32_t, int32_t, void*, uint32_t*);
		for (Entry f : { (Entry)RaylibAMD_OverlapBoxesHost, (Entry)RaylibAMD_OverlapBoxes }) {
			CHECK(f(scene, 3, qp, n, 4, out.data(), NULL) == 0 && f(scene, -1, qp, n, 4, out.data(), NULL) == 0);
			CHECK(f(scene, RAYLIB_AMD_BOX_LIST, qp, n, 0, out.data(), cnt.data()) == 0 && f(scene, RAYLIB_AMD_BOX_LIST, qp, n, RAYLIB_AMD_MAX_OVERLAPS + 1, out.data(), cnt.data()) == 0);
			CHECK(f(scene, RAYLIB_AMD_BOX_LIST, qp, 0x7fffffff, 2, out.data(), cnt.data()) == 0);
			CHECK(f(scene, RAYLIB_AMD_BOX_ANY, qp, n, 4, out.data(), cnt.data()) == 0 && f(scene, RAYLIB_AMD_BOX_MARK, qp, n, 4, out.data(), cnt.data()) == 0);
			CHECK(f(scene, RAYLIB_AMD_BOX_LIST, qp, -1, 4, out.data(), cnt.data()) == 0 && f(scene, RAYLIB_AMD_BOX_MARK, qp, -1, 4, out.data(), NULL) == 0);
			CHECK(f(unfinished, RAYLIB_AMD_BOX_MARK, qp, n, 4, out.data(), NULL) == 0 && f(prims, RAYLIB_AMD_BOX_MARK, qp, n, 4, out.data(), NULL) == 0);
			CHECK(f(0, RAYLIB_AMD_BOX_MARK, qp, n, 4, out.data(), NULL) == 0);
			if (n) CHECK(f(scene, RAYLIB_AMD_BOX_MARK, NULL, n, 4, out.data(), NULL) == 0 && f(scene, RAYLIB_AMD_BOX_MARK, qp, n, 4, NULL, NULL) == 0);
		}
		for (int32_t v : out) CHECK(v == 7);
		for (uint32_t v : cnt) CHECK(v == 7u);
	}
	// the planner: PlanOverlap's answer
	for (int kind : { RAYLIB_AMD_BOX_ANY, RAYLIB_AMD_BOX_LIST, RAYLIB_AMD_BOX_MARK }) {
		for (const char* env : { "", "2", "4", "8" }) {
			if (*env) setenv("RAYLIB_QUERY_TREE", env, 1); else unsetenv("RAYLIB_QUERY_TREE");
			RaylibAMDQueryPlan p, o;
			CHECK(RaylibAMD_PlanOverlapBoxes(scene, kind, &p) == 1);
			CHECK(RaylibAMD_PlanOverlap(scene, kind == RAYLIB_AMD_BOX_ANY ? RAYLIB_AMD_OVERLAP_ANY : RAYLIB_AMD_OVERLAP_LIST, &o) == 1);
			CHECK(memcmp(&p, &o, sizeof(p)) == 0 && p.early == (kind == RAYLIB_AMD_BOX_ANY));
			CHECK(RaylibAMD_PlanOverlapBoxes(scene, 3, &p) == 0 && RaylibAMD_PlanOverlapBoxes(scene, kind, NULL) == 0 && RaylibAMD_PlanOverlapBoxes(unfinished, kind, &p) == 0);
			CHECK(RaylibAMD_PlanOverlapBoxes(prims, kind, &p) == 0 && RaylibAMD_PlanOverlapBoxes(0, kind, &p) == 0);
		}
	}
	Raylib_DestroyScene(unfinished); Raylib_DestroyScene(scene); Raylib_DestroyScene(prims);
	RaylibAMD_DestroySceneElement(sphere); RaylibAMD_DestroyMaterial(m);
	printf("box_host_check: ok\n");
	return 0;
}
