// Sanitizer harness only (tools/host_check.sh overlap): a stand-alone program over the host side of RaylibAMD_OverlapTriangles -- the host oracle
// RaylibAMD_OverlapTrianglesHost on heap arrays of exactly the sizes the contract names, every refusal, and the planner -- linked with tools/nodevice_stub.cc in
// place of the device units, so every accepted call of the plain and the device entry ends at "no device" (0).  Never part of libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "overlap_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static float Rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); }

int main()
{
	const float grey[3] = { 0.5f, 0.5f, 0.5f }, zero[3] = { 0, 0, 0 }, one[3] = { 1, 1, 1 }, up[3] = { 0, 1, 0 };
	MaterialHandle m = RaylibAMD_CreateMaterial(0, grey, 1.0f, 0.0f, zero, 1.5f, one, 0.0f);
	CHECK(m);
	// a soup of 300 triangles (the elements live as long as the program)
	const int numTris = 300;
	std::vector<float> verts;
	SceneHandle scene = Raylib_CreateScene(), unfinished = Raylib_CreateScene();
	CHECK(scene && unfinished);
	{
		uint32_t s = 12345u;
		for (int k = 0; k < numTris; ++k) {
			const float c[3] = { Rnd(s) * 8 - 4, Rnd(s) * 8 - 4, Rnd(s) * 8 - 4 };
			float p[9];
			for (int a = 0; a < 9; ++a) { p[a] = c[a % 3] + Rnd(s) * 1.6f - 0.8f; verts.push_back(p[a]); }
			SceneElementHandle e = RaylibAMD_CreateTriangle(p, p + 3, p + 6, up, up, up, NULL, m);
			CHECK(e);
			Raylib_AddSceneElement(scene, e);
		}
	}
	Raylib_FinalizeScene(scene);
	CHECK(RaylibAMD_SceneNumTriangles(scene) == numTris);
	// (queries of the scene's own triangles meet themselves only if the export order holds their vertices as given)
	{
		std::vector<float> exported((size_t)numTris * 26);
		RaylibAMD_SceneExportTriangles(scene, exported.data());
		for (int k = 0; k < numTris; ++k) CHECK(memcmp(&exported[(size_t)k * 26], &verts[(size_t)k * 9], 9 * sizeof(float)) == 0);
	}

	SceneElementHandle sphere = RaylibAMD_CreateSphere(0, 0, 0, 0.5f, m);
	SceneHandle prims = Raylib_CreateScene();
	CHECK(sphere && prims);
	Raylib_AddSceneElement(prims, sphere);
	Raylib_FinalizeScene(prims);

	for (int n : { 0, 1, 7, 300 }) {
		// exactly n records, n * maxHits words and n counts, on the heap: the oracle may read and write nothing past them
		std::vector<RaylibAMDOverlapQuery> q((size_t)n);
		uint32_t s = 99u + (uint32_t)n;
		for (int i = 0; i < n; ++i) {
			RaylibAMDOverlapQuery& Q = q[(size_t)i];
			memset(&Q, 0xff, sizeof(Q));   // (the reserved words are not read)
			if (i % 3 == 0) {   // a scene triangle itself
				const float* p = &verts[(size_t)(i % numTris) * 9];
				for (int a = 0; a < 3; ++a) { Q.v0[a] = p[a]; Q.v1[a] = p[3 + a]; Q.v2[a] = p[6 + a]; }
			} else {
				const float size = i % 3 == 1 ? 1.0f : 12.0f;
				const float c[3] = { Rnd(s) * 8 - 4, Rnd(s) * 8 - 4, Rnd(s) * 8 - 4 };
				for (int a = 0; a < 3; ++a) { Q.v0[a] = c[a] + (Rnd(s) - 0.5f) * size; Q.v1[a] = c[a] + (Rnd(s) - 0.5f) * size; Q.v2[a] = c[a] + (Rnd(s) - 0.5f) * size; }
			}
			if (i == 5) Q.v1[1] = NAN;
			if (i == 6) Q.v2[0] = 1e30f;
		}
		RaylibAMDOverlapQuery* qp = n ? q.data() : NULL;
		for (uint32_t flags : { 0u, RAYLIB_AMD_OVERLAP_SKIP_SHARED }) {
			std::vector<uint32_t> any((size_t)n, 7u);
			CHECK(RaylibAMD_OverlapTrianglesHost(scene, RAYLIB_AMD_OVERLAP_ANY, flags, qp, n, 12345, n ? any.data() : NULL, NULL) == 1);
			for (int maxHits : { 1, 4, RAYLIB_AMD_MAX_OVERLAPS }) {
				std::vector<int32_t> rows((size_t)n * (size_t)maxHits, 7);
				std::vector<uint32_t> cnt((size_t)n, 7u);
				CHECK(RaylibAMD_OverlapTrianglesHost(scene, RAYLIB_AMD_OVERLAP_LIST, flags, qp, n, maxHits, n ? rows.data() : NULL, n ? cnt.data() : NULL) == 1);
				std::vector<int32_t> rows2((size_t)n * (size_t)maxHits, 7);
				CHECK(RaylibAMD_OverlapTrianglesHost(scene, RAYLIB_AMD_OVERLAP_LIST, flags, qp, n, maxHits, n ? rows2.data() : NULL, NULL) == 1);
				CHECK(rows == rows2);
				for (int i = 0; i < n; ++i) {
					const int32_t* row = &rows[(size_t)i * (size_t)maxHits];
					const uint32_t listed = cnt[(size_t)i] < (uint32_t)maxHits ? cnt[(size_t)i] : (uint32_t)maxHits;
					for (uint32_t e = 0; e < (uint32_t)maxHits; ++e) {
						if (e < listed) CHECK(row[e] >= 0 && row[e] < numTris && (e == 0 || row[e - 1] < row[e]));
						else CHECK(row[e] == -1);
					}
					CHECK(any[(size_t)i] == (cnt[(size_t)i] ? 1u : 0u));
					if (i == 5) CHECK(cnt[(size_t)i] == 0);
					if (i % 3 == 0 && i != 5 && i != 6) CHECK(flags ? true : cnt[(size_t)i] >= 1);
				}
				// accepted by the checks, then "no device" -- but no queries are a success without one
				CHECK(RaylibAMD_OverlapTriangles(scene, RAYLIB_AMD_OVERLAP_LIST, flags, qp, n, maxHits, n ? rows.data() : NULL, n ? cnt.data() : NULL) == 0);
				CHECK(RaylibAMD_OverlapTrianglesDevice(scene, RAYLIB_AMD_OVERLAP_LIST, flags, qp, n, maxHits, n ? rows.data() : NULL, n ? cnt.data() : NULL, NULL) == 0);
			}
		}
		// the refusals write nothing
		std::vector<int32_t> out((size_t)n * 4 + 1, 7);
		std::vector<uint32_t> cnt((size_t)n + 1, 7u);
		typedef int32_t (*Entry)(SceneHandle, int32_t, uint32_t, const RaylibAMDOverlapQuery*, int32_t, int32_t, void*, uint32_t*);
		for (Entry f : { (Entry)RaylibAMD_OverlapTrianglesHost, (Entry)RaylibAMD_OverlapTriangles }) {
			CHECK(f(scene, 2, 0, qp, n, 4, out.data(), NULL) == 0 && f(scene, -1, 0, qp, n, 4, out.data(), NULL) == 0);
			CHECK(f(scene, RAYLIB_AMD_OVERLAP_LIST, 2u, qp, n, 4, out.data(), cnt.data()) == 0 && f(scene, RAYLIB_AMD_OVERLAP_ANY, 0x80000000u, qp, n, 4, out.data(), NULL) == 0);
			CHECK(f(scene, RAYLIB_AMD_OVERLAP_LIST, 0, qp, n, 0, out.data(), cnt.data()) == 0 && f(scene, RAYLIB_AMD_OVERLAP_LIST, 0, qp, n, RAYLIB_AMD_MAX_OVERLAPS + 1, out.data(), cnt.data()) == 0);
			CHECK(f(scene, RAYLIB_AMD_OVERLAP_LIST, 0, qp, 0x7fffffff, 2, out.data(), cnt.data()) == 0);
			CHECK(f(scene, RAYLIB_AMD_OVERLAP_ANY, 0, qp, n, 4, out.data(), cnt.data()) == 0);
			CHECK(f(scene, RAYLIB_AMD_OVERLAP_LIST, 0, qp, -1, 4, out.data(), cnt.data()) == 0);
			CHECK(f(unfinished, RAYLIB_AMD_OVERLAP_LIST, 0, qp, n, 4, out.data(), cnt.data()) == 0 && f(prims, RAYLIB_AMD_OVERLAP_LIST, 0, qp, n, 4, out.data(), cnt.data()) == 0);
			CHECK(f(0, RAYLIB_AMD_OVERLAP_LIST, 0, qp, n, 4, out.data(), cnt.data()) == 0);
			if (n) CHECK(f(scene, RAYLIB_AMD_OVERLAP_LIST, 0, NULL, n, 4, out.data(), cnt.data()) == 0 && f(scene, RAYLIB_AMD_OVERLAP_LIST, 0, qp, n, 4, NULL, cnt.data()) == 0);
		}
		for (int32_t v : out) CHECK(v == 7);
		for (uint32_t v : cnt) CHECK(v == 7u);
	}
	// the planner
	for (int kind : { RAYLIB_AMD_OVERLAP_ANY, RAYLIB_AMD_OVERLAP_LIST }) {
		for (const char* env : { "", "2", "4", "8" }) {
			if (*env) setenv("RAYLIB_QUERY_TREE", env, 1); else unsetenv("RAYLIB_QUERY_TREE");
			RaylibAMDQueryPlan p;
			CHECK(RaylibAMD_PlanOverlap(scene, kind, &p) == 1);
			CHECK((p.treeWidth == 2 || p.treeWidth == 4) && (p.stack == 32 || p.stack == 64) && p.prims == 0 && p.early == (kind == RAYLIB_AMD_OVERLAP_ANY));
			if (env[0] == '2') CHECK(p.treeWidth == 2);
			CHECK(RaylibAMD_PlanOverlap(scene, 2, &p) == 0 && RaylibAMD_PlanOverlap(scene, kind, NULL) == 0 && RaylibAMD_PlanOverlap(unfinished, kind, &p) == 0);
			CHECK(RaylibAMD_PlanOverlap(prims, kind, &p) == 0 && RaylibAMD_PlanOverlap(0, kind, &p) == 0);
		}
	}
	Raylib_DestroyScene(unfinished); Raylib_DestroyScene(scene); Raylib_DestroyScene(prims);
	RaylibAMD_DestroySceneElement(sphere); RaylibAMD_DestroyMaterial(m);
	printf("overlap_host_check: ok\n");
	return 0;
}
