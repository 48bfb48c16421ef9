// Sanitizer harness only (tools/host_check.sh contact): a stand-alone program over the host side of RaylibAMD_OverlapContacts -- the host oracle
// RaylibAMD_OverlapContactsHost on heap arrays of exactly the sizes the contract names, every refusal, and the planner -- linked with tools/nodevice_stub.cc in
// place of the device units, so every accepted call of the plain and the device entry ends at "no device" (0).  Never part of libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "contact_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

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
		// exactly n queries, n * maxHits words, n * maxHits records and n counts, on the heap: the oracle may read and write nothing past them
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
		size_t kinds[4] = { 0, 0, 0, 0 };
		for (uint32_t flags : { 0u, RAYLIB_AMD_OVERLAP_SKIP_SHARED }) {
			for (int maxHits : { 1, 3, RAYLIB_AMD_MAX_OVERLAPS }) {
				const size_t cells = (size_t)n * (size_t)maxHits;
				std::vector<int32_t> rows(cells, 7), listRows(cells, 7);
				std::vector<RaylibAMDContact> recs(cells), recs2(cells);
				if (cells) { memset(recs.data(), 0x7f, cells * sizeof(RaylibAMDContact)); memset(recs2.data(), 0x7f, cells * sizeof(RaylibAMDContact)); }
				std::vector<uint32_t> cnt((size_t)n, 7u), listCnt((size_t)n, 7u);
				CHECK(RaylibAMD_OverlapContactsHost(scene, flags, qp, n, maxHits, n ? rows.data() : NULL, n ? recs.data() : NULL, n ? cnt.data() : NULL) == 1);
				// the rows and counts are LIST's
				CHECK(RaylibAMD_OverlapTrianglesHost(scene, RAYLIB_AMD_OVERLAP_LIST, flags, qp, n, maxHits, n ? listRows.data() : NULL, n ? listCnt.data() : NULL) == 1);
				CHECK(rows == listRows && cnt == listCnt);
				// the records do not depend on outCount
				std::vector<int32_t> rows2(cells, 7);
				CHECK(RaylibAMD_OverlapContactsHost(scene, flags, qp, n, maxHits, n ? rows2.data() : NULL, n ? recs2.data() : NULL, NULL) == 1);
				CHECK(rows == rows2 && (cells == 0 || memcmp(recs.data(), recs2.data(), cells * sizeof(RaylibAMDContact)) == 0));
				for (size_t c = 0; c < cells; ++c) {
					const RaylibAMDContact& R = recs[c];
					static const RaylibAMDContact none = { { 0, 0, 0 }, 0, { 0, 0, 0 }, 0 };
					CHECK(R.kind <= RAYLIB_AMD_CONTACT_NO_CROSSING);
					++kinds[R.kind];
					CHECK((R.kind == RAYLIB_AMD_CONTACT_NONE) == (rows[c] < 0));
					if (R.kind == RAYLIB_AMD_CONTACT_NONE) CHECK(memcmp(&R, &none, sizeof(R)) == 0);
					else if (R.kind == RAYLIB_AMD_CONTACT_NO_CROSSING) { RaylibAMDContact w = none; w.kind = RAYLIB_AMD_CONTACT_NO_CROSSING; CHECK(memcmp(&R, &w, sizeof(R)) == 0); }
					else {
						const uint32_t f0 = R.features & 0xffu, f1 = R.features >> 8;
						CHECK(f0 <= 5u && f1 <= 5u);
						for (int a = 0; a < 3; ++a) CHECK(isfinite(R.p0[a]) && isfinite(R.p1[a]));
					}
				}
				// accepted by the checks, then "no device" -- but no queries are a success without one
				const int32_t want = 0;
				CHECK(RaylibAMD_OverlapContacts(scene, flags, qp, n, maxHits, n ? rows.data() : NULL, n ? recs.data() : NULL, n ? cnt.data() : NULL) == want);
				CHECK(RaylibAMD_OverlapContactsDevice(scene, flags, qp, n, maxHits, n ? rows.data() : NULL, n ? recs.data() : NULL, n ? cnt.data() : NULL, NULL) == want);
			}
		}
		if (n == 300) CHECK(kinds[RAYLIB_AMD_CONTACT_NONE] && kinds[RAYLIB_AMD_CONTACT_SEGMENT] && kinds[RAYLIB_AMD_CONTACT_NO_CROSSING]);   // (a triangle against itself is coplanar)
		// the refusals write nothing
		std::vector<int32_t> out((size_t)n * 4 + 1, 7);
		std::vector<RaylibAMDContact> rec((size_t)n * 4 + 1);
		memset(rec.data(), 0x7f, rec.size() * sizeof(RaylibAMDContact));
		std::vector<uint32_t> cnt((size_t)n + 1, 7u);
		typedef int32_t (*Entry)(SceneHandle, uint32_t, const RaylibAMDOverlapQuery*, int32_t, int32_t, int32_t*, RaylibAMDContact*, uint32_t*);
		for (Entry f : { (Entry)RaylibAMD_OverlapContactsHost, (Entry)RaylibAMD_OverlapContacts }) {
			CHECK(f(scene, 2u, qp, n, 4, out.data(), rec.data(), cnt.data()) == 0 && f(scene, 0x80000000u, qp, n, 4, out.data(), rec.data(), NULL) == 0);
			CHECK(f(scene, 0, qp, n, 0, out.data(), rec.data(), cnt.data()) == 0 && f(scene, 0, qp, n, RAYLIB_AMD_MAX_OVERLAPS + 1, out.data(), rec.data(), cnt.data()) == 0);
			CHECK(f(scene, 0, qp, 0x7fffffff, 2, out.data(), rec.data(), cnt.data()) == 0);
			CHECK(f(scene, 0, qp, -1, 4, out.data(), rec.data(), cnt.data()) == 0);
			CHECK(f(unfinished, 0, qp, n, 4, out.data(), rec.data(), cnt.data()) == 0 && f(prims, 0, qp, n, 4, out.data(), rec.data(), cnt.data()) == 0);
			CHECK(f(0, 0, qp, n, 4, out.data(), rec.data(), cnt.data()) == 0);
			if (n) CHECK(f(scene, 0, NULL, n, 4, out.data(), rec.data(), cnt.data()) == 0 && f(scene, 0, qp, n, 4, NULL, rec.data(), cnt.data()) == 0 &&
			             f(scene, 0, qp, n, 4, out.data(), NULL, cnt.data()) == 0);
		}
		if (n) CHECK(RaylibAMD_OverlapContactsDevice(scene, 0, qp, n, 4, out.data(), NULL, cnt.data(), NULL) == 0);
		// RaylibAMD_OverlapTriangles has no third kind
		CHECK(RaylibAMD_OverlapTrianglesHost(scene, 2, 0, qp, n, 4, out.data(), NULL) == 0);
		for (int32_t v : out) CHECK(v == 7);
		for (const RaylibAMDContact& R : rec) { const unsigned char* b = (const unsigned char*)&R; for (size_t k = 0; k < sizeof(R); ++k) CHECK(b[k] == 0x7f); }
		for (uint32_t v : cnt) CHECK(v == 7u);
	}
	// the planner: RaylibAMD_PlanOverlap's answer for LIST
	for (const char* env : { "", "2", "4", "8" }) {
		if (*env) setenv("RAYLIB_QUERY_TREE", env, 1); else unsetenv("RAYLIB_QUERY_TREE");
		RaylibAMDQueryPlan p, l;
		CHECK(RaylibAMD_PlanOverlapContacts(scene, &p) == 1 && RaylibAMD_PlanOverlap(scene, RAYLIB_AMD_OVERLAP_LIST, &l) == 1);
		CHECK(memcmp(&p, &l, sizeof(p)) == 0 && p.early == 0 && p.prims == 0);
		if (env[0] == '2') CHECK(p.treeWidth == 2);
		CHECK(RaylibAMD_PlanOverlapContacts(scene, NULL) == 0 && RaylibAMD_PlanOverlapContacts(unfinished, &p) == 0);
		CHECK(RaylibAMD_PlanOverlapContacts(prims, &p) == 0 && RaylibAMD_PlanOverlapContacts(0, &p) == 0);
	}
	Raylib_DestroyScene(unfinished); Raylib_DestroyScene(scene); Raylib_DestroyScene(prims);
	RaylibAMD_DestroySceneElement(sphere); RaylibAMD_DestroyMaterial(m);
	printf("contact_host_check: ok\n");
	return 0;
}
