// Sanitizer harness only (tools/host_check.sh nearest_all): a stand-alone program over the host side of RaylibAMD_NearestPointsAll -- the host oracle
// RaylibAMD_NearestPointsAllHost on heap arrays of exactly the sizes the contract names, every refusal, and the planner -- linked with tools/nodevice_stub.cc in
// place of the device units, so every accepted call of the plain and the device entry ends at "no device" (0).  Never part of libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "nearest_all_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static float Rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); }

int main()
{
	const float grey[3] = { 0.5f, 0.5f, 0.5f }, zero[3] = { 0, 0, 0 }, one[3] = { 1, 1, 1 }, up[3] = { 0, 1, 0 };
	MaterialHandle m = RaylibAMD_CreateMaterial(0, grey, 1.0f, 0.0f, zero, 1.5f, one, 0.0f);
	CHECK(m);
	// a soup of 300 triangles, each of them twice (exact ties between different indices)
	const int numTris = 600;
	std::vector<float> verts;
	SceneHandle scene = Raylib_CreateScene(), unfinished = Raylib_CreateScene();
	CHECK(scene && unfinished);
	{
		uint32_t s = 12345u;
		for (int k = 0; k < numTris / 2; ++k) {
			const float c[3] = { Rnd(s) * 8 - 4, Rnd(s) * 8 - 4, Rnd(s) * 8 - 4 };
			float p[9];
			for (int a = 0; a < 9; ++a) { p[a] = c[a % 3] + Rnd(s) * 1.6f - 0.8f; verts.push_back(p[a]); }
			for (int twin = 0; twin < 2; ++twin) {
				SceneElementHandle e = RaylibAMD_CreateTriangle(p, p + 3, p + 6, up, up, up, NULL, m);
				CHECK(e);
				Raylib_AddSceneElement(scene, e);
			}
		}
	}
	Raylib_FinalizeScene(scene);
	CHECK(RaylibAMD_SceneNumTriangles(scene) == numTris);

	SceneElementHandle sphere = RaylibAMD_CreateSphere(0, 0, 0, 0.5f, m);
	SceneHandle prims = Raylib_CreateScene();
	CHECK(sphere && prims);
	Raylib_AddSceneElement(prims, sphere);
	Raylib_FinalizeScene(prims);

	for (int n : { 0, 1, 7, 300 }) {
		// exactly n points, n * maxHits records and n counts, on the heap: the oracle may read and write nothing past them
		std::vector<RaylibAMDNearestQuery> q((size_t)n);
		uint32_t s = 99u + (uint32_t)n;
		for (int i = 0; i < n; ++i) {
			RaylibAMDNearestQuery& Q = q[(size_t)i];
			if (i % 3 == 0) for (int a = 0; a < 3; ++a) Q.pos[a] = verts[(size_t)(i % (numTris / 2)) * 9 + (size_t)a];   // a vertex: D = 0 twice
			else for (int a = 0; a < 3; ++a) Q.pos[a] = Rnd(s) * 10 - 5;
			Q.maxDist = i % 4 == 0 ? INFINITY : i % 4 == 1 ? 0.0f : i % 4 == 2 ? 1.5f : 4.0f;
			if (i == 5) Q.pos[1] = NAN;
			if (i == 6) Q.maxDist = -1.0f;
		}
		RaylibAMDNearestQuery* qp = n ? q.data() : NULL;
		std::vector<uint32_t> within((size_t)n, 7u);
		std::vector<RaylibAMDNearestHit> closest((size_t)n);
		CHECK(RaylibAMD_NearestPointsHost(scene, RAYLIB_AMD_NEAREST_WITHIN, qp, n, n ? within.data() : NULL) == 1);
		CHECK(RaylibAMD_NearestPointsHost(scene, RAYLIB_AMD_NEAREST_CLOSEST, qp, n, n ? closest.data() : NULL) == 1);
		for (int maxHits : { 1, 4, RAYLIB_AMD_MAX_NEAREST }) {
			const RaylibAMDNearestHit fill = { 7.0f, 7, 7.0f, 7.0f }, fill2 = { 9.0f, 9, 9.0f, 9.0f };
			std::vector<RaylibAMDNearestHit> rows((size_t)n * (size_t)maxHits, fill), rows2((size_t)n * (size_t)maxHits, fill2);
			std::vector<uint32_t> cnt((size_t)n, 7u);
			CHECK(RaylibAMD_NearestPointsAllHost(scene, qp, n, maxHits, n ? rows.data() : NULL, n ? cnt.data() : NULL) == 1);
			CHECK(RaylibAMD_NearestPointsAllHost(scene, qp, n, maxHits, n ? rows2.data() : NULL, NULL) == 1);
			CHECK(rows.empty() || memcmp(rows.data(), rows2.data(), rows.size() * sizeof(RaylibAMDNearestHit)) == 0);
			for (int i = 0; i < n; ++i) {
				const RaylibAMDNearestHit* row = &rows[(size_t)i * (size_t)maxHits];
				const uint32_t listed = cnt[(size_t)i] < (uint32_t)maxHits ? cnt[(size_t)i] : (uint32_t)maxHits;
				CHECK(cnt[(size_t)i] % 2u == 0u && cnt[(size_t)i] <= (uint32_t)numTris);
				for (uint32_t e = 0; e < (uint32_t)maxHits; ++e) {
					if (e < listed) {
						CHECK(row[e].prim >= 0 && row[e].prim < numTris && row[e].dist2 <= q[(size_t)i].maxDist * q[(size_t)i].maxDist);
						CHECK(e == 0 || row[e - 1].dist2 < row[e].dist2 || (row[e - 1].dist2 == row[e].dist2 && row[e - 1].prim < row[e].prim));
					} else CHECK(row[e].prim == -1 && row[e].dist2 == 0.0f && row[e].b1 == 0.0f && row[e].b2 == 0.0f);
				}
				CHECK(memcmp(&row[0], &closest[(size_t)i], sizeof(RaylibAMDNearestHit)) == 0);
				CHECK(within[(size_t)i] == (cnt[(size_t)i] ? 1u : 0u));
				if (i == 5 || i == 6) CHECK(cnt[(size_t)i] == 0);
				else if (i % 4 == 0) CHECK(cnt[(size_t)i] == (uint32_t)numTris);
				else if (i % 3 == 0) CHECK(cnt[(size_t)i] >= 2 && row[0].dist2 == 0.0f);
			}
			// accepted by the checks, then "no device" -- but no points are a success without one
			CHECK(RaylibAMD_NearestPointsAll(scene, qp, n, maxHits, n ? rows.data() : NULL, n ? cnt.data() : NULL) == 0);
			CHECK(RaylibAMD_NearestPointsAllDevice(scene, qp, n, maxHits, n ? rows.data() : NULL, n ? cnt.data() : NULL, NULL) == 0);
		}
		// the refusals write nothing
		std::vector<uint32_t> out((size_t)n * 16 + 4, 7u), cnt((size_t)n + 1, 7u);
		RaylibAMDNearestHit* op = (RaylibAMDNearestHit*)out.data();
		typedef int32_t (*Entry)(SceneHandle, const RaylibAMDNearestQuery*, int32_t, int32_t, RaylibAMDNearestHit*, uint32_t*);
		for (Entry f : { (Entry)RaylibAMD_NearestPointsAllHost, (Entry)RaylibAMD_NearestPointsAll }) {
			CHECK(f(scene, qp, n, 0, op, cnt.data()) == 0 && f(scene, qp, n, -1, op, cnt.data()) == 0 && f(scene, qp, n, RAYLIB_AMD_MAX_NEAREST + 1, op, cnt.data()) == 0);
			CHECK(f(scene, qp, 0x7fffffff, 2, op, cnt.data()) == 0 && f(scene, qp, 1 << 27, 16, op, cnt.data()) == 0);
			CHECK(f(scene, qp, -1, 4, op, cnt.data()) == 0);
			CHECK(f(unfinished, qp, n, 4, op, cnt.data()) == 0 && f(prims, qp, n, 4, op, cnt.data()) == 0);
			CHECK(f(0, qp, n, 4, op, cnt.data()) == 0);
			if (n) CHECK(f(scene, NULL, n, 4, op, cnt.data()) == 0 && f(scene, qp, n, 4, NULL, cnt.data()) == 0);
		}
		CHECK(RaylibAMD_NearestPointsAllDevice(prims, qp, n, 4, op, cnt.data(), NULL) == 0 && RaylibAMD_NearestPointsAllDevice(scene, qp, n, 0, op, cnt.data(), NULL) == 0);
		for (uint32_t v : out) CHECK(v == 7u);
		for (uint32_t v : cnt) CHECK(v == 7u);
	}
	// the planner
	for (int wantCount : { 0, 1 }) {
		for (const char* env : { "", "2", "4", "8" }) {
			if (*env) setenv("RAYLIB_QUERY_TREE", env, 1); else unsetenv("RAYLIB_QUERY_TREE");
			RaylibAMDQueryPlan p, c;
			for (int maxHits : { 1, 4, RAYLIB_AMD_MAX_NEAREST }) {
				CHECK(RaylibAMD_PlanNearestAll(scene, maxHits, wantCount, &p) == 1 && RaylibAMD_PlanNearest(scene, RAYLIB_AMD_NEAREST_CLOSEST, &c) == 1);
				CHECK((p.treeWidth == 2 || p.treeWidth == 4) && (p.stack == 32 || p.stack == 64) && p.prims == 0 && p.early == 0);
				CHECK(p.tree == c.tree && p.treeWidth == c.treeWidth && p.nodeBytes == c.nodeBytes && p.stack == c.stack);
				if (env[0] == '2') CHECK(p.treeWidth == 2);
			}
			CHECK(RaylibAMD_PlanNearestAll(scene, 0, wantCount, &p) == 0 && RaylibAMD_PlanNearestAll(scene, RAYLIB_AMD_MAX_NEAREST + 1, wantCount, &p) == 0);
			CHECK(RaylibAMD_PlanNearestAll(scene, 4, wantCount, NULL) == 0 && RaylibAMD_PlanNearestAll(unfinished, 4, wantCount, &p) == 0);
			CHECK(RaylibAMD_PlanNearestAll(prims, 4, wantCount, &p) == 0 && RaylibAMD_PlanNearestAll(0, 4, wantCount, &p) == 0);
		}
	}
	Raylib_DestroyScene(unfinished); Raylib_DestroyScene(scene); Raylib_DestroyScene(prims);
	RaylibAMD_DestroySceneElement(sphere); RaylibAMD_DestroyMaterial(m);
	printf("nearest_all_host_check: ok\n");
	return 0;
}
