// Sanitizer harness only (tools/host_check.sh sweep): a stand-alone program over the host side of RaylibAMD_SweepSpheres -- the host oracle
// RaylibAMD_SweepSpheresHost on heap arrays of exactly the sizes the contract names, every refusal, and the planner -- linked with tools/nodevice_stub.cc in
// place of the device units, so every accepted call of the plain and the device entry ends at "no device" (0).  Never part of libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "sweep_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static float Rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); }

int main()
{
	const float grey[3] = { 0.5f, 0.5f, 0.5f }, zero[3] = { 0, 0, 0 }, one[3] = { 1, 1, 1 }, up[3] = { 0, 1, 0 };
	MaterialHandle m = RaylibAMD_CreateMaterial(0, grey, 1.0f, 0.0f, zero, 1.5f, one, 0.0f);
	CHECK(m);
	// a soup of 300 triangles (the elements live as long as the program), one of them degenerate
	const int numTris = 300;
	std::vector<float> verts;
	SceneHandle scene = Raylib_CreateScene(), unfinished = Raylib_CreateScene();
	CHECK(scene && unfinished);
	{
		uint32_t s = 12345u;
		for (int k = 0; k < numTris; ++k) {
			const float c[3] = { Rnd(s) * 8 - 4, Rnd(s) * 8 - 4, Rnd(s) * 8 - 4 };
			float p[9];
			for (int a = 0; a < 9; ++a) p[a] = c[a % 3] + Rnd(s) * 1.6f - 0.8f;
			if (k == 17) for (int a = 3; a < 9; ++a) p[a] = p[a % 3];   // a point
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

	for (int n : { 0, 1, 7, 300 }) {
		// exactly n queries and n results, on the heap: the oracle may read and write nothing past them
		std::vector<RaylibAMDSweepQuery> q((size_t)n);
		uint32_t s = 99u + (uint32_t)n;
		for (int i = 0; i < n; ++i) {
			RaylibAMDSweepQuery& Q = q[(size_t)i];
			memset(&Q, 0xff, sizeof(Q));   // (the reserved word is not read)
			const float* p = &verts[(size_t)(i % numTris) * 9];
			for (int a = 0; a < 3; ++a) {
				Q.origin[a] = i % 3 == 0 ? p[a] : Rnd(s) * 10 - 5;
				Q.delta[a] = i % 4 == 0 ? 0.0f : (Rnd(s) - 0.5f) * (i % 5 == 0 ? 20.0f : 1.0f);
			}
			Q.radius = i % 7 == 0 ? 0.0f : Rnd(s) * 0.8f;
			if (i == 5) Q.delta[1] = NAN;
			if (i == 6) Q.origin[0] = 1e30f;
			if (i == 8) Q.radius = -1.0f;
			if (i == 9) Q.delta[2] = 1e-42f;
			if (i == 10) Q.radius = INFINITY;
		}
		RaylibAMDSweepQuery* qp = n ? q.data() : NULL;
		std::vector<uint32_t> any((size_t)n, 7u);
		std::vector<RaylibAMDSweepHit> hit((size_t)n);
		if (n) memset(hit.data(), 0x5a, hit.size() * sizeof(RaylibAMDSweepHit));
		CHECK(RaylibAMD_SweepSpheresHost(scene, RAYLIB_AMD_SWEEP_ANY, qp, n, n ? any.data() : NULL) == 1);
		CHECK(RaylibAMD_SweepSpheresHost(scene, RAYLIB_AMD_SWEEP_CLOSEST, qp, n, n ? hit.data() : NULL) == 1);
		int hits = 0;
		for (int i = 0; i < n; ++i) {
			const RaylibAMDSweepHit& H = hit[(size_t)i];
			CHECK(any[(size_t)i] == (H.prim >= 0 ? 1u : 0u));
			CHECK(H.reserved0 == 0u && H.reserved1 == 0u);
			if (H.prim >= 0) { CHECK(H.prim < numTris && H.t >= 0.0f && H.t <= 1.0f && H.feature >= 0 && H.feature <= 7); ++hits; }
			else CHECK(H.t == 0.0f && H.feature == 0 && H.point[0] == 0.0f && H.point[1] == 0.0f && H.point[2] == 0.0f);
			if (i == 5 || i == 6 || i == 8 || i == 10) CHECK(H.prim == -1);
			if (i % 3 == 0 && i != 6) CHECK(H.prim >= 0 && H.t == 0.0f && H.feature == 7);   // the origin is a vertex of the scene
		}
		if (n == 300) CHECK(hits > 100 && hits < 300);
		// accepted by the checks, then "no device"
		CHECK(RaylibAMD_SweepSpheres(scene, RAYLIB_AMD_SWEEP_CLOSEST, qp, n, n ? hit.data() : NULL) == 0);
		CHECK(RaylibAMD_SweepSpheresDevice(scene, RAYLIB_AMD_SWEEP_ANY, qp, n, n ? any.data() : NULL, NULL) == 0);
		// the refusals write nothing
		std::vector<uint32_t> out((size_t)n * 8 + 1, 7u);
		typedef int32_t (*Entry)(SceneHandle, int32_t, const RaylibAMDSweepQuery*, int32_t, void*);
		for (Entry f : { (Entry)RaylibAMD_SweepSpheresHost, (Entry)RaylibAMD_SweepSpheres }) {
			CHECK(f(scene, 2, qp, n, out.data()) == 0 && f(scene, -1, qp, n, out.data()) == 0);
			CHECK(f(scene, RAYLIB_AMD_SWEEP_CLOSEST, qp, -1, out.data()) == 0);
			CHECK(f(unfinished, RAYLIB_AMD_SWEEP_CLOSEST, qp, n, out.data()) == 0 && f(prims, RAYLIB_AMD_SWEEP_ANY, qp, n, out.data()) == 0);
			CHECK(f(0, RAYLIB_AMD_SWEEP_CLOSEST, qp, n, out.data()) == 0);
			if (n) CHECK(f(scene, RAYLIB_AMD_SWEEP_CLOSEST, NULL, n, out.data()) == 0 && f(scene, RAYLIB_AMD_SWEEP_CLOSEST, qp, n, NULL) == 0);
		}
		for (uint32_t v : out) CHECK(v == 7u);
	}
	CHECK(RaylibAMD_SweepSpheresHost(scene, RAYLIB_AMD_SWEEP_CLOSEST, NULL, 0, NULL) == 1);
	// the planner
	for (int kind : { RAYLIB_AMD_SWEEP_ANY, RAYLIB_AMD_SWEEP_CLOSEST }) {
		for (const char* env : { "", "2", "4", "8" }) {
			if (*env) setenv("RAYLIB_QUERY_TREE", env, 1); else unsetenv("RAYLIB_QUERY_TREE");
			RaylibAMDQueryPlan p, pn;
			CHECK(RaylibAMD_PlanSweep(scene, kind, &p) == 1 && RaylibAMD_PlanNearest(scene, RAYLIB_AMD_NEAREST_CLOSEST, &pn) == 1);
			CHECK((p.treeWidth == 2 || p.treeWidth == 4) && (p.stack == 32 || p.stack == 64) && p.prims == 0 && p.early == (kind == RAYLIB_AMD_SWEEP_ANY));
			CHECK(p.tree == pn.tree && p.treeWidth == pn.treeWidth && p.stack == pn.stack && p.nodeBytes == pn.nodeBytes);
			if (env[0] == '2') CHECK(p.treeWidth == 2);
			CHECK(RaylibAMD_PlanSweep(scene, 2, &p) == 0 && RaylibAMD_PlanSweep(scene, kind, NULL) == 0 && RaylibAMD_PlanSweep(unfinished, kind, &p) == 0);
			CHECK(RaylibAMD_PlanSweep(prims, kind, &p) == 0 && RaylibAMD_PlanSweep(0, kind, &p) == 0);
		}
	}
	Raylib_DestroyScene(unfinished); Raylib_DestroyScene(scene); Raylib_DestroyScene(prims);
	RaylibAMD_DestroySceneElement(sphere); RaylibAMD_DestroyMaterial(m);
	printf("sweep_host_check: ok\n");
	return 0;
}
