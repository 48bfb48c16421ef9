// Sanitizer harness only (tools/host_check.sh sdf): a stand-alone program over the host side of RaylibAMD_BakeDistanceField -- the host oracle
// RaylibAMD_BakeDistanceFieldHost on heap arrays of exactly nx * ny * nz words, every refusal of statement V7 that needs no device, and the planner -- linked
// with tools/nodevice_stub.cc in place of the device units, so every accepted call of the plain and the device entry ends at "no device" (0).  Never part of
// libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "sdf_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static RaylibAMDDistanceFieldParams Grid(float lo, float size, int nx, int ny, int nz, float maxDist, int sign)
{
	RaylibAMDDistanceFieldParams p;
	const int n[3] = { nx, ny, nz };
	for (int a = 0; a < 3; ++a) { p.dims[a] = n[a]; p.spacing[a] = size / (float)(n[a] > 0 ? n[a] : 1); p.origin[a] = lo + 0.37f * p.spacing[a]; }
	p.maxDist = maxDist; p.sign = sign;
	return p;
}

int main()
{
	const float grey[3] = { 0.5f, 0.5f, 0.5f }, zero[3] = { 0, 0, 0 }, one[3] = { 1, 1, 1 }, up[3] = { 0, 1, 0 };
	MaterialHandle m = RaylibAMD_CreateMaterial(0, grey, 1.0f, 0.0f, zero, 1.5f, one, 0.0f);
	CHECK(m);
	// an octahedron subdivided once towards the unit sphere: 32 triangles, closed
	SceneHandle scene = Raylib_CreateScene(), unfinished = Raylib_CreateScene();
	CHECK(scene && unfinished);
	int numTris = 0;
	for (int sx = -1; sx <= 1; sx += 2) for (int sy = -1; sy <= 1; sy += 2) for (int sz = -1; sz <= 1; sz += 2) {
		const float A[3] = { (float)sx, 0, 0 }, B[3] = { 0, (float)sy, 0 }, Cc[3] = { 0, 0, (float)sz };
		float ab[3], bc[3], ca[3];
		const float* src[3][2] = { { A, B }, { B, Cc }, { Cc, A } };
		float* mid[3] = { ab, bc, ca };
		for (int k = 0; k < 3; ++k) {
			float len = 0;
			for (int a = 0; a < 3; ++a) { mid[k][a] = 0.5f * (src[k][0][a] + src[k][1][a]); len += mid[k][a] * mid[k][a]; }
			for (int a = 0; a < 3; ++a) mid[k][a] /= sqrtf(len);
		}
		const float* tris[4][3] = { { A, ab, ca }, { ab, B, bc }, { ca, bc, Cc }, { ab, bc, ca } };
		for (int t = 0; t < 4; ++t) {
			SceneElementHandle e = RaylibAMD_CreateTriangle(tris[t][0], tris[t][1], tris[t][2], up, up, up, NULL, m);
			CHECK(e);
			Raylib_AddSceneElement(scene, e);
			++numTris;
		}
	}
	Raylib_FinalizeScene(scene);
	CHECK(RaylibAMD_SceneNumTriangles(scene) == numTris && numTris == 32);

	SceneElementHandle sphere = RaylibAMD_CreateSphere(0, 0, 0, 0.5f, m);
	SceneHandle prims = Raylib_CreateScene();
	CHECK(sphere && prims);
	Raylib_AddSceneElement(prims, sphere);
	Raylib_FinalizeScene(prims);

	const int dims[][3] = { { 1, 1, 1 }, { 9, 7, 5 }, { 33, 3, 2 }, { 2, 3, 33 } };
	for (const int* d : dims) {
		const size_t voxels = (size_t)d[0] * d[1] * d[2];
		std::vector<float> unsignedDist(voxels, 7.0f);
		for (float maxDist : { INFINITY, 0.3f, 0.0f }) {
			for (int sign = RAYLIB_AMD_SDF_UNSIGNED; sign <= RAYLIB_AMD_SDF_SIGN_MAJORITY; ++sign) {
				// exactly nx * ny * nz words each, on the heap: the oracle may write nothing past them
				const RaylibAMDDistanceFieldParams p = Grid(-1.4f, 2.8f, d[0], d[1], d[2], maxDist, sign);
				std::vector<float> dist(voxels, 7.0f), dist2(voxels, 9.0f);
				std::vector<int32_t> prim(voxels, 7);
				CHECK(RaylibAMD_BakeDistanceFieldHost(scene, &p, dist.data(), prim.data()) == 1);
				CHECK(RaylibAMD_BakeDistanceFieldHost(scene, &p, dist2.data(), NULL) == 1);
				CHECK(memcmp(dist.data(), dist2.data(), voxels * sizeof(float)) == 0);
				if (sign == RAYLIB_AMD_SDF_UNSIGNED) unsignedDist = dist;
				size_t negative = 0;
				for (size_t v = 0; v < voxels; ++v) {
					CHECK(fabsf(dist[v]) == unsignedDist[v] && !(sign == RAYLIB_AMD_SDF_UNSIGNED && signbit(dist[v])));
					CHECK(prim[v] >= -1 && prim[v] < numTris && (prim[v] >= 0 ? fabsf(dist[v]) <= maxDist : fabsf(dist[v]) == maxDist));
					negative += signbit(dist[v]) ? 1u : 0u;
				}
				if (sign != RAYLIB_AMD_SDF_UNSIGNED && voxels > 100) CHECK(negative > 0 && negative < voxels / 2);
				// accepted by the checks, then "no device"
				CHECK(RaylibAMD_BakeDistanceField(scene, &p, dist.data(), prim.data()) == 0);
				CHECK(RaylibAMD_BakeDistanceFieldDevice(scene, &p, dist.data(), prim.data(), NULL) == 0);
			}
		}
	}
	// the refusals write nothing
	{
		std::vector<uint32_t> out(64 + 4, 7u), prim(64 + 4, 7u);
		float* op = (float*)out.data(); int32_t* pp = (int32_t*)prim.data();
		const RaylibAMDDistanceFieldParams good = Grid(-1.0f, 2.0f, 4, 4, 4, INFINITY, RAYLIB_AMD_SDF_SIGN_MAJORITY);
		std::vector<RaylibAMDDistanceFieldParams> bad;
		{ RaylibAMDDistanceFieldParams p = good; p.dims[1] = 0; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.dims[2] = -3; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.dims[0] = 2048; p.dims[1] = 2048; p.dims[2] = 512; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.dims[0] = p.dims[1] = p.dims[2] = 0x7fffffff; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.spacing[0] = 0.0f; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.spacing[1] = -1.0f; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.spacing[2] = INFINITY; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.spacing[2] = NAN; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.origin[0] = NAN; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.origin[1] = -INFINITY; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.origin[0] = 3e38f; p.spacing[0] = 1e37f; p.dims[0] = 16; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.maxDist = NAN; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.maxDist = -1.0f; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.sign = 5; bad.push_back(p); }
		{ RaylibAMDDistanceFieldParams p = good; p.sign = -1; bad.push_back(p); }
		typedef int32_t (*Entry)(SceneHandle, const RaylibAMDDistanceFieldParams*, float*, int32_t*);
		RaylibAMDQueryPlan a, b;
		for (Entry f : { (Entry)RaylibAMD_BakeDistanceFieldHost, (Entry)RaylibAMD_BakeDistanceField }) {
			for (const RaylibAMDDistanceFieldParams& p : bad) CHECK(f(scene, &p, op, pp) == 0);
			CHECK(f(unfinished, &good, op, pp) == 0 && f(prims, &good, op, pp) == 0 && f(0, &good, op, pp) == 0);
			CHECK(f(scene, NULL, op, pp) == 0 && f(scene, &good, NULL, pp) == 0);
		}
		for (const RaylibAMDDistanceFieldParams& p : bad) {
			CHECK(RaylibAMD_BakeDistanceFieldDevice(scene, &p, op, pp, NULL) == 0);
			CHECK(RaylibAMD_PlanDistanceField(scene, &p, &a, &b) == 0);
		}
		for (uint32_t v : out) CHECK(v == 7u);
		for (uint32_t v : prim) CHECK(v == 7u);
		CHECK(RaylibAMD_PlanDistanceField(unfinished, &good, &a, &b) == 0 && RaylibAMD_PlanDistanceField(prims, &good, &a, &b) == 0);
		CHECK(RaylibAMD_PlanDistanceField(0, &good, &a, &b) == 0 && RaylibAMD_PlanDistanceField(scene, NULL, &a, &b) == 0);
		// the planner: the two walks' own plans
		for (const char* env : { "", "2", "4", "8" }) {
			if (*env) setenv("RAYLIB_QUERY_TREE", env, 1); else unsetenv("RAYLIB_QUERY_TREE");
			RaylibAMDQueryPlan c, r;
			CHECK(RaylibAMD_PlanDistanceField(scene, &good, &a, &b) == 1 && RaylibAMD_PlanDistanceField(scene, &good, NULL, NULL) == 1);
			CHECK(RaylibAMD_PlanNearest(scene, RAYLIB_AMD_NEAREST_CLOSEST, &c) == 1 && RaylibAMD_PlanRayQueryAll(scene, 1, 1, &r) == 1);
			CHECK(memcmp(&a, &c, sizeof(a)) == 0 && memcmp(&b, &r, sizeof(b)) == 0);
			CHECK((a.treeWidth == 2 || a.treeWidth == 4) && (b.treeWidth == 2 || b.treeWidth == 8));
		}
	}
	Raylib_DestroyScene(unfinished); Raylib_DestroyScene(scene); Raylib_DestroyScene(prims);
	RaylibAMD_DestroySceneElement(sphere); RaylibAMD_DestroyMaterial(m);
	printf("sdf_host_check: ok\n");
	return 0;
}
