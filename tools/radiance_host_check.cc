// Sanitizer harness only (tools/host_check.sh radiance): a stand-alone program over the host side of RaylibAMD_TraceRadiance / RaylibAMD_PlanRadiance -- the
// argument checks, the scan of the rays' times and the planner -- linked with tools/nodevice_stub.cc in place of the device units, so every accepted call ends at
// "no device" (0) after the host code under test has run.  Never part of libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "radiance_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main()
{
	const float grey[3] = { 0.5f, 0.5f, 0.5f }, zero[3] = { 0, 0, 0 }, one[3] = { 1, 1, 1 };
	MaterialHandle m = RaylibAMD_CreateMaterial(0, grey, 1.0f, 0.0f, zero, 1.5f, one, 0.0f);
	CHECK(m);
	const float lo[3] = { 1, 0, 0 }, hi[3] = { 1.5f, 0.5f, 0.5f }, vel[3] = { 0, 0.5f, 0 };
	SceneElementHandle sphere = RaylibAMD_CreateSphere(0, 0, 0, 0.5f, m), cube = RaylibAMD_CreateCube(lo, hi, 0.0f, vel, m);
	CHECK(sphere && cube);
	SceneHandle scene = Raylib_CreateScene(), unfinished = Raylib_CreateScene();
	Raylib_AddSceneElement(scene, sphere); Raylib_AddSceneElement(scene, cube);
	Raylib_FinalizeScene(scene);

	const RaylibAMDRadianceParams good = { 5, 1e-4f, 0, 1, 3, 0.0f, 1.0f };
	RaylibAMDQueryPlan plan;
	CHECK(RaylibAMD_PlanRadiance(scene, &good, &plan) == 1 && plan.tree == 1 && plan.treeWidth == 2 && plan.prims == 1 && plan.early == 0);
	RaylibAMDRadianceParams longest = good; longest.maxPathLength = 32768;
	CHECK(RaylibAMD_PlanRadiance(scene, &longest, &plan) == 1);
	CHECK(RaylibAMD_PlanRadiance(scene, NULL, &plan) == 0 && RaylibAMD_PlanRadiance(scene, &good, NULL) == 0);
	CHECK(RaylibAMD_PlanRadiance(0, &good, &plan) == 0 && RaylibAMD_PlanRadiance(unfinished, &good, &plan) == 0);

	// exactly n records, on the heap: the time scan must not read past them
	for (int n : { 0, 1, 7, 1000 }) {
		std::vector<RaylibAMDPathRay> rays((size_t)n);
		std::vector<float> out((size_t)n * 4, 7.0f);
		for (int i = 0; i < n; ++i) { rays[(size_t)i] = RaylibAMDPathRay{ { 0, 0, 3 }, (float)i / (float)(n + 1), { 0, 0, -1 }, (uint32_t)i }; }
		RaylibAMDPathRay* rp = n ? rays.data() : NULL; float* op = n ? out.data() : NULL;
		// accepted by the checks, then "no device"
		CHECK(RaylibAMD_TraceRadiance(scene, &good, rp, n, op) == 0);
		CHECK(RaylibAMD_TraceRadianceDevice(scene, &good, rp, n, op, NULL) == 0);
		RaylibAMDRadianceParams bad[7] = { good, good, good, good, good, good, good };
		bad[6].maxPathLength = 32769;         // one workgroup's path stack would not fit its budget (include/raylib_amd.h)
		bad[0].maxPathLength = -1; bad[1].sampleCount = 0; bad[2].skipDraws = 65; bad[3].rayTMin = -1.0f; bad[4].rayTMin = NAN; bad[5].rayTMin = INFINITY;
		for (const RaylibAMDRadianceParams& b : bad) {
			CHECK(RaylibAMD_PlanRadiance(scene, &b, &plan) == 0);
			CHECK(RaylibAMD_TraceRadiance(scene, &b, rp, n, op) == 0 && RaylibAMD_TraceRadianceDevice(scene, &b, rp, n, op, NULL) == 0);
		}
		CHECK(RaylibAMD_TraceRadiance(scene, &good, rp, -1, op) == 0 && RaylibAMD_TraceRadiance(unfinished, &good, rp, n, op) == 0 && RaylibAMD_TraceRadiance(0, &good, rp, n, op) == 0);
		if (n) {
			CHECK(RaylibAMD_TraceRadiance(scene, &good, NULL, n, op) == 0 && RaylibAMD_TraceRadiance(scene, &good, rp, n, NULL) == 0);
			rays[(size_t)n - 1].time = NAN;       // the last record's time is looked at
			CHECK(RaylibAMD_TraceRadiance(scene, &good, rp, n, op) == 0);
			rays[(size_t)n - 1].time = INFINITY;
			CHECK(RaylibAMD_TraceRadiance(scene, &good, rp, n, op) == 0);
		}
		RaylibAMDRadianceParams t = good;
		t.timeMin = 1.0f; t.timeMax = 0.0f; CHECK(RaylibAMD_TraceRadianceDevice(scene, &t, rp, n, op, NULL) == 0);
		t.timeMin = NAN; CHECK(RaylibAMD_TraceRadianceDevice(scene, &t, rp, n, op, NULL) == 0);
		t.timeMin = 0.0f; t.timeMax = INFINITY; CHECK(RaylibAMD_TraceRadianceDevice(scene, &t, rp, n, op, NULL) == 0);
		for (float v : out) CHECK(v == 7.0f);
	}
	Raylib_DestroyScene(unfinished); Raylib_DestroyScene(scene);
	RaylibAMD_DestroySceneElement(sphere); RaylibAMD_DestroySceneElement(cube); RaylibAMD_DestroyMaterial(m);
	printf("radiance_host_check: ok\n");
	return 0;
}
