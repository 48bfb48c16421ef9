// Sanitizer harness only (tools/host_check.sh gather): a stand-alone program over the host side of RaylibAMD_Gather / RaylibAMD_GatherDevice -- the argument
// checks and the scan of the points' times -- and over RaylibAMD_GatherDirectionsHost, linked with tools/nodevice_stub.cc in place of the device units, so every
// accepted call with points ends at "no device" (0) after the host code under test has run.  Never part of libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "gather_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

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

	for (int kind : { RAYLIB_AMD_GATHER_IRRADIANCE, RAYLIB_AMD_GATHER_SH9 }) {
		const RaylibAMDGatherParams good = { kind, 5, 1e-4f, 2, 3, 62, 0.0f, 1.0f };
		// exactly n records, on the heap: neither the time scan nor the host hook may read or write past them
		for (int n : { 0, 1, 7, 1000 }) {
			std::vector<RaylibAMDGatherPoint> pts((size_t)n);
			std::vector<float> out((size_t)n * 27, 7.0f), dirs((size_t)n * 3, 7.0f);
			for (int i = 0; i < n; ++i) pts[(size_t)i] = RaylibAMDGatherPoint{ { 0, 0, 3 }, (float)i / (float)(n + 1), { 0, (i & 1) ? 1.0f : -1.0f, 0 }, (uint32_t)i * 2654435761u };
			RaylibAMDGatherPoint* pp = n ? pts.data() : NULL; float* op = n ? out.data() : NULL; float* dp = n ? dirs.data() : NULL;
			// accepted by the checks, then "no device" -- but no points are a success without one
			CHECK(RaylibAMD_Gather(scene, &good, pp, n, op) == (n == 0));
			CHECK(RaylibAMD_GatherDevice(scene, &good, pp, n, op, NULL) == (n == 0));
			RaylibAMDGatherParams bad[9] = { good, good, good, good, good, good, good, good, good };
			bad[0].maxPathLength = -1; bad[1].sampleCount = 0; bad[2].skipDraws = 63; bad[3].rayTMin = -1.0f; bad[4].rayTMin = NAN; bad[5].rayTMin = INFINITY;
			bad[6].maxPathLength = 32769; bad[7].kind = 2; bad[8].kind = -1;
			for (const RaylibAMDGatherParams& b : bad)
				CHECK(RaylibAMD_Gather(scene, &b, pp, n, op) == 0 && RaylibAMD_GatherDevice(scene, &b, pp, n, op, NULL) == 0);
			CHECK(RaylibAMD_Gather(scene, &good, pp, -1, op) == 0 && RaylibAMD_Gather(unfinished, &good, pp, n, op) == 0 && RaylibAMD_Gather(0, &good, pp, n, op) == 0);
			CHECK(RaylibAMD_Gather(scene, NULL, pp, n, op) == 0);
			if (n) {
				CHECK(RaylibAMD_Gather(scene, &good, NULL, n, op) == 0 && RaylibAMD_Gather(scene, &good, pp, n, NULL) == 0);
				pts[(size_t)n - 1].time = NAN;        // the last record's time is looked at
				CHECK(RaylibAMD_Gather(scene, &good, pp, n, op) == 0);
				pts[(size_t)n - 1].time = INFINITY;
				CHECK(RaylibAMD_Gather(scene, &good, pp, n, op) == 0);
				pts[(size_t)n - 1].time = 0.5f;
			}
			RaylibAMDGatherParams t = good;
			t.timeMin = 1.0f; t.timeMax = 0.0f; CHECK(RaylibAMD_GatherDevice(scene, &t, pp, n, op, NULL) == 0);
			t.timeMin = NAN; CHECK(RaylibAMD_GatherDevice(scene, &t, pp, n, op, NULL) == 0);
			t.timeMin = 0.0f; t.timeMax = INFINITY; CHECK(RaylibAMD_GatherDevice(scene, &t, pp, n, op, NULL) == 0);
			for (float v : out) CHECK(v == 7.0f);
			// the cut: every launch index below the count is answered, the count itself is refused, at the top of both ranges too
			if (n) {
				RaylibAMDGatherParams big = good; big.sampleCount = 0xffffffffu;
				for (int m : { n, 0x7fffffff }) {
					RaylibAMDGatherCut cut;
					CHECK(RaylibAMD_PlanGatherCut(&big, m, 0, &cut) == 1 && cut.launches == cut.pointRanges * cut.sampleRanges && cut.first == 1);
					const uint64_t count = cut.launches;
					CHECK(RaylibAMD_PlanGatherCut(&big, m, count - 1, &cut) == 1 && cut.last == 1 && (uint64_t)cut.sampleBase + cut.numSamples == 0xffffffffull);
					CHECK((uint64_t)cut.pointFirst + cut.numPoints == (uint64_t)m);
					CHECK(RaylibAMD_PlanGatherCut(&big, m, count, &cut) == 0 && RaylibAMD_PlanGatherCut(&bad[7], m, 0, &cut) == 0);
				}
				CHECK(RaylibAMD_PlanGatherCut(NULL, n, 0, NULL) == 0);
			}
			// the host hook: refusals write nothing, then n x 3 unit vectors
			CHECK(RaylibAMD_GatherDirectionsHost(&bad[7], pp, n, 1, 0, dp) == 0 && RaylibAMD_GatherDirectionsHost(&bad[2], pp, n, 1, 0, dp) == 0);
			CHECK(RaylibAMD_GatherDirectionsHost(NULL, pp, n, 1, 0, dp) == 0 && RaylibAMD_GatherDirectionsHost(&good, pp, -1, 1, 0, dp) == 0);
			for (float v : dirs) CHECK(v == 7.0f);
			CHECK(RaylibAMD_GatherDirectionsHost(&good, pp, n, 12345, 0xffffffffu, dp) == 1);
			for (int i = 0; i < n; ++i) {
				const float* d = &dirs[(size_t)i * 3];
				CHECK(fabs(sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]) - 1.0) < 3e-7);
				if (kind == RAYLIB_AMD_GATHER_IRRADIANCE) CHECK(d[1] * pts[(size_t)i].normal[1] >= 0.0f);
			}
		}
	}
	Raylib_DestroyScene(unfinished); Raylib_DestroyScene(scene);
	RaylibAMD_DestroySceneElement(sphere); RaylibAMD_DestroySceneElement(cube); RaylibAMD_DestroyMaterial(m);
	printf("gather_host_check: ok\n");
	return 0;
}
