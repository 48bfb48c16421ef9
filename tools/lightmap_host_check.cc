// Sanitizer harness only (tools/host_check.sh lightmap): a stand-alone program over the host side of the lightmap calls -- the argument checks of all four and
// the oracle RaylibAMD_LightmapPointsHost --, linked with tools/nodevice_stub.cc in place of the device units, so every accepted device call ends at "no
// device".  The outputs are heap arrays of exactly the size the contract names: the oracle may not write past min(count, capacity) records, and it must keep
// inside its owner map for charts that lie on, across and far outside the atlas' edges.  Never part of libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "lightmap_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main()
{
	const float grey[3] = { 0.5f, 0.5f, 0.5f }, zero[3] = { 0, 0, 0 }, one[3] = { 1, 1, 1 }, up[3] = { 0, 1, 0 };
	MaterialHandle m = RaylibAMD_CreateMaterial(0, grey, 1.0f, 0.0f, zero, 1.5f, one, 0.0f);
	CHECK(m);
	SceneHandle scene = Raylib_CreateScene(), unfinished = Raylib_CreateScene();
	const int kTris = 40;
	for (int i = 0; i < kTris; ++i) {
		const float x = (float)(i % 8), z = (float)(i / 8);
		const float v0[3] = { x, 0, z }, v1[3] = { x + 1, 0, z }, v2[3] = { x, 0, z + 1 };
		const float uv[6] = { x / 8, z / 5, (x + 1) / 8, z / 5, x / 8, (z + 1) / 5 };
		SceneElementHandle e = RaylibAMD_CreateTriangle(v0, v1, v2, i & 1 ? zero : up, i & 1 ? zero : up, i & 1 ? zero : up, uv, m);
		CHECK(e);
		Raylib_AddSceneElement(scene, e);
	}
	Raylib_FinalizeScene(scene);
	CHECK(RaylibAMD_SceneNumTriangles(scene) == kTris);

	const RaylibAMDGatherParams g = { RAYLIB_AMD_GATHER_IRRADIANCE, 3, 1e-4f, 0, 2, 0, 0.0f, 0.0f };
	const int sizes[][2] = { { 1, 1 }, { 7, 5 }, { 61, 47 }, { 128, 128 }, { 1, 300 }, { 300, 1 } };
	for (const auto& wh : sizes) {
		for (int variant = 0; variant < 6; ++variant) {
			RaylibAMDLightmapParams P = { wh[0], wh[1], 0, -1, 2, 0.5f, g };
			std::vector<float> uv((size_t)kTris * 6);
			const float* uvp = uv.data();
			for (int k = 0; k < kTris; ++k) for (int j = 0; j < 6; ++j) {
				const float base = (float)((k * 7 + j * 3) % 11) / 10.0f;
				float v = base;
				if (variant == 1) v = base * 4.0f - 1.5f;                      // across the edges
				if (variant == 2) v = (k & 1) ? 1e6f * base : -30.0f + 70.0f * base;   // far outside: skipped and clipped
				if (variant == 3) v = (j == k % 6) ? NAN : base;
				if (variant == 4) v = (float)((k + j) % 3) * 0.5f;             // corners on texel corners and edges, degenerate charts
				uv[(size_t)k * 6 + j] = v;
			}
			if (variant == 5) { uvp = NULL; P.triFirst = 3; P.triCount = 30; }
			const int64_t count = RaylibAMD_LightmapPointsHost(scene, &P, uvp, NULL, NULL, 0);
			CHECK(count >= 0 && count <= (int64_t)wh[0] * wh[1]);
			for (int64_t cap : { count, count / 2, count + 3 }) {
				std::vector<RaylibAMDGatherPoint> pts((size_t)cap);
				std::vector<uint32_t> tex((size_t)cap);
				CHECK(RaylibAMD_LightmapPointsHost(scene, &P, uvp, cap ? pts.data() : NULL, cap ? tex.data() : NULL, cap) == count);
				for (int64_t i = 0; i < (cap < count ? cap : count); ++i) {
					CHECK(tex[(size_t)i] < (uint32_t)(wh[0] * wh[1]) && pts[(size_t)i].stream == tex[(size_t)i] && pts[(size_t)i].time == 0.5f);
					CHECK(i == 0 || tex[(size_t)i] > tex[(size_t)i - 1]);
					CHECK(isfinite(pts[(size_t)i].pos[0]) && isfinite(pts[(size_t)i].normal[1]));
				}
			}
			// accepted by the checks, then "no device"
			std::vector<float> out((size_t)wh[0] * wh[1] * 4, 7.0f);
			std::vector<uint8_t> cov((size_t)wh[0] * wh[1], 7);
			CHECK(RaylibAMD_LightmapPoints(scene, &P, uvp, NULL, NULL, 0) == -1);
			CHECK(RaylibAMD_BakeLightmap(scene, &P, uvp, out.data(), cov.data()) == 0 && RaylibAMD_BakeLightmapDevice(scene, &P, uvp, out.data(), NULL, NULL) == 0);
			CHECK(out[0] == 7.0f && cov[0] == 7);
		}
	}
	// the refusals
	RaylibAMDLightmapParams good = { 8, 8, 0, -1, 1, 0.0f, g };
	RaylibAMDLightmapParams bad[12] = { good, good, good, good, good, good, good, good, good, good, good, good };
	bad[0].width = 0; bad[1].height = 16385; bad[2].dilate = 65; bad[3].dilate = -1; bad[4].triFirst = kTris; bad[5].triCount = kTris + 1; bad[6].triCount = 0;
	bad[7].time = NAN; bad[8].gather.kind = 2; bad[9].gather.sampleCount = 0; bad[10].gather.skipDraws = 63; bad[11].triFirst = -1;
	RaylibAMDGatherPoint pts[64]; uint32_t tex[64]; float out[64 * 4]; uint8_t cov[64];
	for (const RaylibAMDLightmapParams& b : bad) {
		CHECK(RaylibAMD_LightmapPointsHost(scene, &b, NULL, pts, tex, 64) == -1 && RaylibAMD_LightmapPoints(scene, &b, NULL, pts, tex, 64) == -1);
		CHECK(RaylibAMD_BakeLightmap(scene, &b, NULL, out, cov) == 0 && RaylibAMD_BakeLightmapDevice(scene, &b, NULL, out, cov, NULL) == 0);
	}
	CHECK(RaylibAMD_LightmapPointsHost(unfinished, &good, NULL, pts, tex, 64) == -1 && RaylibAMD_LightmapPointsHost(0, &good, NULL, pts, tex, 64) == -1);
	CHECK(RaylibAMD_LightmapPointsHost(scene, NULL, NULL, pts, tex, 64) == -1 && RaylibAMD_LightmapPointsHost(scene, &good, NULL, NULL, tex, 64) == -1);
	CHECK(RaylibAMD_LightmapPointsHost(scene, &good, NULL, pts, tex, -1) == -1 && RaylibAMD_BakeLightmap(scene, &good, NULL, NULL, cov) == 0);
	Raylib_DestroyScene(scene); Raylib_DestroyScene(unfinished);
	printf("lightmap_host_check: ok\n");
	return 0;
}
