// Sanitizer harness only (tools/host_check.sh bvh): a stand-alone program over the BVH builder, its validators and the host walks (csrc/rl_bvh.cc) on a scene large
// enough that every threaded stage of the build engages -- the all-thread scans of the top levels and the task workers (from 2^17 primitives), the grid copy of
// the 4-wide tree (from 2^16 nodes) and the emission of the 8-wide tree (from 2^15 nodes) --, built through the ABI and linked with tools/nodevice_stub.cc in
// place of the device units.  Never part of libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "bvh_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static const int kCellsX = 1024, kCellsY = 256;   // two triangles per cell: 2^19 (the 8-wide tree of a field this regular has a node per 14 triangles)
static uint32_t Mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
// a height field over [0, 16] x [0, 4] whose vertices are lifted by up to 0.02: boxes with a volume, no two alike
static void Vertex(int i, int j, float* v) { v[0] = (float)i / 64.0f; v[1] = (float)j / 64.0f; v[2] = (float)(Mix((uint32_t)(j * (kCellsX + 1) + i)) & 1023u) / 51200.0f; }

static SceneHandle Build(OBJModelHandle model, const char* threads)
{
	setenv("RAYLIB_BUILD_THREADS", threads, 1);
	SceneHandle scene = Raylib_CreateScene();
	Raylib_AddOBJModelToScene(scene, model);
	Raylib_FinalizeScene(scene);
	unsetenv("RAYLIB_BUILD_THREADS");
	return scene;
}

int main()
{
	const char* dir = getenv("TMPDIR");
	const std::string path = std::string(dir ? dir : "/tmp") + "/bvh_host_check.obj";
	{
		FILE* f = fopen(path.c_str(), "w");
		CHECK(f);
		for (int j = 0; j <= kCellsY; ++j) for (int i = 0; i <= kCellsX; ++i) { float v[3]; Vertex(i, j, v); fprintf(f, "v %.9g %.9g %.9g\n", v[0], v[1], v[2]); }
		for (int j = 0; j < kCellsY; ++j) for (int i = 0; i < kCellsX; ++i) {
			const int a = j * (kCellsX + 1) + i + 1, b = a + 1, d = a + kCellsX + 1, c = d + 1;
			fprintf(f, "f %d %d %d\nf %d %d %d\n", a, b, c, a, c, d);
		}
		CHECK(fclose(f) == 0);
	}
	OBJModelHandle model = Raylib_LoadOBJModel(path.c_str());
	remove(path.c_str());
	CHECK(model);
	Raylib_FinalizeOBJModel(model);
	SceneHandle one_thread = Build(model, "1"), five_threads = Build(model, "5");
	CHECK(one_thread && five_threads);

	// the thresholds of the threaded stages (rl_bvh.cc kParallelRange, kThreadedQuantize, kThreadedEmit8) are all passed; the Info calls run the three validators
	uint32_t nodes = 0, depth = 0, nodes4 = 0, need4 = 0, nodes8 = 0, levels8 = 0; float sah = 0, steps4 = 0, steps8 = 0;
	CHECK(RaylibAMD_SceneNumTriangles(five_threads) >= (1 << 17));
	CHECK(RaylibAMD_SceneBVHInfo(five_threads, &nodes, &depth, &sah) == 1 && nodes > 0 && depth > 0 && depth < 64);
	CHECK(RaylibAMD_SceneBVH4Info(five_threads, &nodes4, &need4) == 1 && nodes4 >= (1u << 16) && need4 > 0);
	CHECK(RaylibAMD_SceneBVH8Info(five_threads, &nodes8, &levels8, &steps4, &steps8) == 1 && nodes8 >= (1u << 15) && levels8 > 0 && steps4 > 0 && steps8 > 0);
	CHECK(RaylibAMD_SceneBVHInfo(one_thread, NULL, NULL, NULL) == 1 && RaylibAMD_SceneBVH4Info(one_thread, NULL, NULL) == 1 && RaylibAMD_SceneBVH8Info(one_thread, NULL, NULL, NULL, NULL) == 1);
	// the same tree whatever the thread count
	CHECK(RaylibAMD_SceneBVHHash(one_thread) == RaylibAMD_SceneBVHHash(five_threads));

	// both walkers: rays from above the field, down onto it at a slant; every tree's walk at full capacity finds the same closest hit
	const int n = 400;
	std::vector<float> rays(6 * (size_t)n), tmax((size_t)n, FLT_MAX), t8((size_t)n);
	for (int r = 0; r < n; ++r) {
		const float x = (float)(Mix(2u * (uint32_t)r + 1u) & 16383u) / 1024.0f, y = (float)(Mix(2u * (uint32_t)r + 2u) & 4095u) / 1024.0f;
		float* ray = &rays[6 * (size_t)r];
		ray[0] = 8.0f; ray[1] = 2.0f; ray[2] = 3.0f;
		const float dx = x - ray[0], dy = y - ray[1], dz = -ray[2], len = sqrtf(dx * dx + dy * dy + dz * dz);
		ray[3] = dx / len; ray[4] = dy / len; ray[5] = dz / len;
	}
	std::vector<uint32_t> steps((size_t)n);
	CHECK(RaylibAMD_SceneWalk8Host(five_threads, rays.data(), n, 1e-4f, tmax.data(), t8.data(), steps.data()) == 1);
	std::vector<float> t2((size_t)n), tk((size_t)n); std::vector<uint32_t> high((size_t)n);
	CHECK(RaylibAMD_SceneWalkStackHost(five_threads, 2, rays.data(), n, 1e-4f, 64, t2.data(), high.data()) == 1);
	int hits = 0;
	for (int r = 0; r < n; ++r) if (t2[(size_t)r] < FLT_MAX) { ++hits; CHECK(t8[(size_t)r] < FLT_MAX && fabsf(t8[(size_t)r] - t2[(size_t)r]) <= 1e-4f * t2[(size_t)r] && steps[(size_t)r] > 0); }
	CHECK(hits > n / 2);
	const int trees[3] = { 3, 4, 8 };
	for (int tree : trees) {
		CHECK(RaylibAMD_SceneWalkStackHost(five_threads, tree, rays.data(), n, 1e-4f, 64, tk.data(), high.data()) == 1);
		for (int r = 0; r < n; ++r) CHECK(tk[(size_t)r] == t2[(size_t)r]);
		CHECK(RaylibAMD_SceneWalkStackHost(five_threads, tree, rays.data(), n, 1e-4f, 3, tk.data(), high.data()) == 1);   // a stack that drops pushes: no more than 3 entries, ever
		for (int r = 0; r < n; ++r) CHECK(high[(size_t)r] <= 3u);
	}
	Raylib_DestroyScene(one_thread); Raylib_DestroyScene(five_threads); Raylib_UnloadOBJModel(model);
	printf("bvh_host_check: ok (%u nodes, %u 4-wide, %u 8-wide)\n", nodes, nodes4, nodes8);
	return 0;
}
