// Stand-alone sanitizer run over the host oracles of the variance-guided filter (RaylibAMD_TemporalAccumulateMomentsHost, RaylibAMD_FilterVarianceHost; csrc/rl_oracle.cc,
// csrc/rl_temporal.h, csrc/rl_variance.h; tools/host_check.sh variance): frames from 1 x 1 to 67 x 41 in exact-size arrays, so that a read or write one element out
// of bounds is seen -- sky and surfaces, perpendicular normals, duplicate positions, short and long histories, channels that are not finite, K = 1 .. 6 (taps up
// to 64 pixels outside the frame), with and without the variance plane and the history.  With a file name: the crafted planes of the tests as
// tests/variance_cases.dump wrote them, through both oracles.  No GPU, no Python.
#include "raylib_amd.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { printf("variance_host_check: FAILED %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

struct Surface { int32_t hit; float t, p[3], n[3], paramU, paramV; int32_t material; };
static_assert(sizeof(Surface) == 44, "the G-buffer's surface record");

static int RunFile(const char* path)
{
	FILE* f = fopen(path, "rb");
	CHECK(f);
	uint32_t wh[2];
	CHECK(fread(wh, 4, 2, f) == 2);
	const uint32_t W = wh[0], H = wh[1];
	const size_t n = (size_t)W * H;
	// the accumulation's colour, hit, motion, history colour, hit, length, moments; the filter's colour, moments, length, hit, surface: floats per pixel
	const size_t words[12] = { 4, 4, 4, 4, 4, 1, 2, 4, 2, 1, 4, 11 };
	std::vector<float> a[12];
	for (int k = 0; k < 12; ++k) { a[k].resize(n * words[k]); CHECK(fread(a[k].data(), 4, a[k].size(), f) == a[k].size()); }
	fclose(f);
	const RaylibAMDTemporalParams tp = { 0.0625f, 8.0f };
	const RaylibAMDTemporalMomentsFrame hist = { a[3].data(), (const RaylibAMDHitT*)a[4].data(), a[5].data(), a[6].data() };
	std::vector<float> oc(n * 4), ol(n), om(n * 2), ov(n);
	CHECK(RaylibAMD_TemporalAccumulateMomentsHost(W, H, &tp, a[0].data(), (const RaylibAMDHitT*)a[1].data(), (const RaylibAMDMotion*)a[2].data(), &hist, oc.data(), ol.data(), om.data()) == 1);
	const RaylibAMDVarianceFilterPlanes pl = { a[7].data(), a[8].data(), a[9].data(), (const RaylibAMDHitT*)a[10].data(), a[11].data() };
	for (int K = 1; K <= 6; ++K) {
		const RaylibAMDVarianceFilterParams fp = { K, 4.0f, 0.35f, 0.1f, 2.5f };
		CHECK(RaylibAMD_FilterVarianceHost(W, H, &fp, &pl, oc.data(), ov.data()) == 1);
		for (float v : oc) CHECK(isfinite(v));
	}
	printf("variance_host_check: %u x %u crafted planes ok\n", W, H);
	return 0;
}

int main(int argc, char** argv)
{
	if (argc > 1) return RunFile(argv[1]);
	const int sizes[][2] = { { 1, 1 }, { 2, 3 }, { 7, 5 }, { 16, 16 }, { 37, 21 }, { 67, 41 } };
	uint32_t seed = 12345u;
	auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) * (1.0f / 16777216.0f); };
	for (const auto& wh : sizes) {
		const uint32_t W = (uint32_t)wh[0], H = (uint32_t)wh[1];
		const size_t n = (size_t)W * H;
		std::vector<float> colour(n * 4), moments(n * 2), length(n), histColour(n * 4), histLength(n), histMoments(n * 2);
		std::vector<RaylibAMDHitT> hit(n);
		std::vector<RaylibAMDMotion> motion(n);
		std::vector<Surface> surface(n);
		for (size_t p = 0; p < n; ++p) {
			const uint32_t x = (uint32_t)(p % W), y = (uint32_t)(p / W);
			const bool sky = (x / 3 + y / 2) % 5 == 4, wall = x >= W / 3;
			for (int c = 0; c < 4; ++c) { colour[4 * p + c] = 2.0f * rnd(); histColour[4 * p + c] = 2.0f * rnd(); }
			const float m1 = 2.0f * rnd();
			moments[2 * p] = m1; moments[2 * p + 1] = m1 * m1 + rnd() - 0.3f;
			histMoments[2 * p] = rnd(); histMoments[2 * p + 1] = rnd();
			const float lens[5] = { 0.0f, 1.0f, 2.5f, 4.0f, 8.0f };
			length[p] = lens[(int)(rnd() * 4.999f)]; histLength[p] = lens[(int)(rnd() * 4.999f)];
			hit[p] = { sky ? 0.0f : 2.0f, sky ? -1 : (int32_t)(x / 4), 0.0f, 0.0f };
			motion[p] = { (float)x + 3.0f * rnd() - 1.5f, (float)y + 3.0f * rnd() - 1.5f, sky ? 0.0f : 2.0f, sky ? 2u : 1u };
			Surface s; memset(&s, 0, sizeof(s)); s.material = -1;
			if (!sky) {
				s.hit = 1; s.t = 2.0f; s.material = 0;
				s.p[0] = wall ? 0.1f * (float)(W / 3) : 0.1f * (float)x; s.p[1] = 0.1f * (float)(y / 2); s.p[2] = wall ? 0.1f * (float)x : 0.02f * rnd();   // (y / 2: rows in pairs at one position)
				s.n[wall ? 0 : 2] = 1.0f;
			}
			surface[p] = s;
		}
		if (n > 2) { colour[0] = NAN; colour[5] = INFINITY; }
		const RaylibAMDTemporalParams tp = { 0.05f, 8.0f };
		const RaylibAMDTemporalMomentsFrame hist = { histColour.data(), hit.data(), histLength.data(), histMoments.data() };
		for (int withHistory = 0; withHistory < 2; ++withHistory) {
			std::vector<float> oc(n * 4, 7.0f), ol(n, 7.0f), om(n * 2, 7.0f), pc(n * 4), plen(n);
			CHECK(RaylibAMD_TemporalAccumulateMomentsHost(W, H, &tp, colour.data(), hit.data(), motion.data(), withHistory ? &hist : NULL, oc.data(), ol.data(), om.data()) == 1);
			const RaylibAMDTemporalFrame three = { histColour.data(), hit.data(), histLength.data() };
			CHECK(RaylibAMD_TemporalAccumulateHost(W, H, &tp, colour.data(), hit.data(), motion.data(), withHistory ? &three : NULL, pc.data(), plen.data()) == 1);
			CHECK(memcmp(pc.data(), oc.data(), n * 16) == 0 && memcmp(plen.data(), ol.data(), n * 4) == 0);   // S2
		}
		const RaylibAMDVarianceFilterPlanes pl = { colour.data(), moments.data(), length.data(), hit.data(), surface.data() };
		for (int K = 1; K <= 6; ++K) {
			const RaylibAMDVarianceFilterParams fp = { K, 4.0f, 0.35f, 0.1f, 2.5f };
			std::vector<float> oc(n * 4, 7.0f), ov(n, 7.0f), oc2(n * 4, 7.0f);
			CHECK(RaylibAMD_FilterVarianceHost(W, H, &fp, &pl, oc.data(), ov.data()) == 1);
			for (float v : oc) CHECK(isfinite(v));
			for (size_t p = 0; p < n; ++p) CHECK(hit[p].prim != -1 || ov[p] == 0.0f);
			CHECK(RaylibAMD_FilterVarianceHost(W, H, &fp, &pl, oc2.data(), NULL) == 1);
			CHECK(oc == oc2);                                                                                  // S7
		}
		std::vector<float> oc(n * 4, 7.0f);
		CHECK(RaylibAMD_FilterVarianceHost(W, H, NULL, &pl, oc.data(), NULL) == 1);                            // the defaults
		CHECK(RaylibAMD_FilterVarianceHost(W, H, NULL, &pl, colour.data(), NULL) == 0);                        // in place: refused
	}
	printf("variance_host_check: ok\n");
	return 0;
}
