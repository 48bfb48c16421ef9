// Stand-alone sanitizer run over the host oracle of the lightmap atlas filter (rl::FilterLightmapHost, csrc/rl_lightmap_filter.hip; tools/host_check.sh lightmap_filter):
// atlases from 1 x 1 to 67 x 41 with gutters, covered borders and corners, both kinds, K = 1 .. 8 (taps up to 256 texels outside the atlas), exact-size
// arrays so that a read or write one element out of bounds is seen; in place; values that are not finite; the texel array's refusals.  No GPU, no Python.
#include "rl_host.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { printf("lightmap_filter_host_check: FAILED %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
	const int sizes[][2] = { { 1, 1 }, { 2, 3 }, { 7, 5 }, { 16, 16 }, { 67, 41 } };
	uint32_t seed = 12345u;
	auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) * (1.0f / 16777216.0f); };
	for (const auto& wh : sizes) {
		const int W = wh[0], H = wh[1];
		for (int pattern = 0; pattern < 3; ++pattern) {
			// 0: every texel; 1: charts of 5 x 5 with one-texel gutters; 2: the border ring only
			std::vector<uint32_t> texel;
			for (int y = 0; y < H; ++y)
				for (int x = 0; x < W; ++x) {
					const bool on = pattern == 0 || (pattern == 1 ? (x % 6 != 5 && y % 6 != 5) : (x == 0 || y == 0 || x == W - 1 || y == H - 1));
					if (on) texel.push_back((uint32_t)(y * W + x));
				}
			const int64_t n = (int64_t)texel.size();
			std::vector<RaylibAMDGatherPoint> pts((size_t)n);
			for (int64_t i = 0; i < n; ++i) {
				RaylibAMDGatherPoint& g = pts[(size_t)i];
				g.pos[0] = 0.1f * (float)(texel[(size_t)i] % (uint32_t)W); g.pos[1] = 0.0f; g.pos[2] = 0.1f * (float)(texel[(size_t)i] / (uint32_t)W); g.time = 0.0f;
				g.normal[0] = 0.0f; g.normal[1] = 1.0f; g.normal[2] = 0.0f; g.stream = texel[(size_t)i];
			}
			for (int kind = 0; kind < 2; ++kind) {
				const size_t C = kind ? 27 : 4;
				for (int K = 1; K <= 8; ++K) {
					const RaylibAMDLightmapFilterParams F = { K, 0.7f, 0.5f, 0.2f };
					std::vector<float> in((size_t)n * C), out((size_t)n * C, 7.0f);
					for (float& v : in) v = rnd() - (kind ? 0.3f : 0.0f);
					if (n > 2) { in[0] = NAN; in[C + 1] = INFINITY; }
					CHECK(rl::FilterLightmapHost(W, H, kind, F, pts.data(), texel.data(), n, in.data(), out.data()));
					for (float v : out) CHECK(isfinite(v));
					std::vector<float> work = in;
					CHECK(rl::FilterLightmapHost(W, H, kind, F, pts.data(), texel.data(), n, work.data(), work.data()));   // in place
					CHECK(work == out);
				}
			}
			// the texel array's refusals: nothing written
			if (n >= 2) {
				const RaylibAMDLightmapFilterParams F = { 2, 1.0f, 1.0f, 1.0f };
				std::vector<float> in((size_t)n * 4, 1.0f), out((size_t)n * 4, 7.0f);
				std::vector<uint32_t> t = texel; t[1] = t[0];
				CHECK(!rl::FilterLightmapHost(W, H, 0, F, pts.data(), t.data(), n, in.data(), out.data()));
				t = texel; t[(size_t)n - 1] = (uint32_t)(W * H);
				CHECK(!rl::FilterLightmapHost(W, H, 0, F, pts.data(), t.data(), n, in.data(), out.data()));
				for (float v : out) CHECK(v == 7.0f);
			}
		}
	}
	const RaylibAMDLightmapFilterParams F = { 3, 1.0f, 1.0f, 1.0f };
	CHECK(rl::FilterLightmapHost(8, 8, 1, F, NULL, NULL, 0, NULL, NULL));   // no point: a success that touches nothing
	printf("lightmap_filter_host_check: ok\n");
	return 0;
}
