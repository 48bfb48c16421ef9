// The lit-sample mask of the lazy-reflectance instance (rl_device.h DLitList), one statement for the device and the host: k_resolve_lit (rl_render_lazy.hip) sums a
// slot's batch with it, tools/lit_mask_host_check.cc sets it against the straight loop of SumSlotBatch (rl_dev_jobs.h).
//
// Why the flagged samples alone give the straight loop's bits: a pixel's sum starts at +0 and takes `a += v` per sample, in sample order.  No partial sum is -0:
// (+0) + (+-0) is +0 under round-to-nearest, x + y of a non-zero x is -0 for no y, and a sum that cancels exactly is +0.  For every other a -- NaNs included, which an
// addition has already quieted -- a + (+0) has a's bits.  So the additions of the samples whose three words are all zero bits change nothing and are left out, with
// their loads; a sample with any bit set (a -0 component too) is stored, flagged and added, in the same order as before.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RL_LM_HD __host__ __device__ inline
#else
#define RL_LM_HD inline
#endif

namespace rl {

// where sample s of a slot has its bit
RL_LM_HD size_t LitMaskWord(uint32_t s, uint32_t numSlots, uint32_t slot) { return (size_t)(s >> 5) * numSlots + slot; }
RL_LM_HD uint32_t LitMaskBit(uint32_t s) { return 1u << (s & 31u); }

// The flagged samples of one slot added to (ax, ay, az), lowest sample first.  samples: [s][numSlots] triples of float (SampleRGB).
RL_LM_HD void LitMaskSum(const uint32_t* mask, uint32_t maskWords, const float* samples, uint32_t numSlots, uint32_t slot, float& ax, float& ay, float& az)
{
	for (uint32_t w = 0; w < maskWords; ++w) {
		uint32_t m = mask[(size_t)w * numSlots + slot];
		while (m != 0u) {
			const uint32_t s = w * 32u + (uint32_t)__builtin_ctz(m);
			const float* v = samples + ((size_t)s * numSlots + slot) * 3u;
			ax += v[0]; ay += v[1]; az += v[2];
			m &= m - 1u;
		}
	}
}

} // namespace rl
