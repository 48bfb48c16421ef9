// k_gather_resolve and its adaptive twin, one source for both: a translation unit includes this file with RL_GATHER_ADAPTIVE 0 for RaylibAMD_Gather's kernel
// (rl_gather.hip) or 1 for RaylibAMD_GatherAdaptive's (rl_gather_adaptive.hip); prototypes: rl_kernels.h.  Everything under RL_GATHER_ADAPTIVE is the twin's
// alone, so that each kernel is the token sequence it always was (a shared device function would add an inlining level, which reorders both kernels' code:
// tools/isa_equivalence.py).
//
// One thread per point of the launch.  A point's samples lie numPoints slots apart (the trace kernel's jobs are sample-major), so a wave's lanes read 64
// neighbouring slots per sample index -- 1 KiB back to back -- and the loop over the samples is the serial sum the contract asks for: in sample order, from +0
// (or from the sums the launch before left).  The loads do not depend on the sums; RL_GATHER_AHEAD of them are issued before the adds that use them, which is
// what a single point with many samples (one lane, nothing else to hide the latency behind) lives on.
// The sphere's value per sample and basis function is L * Y_j(Wi), the nine real SH of include/raylib_amd.h, statement 3, in its order of operations.
//
// The plain kernel carries the sums of a point range from launch to launch in `acc` (first: from +0; last: the result).
// The twin works on the point `orig` the launch's slot stands for.  The sums and the moments are the call's state, indexed by orig; they start at +0 (the host
// clears them) and are always loaded: +0 + x has the bits of the plain kernel's `first ? 0 : acc` form, which starts from +0 too (x = -0 gives +0 in both).  The
// moments come from the first plane's xyz -- the hemisphere's weighted sample, the sphere's L -- by statement A2.  decide: the launch holds the pass's last
// sample range (rl_progressive.h ProgressivePixelError: the progressive renderer's statement, not restated); a point that stops writes its result exactly as
// the plain kernel's last launch does.
#define RL_GATHER_AHEAD 8
template <int GEN>
__global__ void __launch_bounds__(RL_BLOCK)
#if RL_GATHER_ADAPTIVE
k_gather_adaptive_resolve(const float4* __restrict__ samples, uint32_t numPoints, uint32_t numSamples, const uint32_t* __restrict__ live, uint32_t pointFirst,
                          const GatherAdaptiveState st, int decide, uint32_t samplesNow, float* __restrict__ out, uint32_t* __restrict__ outSamples)
#else
k_gather_resolve(const float4* __restrict__ samples, uint32_t numPoints, uint32_t numSamples, float* __restrict__ acc, float* __restrict__ out, int first, int last,
                 uint32_t sampleCount)
#endif
{
	static_assert(GEN == RL_GEN_HEMISPHERE || GEN == RL_GEN_SPHERE, "generator");
	constexpr int NA = GEN == RL_GEN_HEMISPHERE ? 3 : 27;
	const uint32_t p = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (p >= numPoints) return;
#if RL_GATHER_ADAPTIVE
	const uint32_t orig = live ? live[pointFirst + p] : pointFirst + p;
#endif
	float a[NA];
#if RL_GATHER_ADAPTIVE
#pragma unroll
	for (int j = 0; j < NA; ++j) a[j] = st.sum[(size_t)j * st.numPoints + orig];
	float s1 = st.s1[orig], s2 = st.s2[orig];
#else
#pragma unroll
	for (int j = 0; j < NA; ++j) a[j] = first ? 0.0f : acc[(size_t)j * numPoints + p];
#endif
	const float4* lp = samples + p;                                    // L (hemisphere: the weighted sample) of sample s at lp[s * numPoints]
	const float4* wp = samples + (size_t)numPoints * numSamples + p;   // the sphere's Wi plane
	auto add = [&](const float4 l, const float4 w) __attribute__((always_inline)) {
#if RL_GATHER_ADAPTIVE
		const float lum = dot(v3(l.x, l.y, l.z), v3(0.2126f, 0.7152f, 0.0722f));   // (k_progressive_resolve's statement)
		const float yv = lum / (1.0f + lum);
		s1 += yv; s2 += yv * yv;
#endif
		if constexpr (GEN == RL_GEN_HEMISPHERE) {
			(void)w;
			a[0] = a[0] + l.x; a[1] = a[1] + l.y; a[2] = a[2] + l.z;
		} else {
			const float x = w.x, y = w.y, z = w.z;
			float Y[9];
			Y[0] = 0.282095f;
			Y[1] = 0.488603f * y;
			Y[2] = 0.488603f * z;
			Y[3] = 0.488603f * x;
			Y[4] = 1.092548f * (x * y);
			Y[5] = 1.092548f * (y * z);
			Y[6] = 0.315392f * (3.0f * (z * z) - 1.0f);
			Y[7] = 1.092548f * (x * z);
			Y[8] = 0.546274f * (x * x - y * y);
#pragma unroll
			for (int j = 0; j < 9; ++j) {
				a[3 * j + 0] = a[3 * j + 0] + l.x * Y[j];
				a[3 * j + 1] = a[3 * j + 1] + l.y * Y[j];
				a[3 * j + 2] = a[3 * j + 2] + l.z * Y[j];
			}
		}
	};
	uint32_t s = 0u;
	for (; s + RL_GATHER_AHEAD <= numSamples; s += RL_GATHER_AHEAD) {
		float4 l[RL_GATHER_AHEAD], w[RL_GATHER_AHEAD];
#pragma unroll
		for (int k = 0; k < RL_GATHER_AHEAD; ++k) {
			l[k] = lp[(size_t)(s + k) * numPoints];
			if constexpr (GEN == RL_GEN_SPHERE) w[k] = wp[(size_t)(s + k) * numPoints]; else w[k] = l[k];
		}
#pragma unroll
		for (int k = 0; k < RL_GATHER_AHEAD; ++k) add(l[k], w[k]);
	}
	for (; s < numSamples; ++s) {
		const float4 l = lp[(size_t)s * numPoints];
		add(l, GEN == RL_GEN_SPHERE ? wp[(size_t)s * numPoints] : l);
	}
#if RL_GATHER_ADAPTIVE
	const bool stops = decide && (samplesNow == st.cap || ProgressiveCellStops(ProgressivePixelError(s1, s2, samplesNow), samplesNow, st.threshold, st.minSamples));
	if (!stops) {
#pragma unroll
		for (int j = 0; j < NA; ++j) st.sum[(size_t)j * st.numPoints + orig] = a[j];
		st.s1[orig] = s1; st.s2[orig] = s2;
		return;
	}
	const uint32_t at = orig, count = samplesNow;
#else
	if (!last) {
#pragma unroll
		for (int j = 0; j < NA; ++j) acc[(size_t)j * numPoints + p] = a[j];
		return;
	}
	const uint32_t at = p, count = sampleCount;
#endif
	// the mean, then the solid angle of the directions' domain: 2 pi (bits 0x40C90FDB) or 4 pi (0x41490FDB)
	const float k = rtm::rcp1_((float)count);
	const float omega = GEN == RL_GEN_HEMISPHERE ? 6.2831855f : 12.566371f;
	if constexpr (GEN == RL_GEN_HEMISPHERE) {
		((float4*)out)[at] = make_float4(a[0] * k * omega, a[1] * k * omega, a[2] * k * omega, 1.0f);
	} else {
#pragma unroll
		for (int j = 0; j < NA; ++j) out[(size_t)at * NA + j] = a[j] * k * omega;
	}
#if RL_GATHER_ADAPTIVE
	if (outSamples) outSamples[orig] = samplesNow;
	st.stopped[orig] = 1;
#endif
}
