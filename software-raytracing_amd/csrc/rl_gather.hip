// Irradiance and SH probes gathered at a caller's points (RaylibAMD_Gather, include/raylib_amd.h) as a translation unit of its own: the generator instances of
// the radiance loop (k_gather: rl_k_radiance.inl's twin) and the kernel that sums their samples (k_gather_resolve, below).  Instantiated beside k_radiance
// they would be further callers of the walks and the shading it inlines, and k_radiance must stay the code it is (tools/isa_equivalence.py).

// ---- settings ----
// None, as rl_radiance.hip: a gather's sample is bit for bit RaylibAMD_TraceRadiance's along the same ray.

// ---- the device library ----
#include "rl_kernels.h"

namespace rl {

// ---- kernel bodies ----
#define RL_GATHER_TWIN 1
#include "rl_k_radiance.inl"

// k_gather_resolve: one thread per point of the launch.  A point's samples lie numPoints slots apart (the trace kernel's jobs are sample-major), so a wave's
// lanes read 64 neighbouring slots per sample index -- 1 KiB back to back -- and the loop over the samples is the serial sum the contract asks for: in sample
// order, from +0 (or from the sums the launch before left in `acc`).  The loads do not depend on the sums; RL_GATHER_AHEAD of them are issued before the adds
// that use them, which is what a single point with many samples (one lane, nothing else to hide the latency behind) lives on.
// The sphere's value per sample and basis function is L * Y_j(Wi), the nine real SH of include/raylib_amd.h, statement 3, in its order of operations.
#define RL_GATHER_AHEAD 8
template <int GEN>
__global__ void __launch_bounds__(RL_BLOCK)
k_gather_resolve(const float4* __restrict__ samples, uint32_t numPoints, uint32_t numSamples, float* __restrict__ acc, float* __restrict__ out, int first, int last,
                 uint32_t sampleCount)
{
	static_assert(GEN == RL_GEN_HEMISPHERE || GEN == RL_GEN_SPHERE, "generator");
	constexpr int NA = GEN == RL_GEN_HEMISPHERE ? 3 : 27;
	const uint32_t p = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (p >= numPoints) return;
	float a[NA];
#pragma unroll
	for (int j = 0; j < NA; ++j) a[j] = first ? 0.0f : acc[(size_t)j * numPoints + p];
	const float4* lp = samples + p;                                    // L (hemisphere: the weighted sample) of sample s at lp[s * numPoints]
	const float4* wp = samples + (size_t)numPoints * numSamples + p;   // the sphere's Wi plane
	auto add = [&](const float4 l, const float4 w) __attribute__((always_inline)) {
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
	if (!last) {
#pragma unroll
		for (int j = 0; j < NA; ++j) acc[(size_t)j * numPoints + p] = a[j];
		return;
	}
	// the mean, then the solid angle of the directions' domain: 2 pi (bits 0x40C90FDB) or 4 pi (0x41490FDB)
	const float k = rtm::rcp1_((float)sampleCount);
	const float omega = GEN == RL_GEN_HEMISPHERE ? 6.2831855f : 12.566371f;
	if constexpr (GEN == RL_GEN_HEMISPHERE) {
		((float4*)out)[p] = make_float4(a[0] * k * omega, a[1] * k * omega, a[2] * k * omega, 1.0f);
	} else {
#pragma unroll
		for (int j = 0; j < NA; ++j) out[(size_t)p * NA + j] = a[j] * k * omega;
	}
}

// ---- instances ----
RL_GATHER_INSTANCES(RL_K_GATHER)
template __global__ void k_gather_resolve<RL_GEN_HEMISPHERE>(RL_GATHER_RESOLVE_ARGS);
template __global__ void k_gather_resolve<RL_GEN_SPHERE>(RL_GATHER_RESOLVE_ARGS);

} // namespace rl
