// Irradiance and SH probes gathered at a caller's points (RaylibAMD_Gather, include/raylib_amd.h) as a translation unit of its own: the generator instances of
// the radiance loop (k_gather: rl_k_radiance.inl's twin) and the kernel that sums their samples (k_gather_resolve: rl_k_gather_resolve.inl).  Instantiated beside k_radiance
// they would be further callers of the walks and the shading it inlines, and k_radiance must stay the code it is (tools/isa_equivalence.py).

// ---- settings ----
// None, as rl_radiance.hip: a gather's sample is bit for bit RaylibAMD_TraceRadiance's along the same ray.

// ---- the device library ----
#include "rl_kernels.h"

namespace rl {

// ---- kernel bodies ----
#define RL_GATHER_TWIN 1
#include "rl_k_radiance.inl"

// k_gather_resolve, the kernel that sums a launch's samples per point: one source with the adaptive gather's resolve (rl_gather_adaptive.hip)
#define RL_GATHER_ADAPTIVE 0
#include "rl_k_gather_resolve.inl"

// ---- instances ----
RL_GATHER_INSTANCES(RL_K_GATHER)
template __global__ void k_gather_resolve<RL_GEN_HEMISPHERE>(RL_GATHER_RESOLVE_ARGS);
template __global__ void k_gather_resolve<RL_GEN_SPHERE>(RL_GATHER_RESOLVE_ARGS);

} // namespace rl
