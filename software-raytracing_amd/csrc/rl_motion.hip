// The motion plane of RaylibAMD_RenderMotion (k_motion, rl_k_motion.inl) as a translation unit of its own: beside k_gbuffer it would be one more caller of the
// walks that kernel inlines, and k_gbuffer must stay what it is (tools/isa_equivalence.py).
//
// No setting: the hit is the render's, as in rl_gbuffer.hip (include/raylib_amd.h statements G2 and T1).

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_motion.h"

namespace rl {

// ---- kernel bodies ----
// k_gbuffer's pixel numbering and camera ray (GBufferPixel, GBufferRay) and RL_QUERY_REFILL; k_gbuffer itself is declared extern in rl_kernels.h and gets no
// instance here
#include "rl_k_gbuffer.inl"
#include "rl_k_motion.inl"

// ---- instances ----
RL_GBUFFER_INSTANCES(RL_K_MOTION)

} // namespace rl
