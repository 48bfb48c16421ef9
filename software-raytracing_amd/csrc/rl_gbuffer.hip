// The primary-hit G-buffer of RaylibAMD_RenderGBuffer (k_gbuffer, rl_k_gbuffer.inl) as a translation unit of its own.  Instantiated beside the render or the
// query kernels it would change how the walks and the shading they share are inlined into those, and they must stay what they are
// (tools/isa_equivalence.py).
//
// No setting: the hit is the render's, so the candidate rule's "own box ends before tMin" stays unwidened here -- the ray queries' unit (rl_query.hip) widens
// it, this one must not (include/raylib_amd.h statement G2).

// ---- the device library ----
#include "rl_kernels.h"

namespace rl {

// ---- kernel bodies ----
#include "rl_k_gbuffer.inl"

// ---- instances ----
RL_GBUFFER_INSTANCES(RL_K_GBUFFER)

} // namespace rl
