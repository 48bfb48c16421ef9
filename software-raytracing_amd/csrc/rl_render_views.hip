// The views twins of k_trace, k_aov and k_resolve (RaylibAMD_RenderViews) as a translation unit of their own.  Instantiated beside the one-view
// kernels, the twins change how the helpers both call are inlined into those, and the one-view kernels
// must stay what they are (tools/isa_equivalence.py).  (k_trace_pool's twins live in rl_render_pool.hip's unit, which they leave unchanged.)

// ---- settings: this unit takes every default ----

// ---- the device library ----
#include "rl_kernels.h"

namespace rl {

// ---- kernel bodies ----
#define RL_VIEWS_TWIN 1
#include "rl_k_trace.inl"
#include "rl_k_resolve.inl"
#include "rl_k_aov.inl"
#undef RL_VIEWS_TWIN

// ---- instances ----
RL_TRACE_INSTANCES(RL_K_TRACE_VIEWS)
RL_AOV_INSTANCES(RL_K_AOV_VIEWS)

} // namespace rl
