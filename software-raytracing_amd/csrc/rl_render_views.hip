// The views twins of k_trace, k_aov and k_resolve (RaylibAMD_RenderViews) as a translation unit of their own: the same source as rl_render.hip, which
// only declares them.  Instantiated beside the one-view kernels, the twins change how the helpers both call are inlined into those, and the one-view kernels
// must stay what they are (tools/isa_equivalence.py).  (k_trace_pool's twins live in rl_render_pool.hip's unit, which they leave unchanged.)
#define RL_TU_VIEWS 1
#include "rl_render.hip"
