// The ray queries of RaylibAMD_TraceRays (k_query, rl_k_query.inl) as a translation unit of their own: the same source as rl_render.hip, which then only
// declares them.  Instantiated beside the render kernels they would change how the walks they share are inlined into those, and the render kernels must
// stay what they are (tools/isa_equivalence.py).
#define RL_TU_QUERY 1
#include "rl_render.hip"
