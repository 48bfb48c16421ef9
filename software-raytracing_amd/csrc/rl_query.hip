// The ray queries of RaylibAMD_TraceRays (k_query, rl_k_query.inl) as a translation unit of their own.  Instantiated beside the render kernels they
// would change how the walks they share are inlined into those, and the render kernels must
// stay what they are (tools/isa_equivalence.py).

// ---- settings ----
// The candidate rule's "own box ends before tMin" is widened here: a query's tMin is the caller's and may be a surface's own t (rl_dev_walk.h OwnBoxPassBox)
#define RL_OWN_BOX_WIDEN_TMIN 1

// ---- the device library ----
#include "rl_kernels.h"

namespace rl {

// ---- kernel bodies ----
#include "rl_k_query.inl"

// ---- instances ----
RL_QUERY_INSTANCES(RL_K_QUERY)

} // namespace rl
