// The ordered multi-hit ray queries of RaylibAMD_TraceRaysAll (k_query_all, rl_k_multihit.inl) as a translation unit of their own: two walks with a list
// behind the triangle test, written on the pieces the other walks share.  Apart so that the render, query, nearest, radiance and gather units stay the code
// they are (tools/isa_equivalence.py).

// ---- settings ----
// The candidate rule's "own box ends before tMin" is widened as in the ray queries' unit: the accepted set is CLOSEST's (rl_dev_walk.h OwnBoxPassBox)
#define RL_OWN_BOX_WIDEN_TMIN 1

// ---- the device library ----
#include "rl_kernels.h"

namespace rl {

// ---- kernel bodies ----
// (k_query's helpers and schedule constants -- NextUpF, QueryTMin, RL_QUERY_REFILL -- and its template, which this unit does not instantiate)
#include "rl_k_query.inl"
#include "rl_k_multihit.inl"

// ---- instances ----
RL_QUERY_ALL_INSTANCES(RL_K_QUERY_ALL)

} // namespace rl
