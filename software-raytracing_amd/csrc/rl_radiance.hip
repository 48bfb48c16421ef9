// Path-traced radiance along a caller's rays (RaylibAMD_TraceRadiance: k_radiance, rl_k_radiance.inl) as a translation unit of its own.  Instantiated
// beside the render or query kernels it would change how the walks and the shading they share are inlined into those, and they must
// stay what they are (tools/isa_equivalence.py).

// ---- settings ----
// None: the candidate rule stays the render's (RL_OWN_BOX_WIDEN_TMIN is the queries' alone, rl_query.hip), so that a camera's rays on the camera's
// streams give the render's bits.

// ---- the device library ----
#include "rl_kernels.h"

namespace rl {

// ---- kernel bodies ----
#define RL_GATHER_TWIN 0
#include "rl_k_radiance.inl"

// ---- instances ----
RL_RADIANCE_INSTANCES(RL_K_RADIANCE)

} // namespace rl
