// The nearest-point queries of RaylibAMD_NearestPoints (k_nearest, rl_k_nearest.inl) and of RaylibAMD_NearestPointsAll (k_nearest_all, rl_k_nearest_all.inl) as
// a translation unit of their own, beside the ray walks: both run the point walk of rl_dev_boxwalk.h.

// ---- settings ----
// None: single float operations without FMA (the Makefile's -ffp-contract=off) and the compiler's correctly rounded divisions, as the host oracle that
// compiles the same statements (rl_nearest.h).

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_nearest.h"
#include "rl_dev_boxwalk.h"

namespace rl {

// ---- kernel bodies ----
#include "rl_k_nearest.inl"
#include "rl_k_nearest_all.inl"

// ---- instances ----
RL_NEAREST_INSTANCES(RL_K_NEAREST)
RL_NEAREST_ALL_INSTANCES(RL_K_NEAREST_ALL)

} // namespace rl
