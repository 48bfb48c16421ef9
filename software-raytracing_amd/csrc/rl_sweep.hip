// The swept-sphere queries of RaylibAMD_SweepSpheres (k_sweep, rl_k_sweep.inl) as a translation unit of their own, beside the point and the box walks: the
// pieces of rl_dev_boxwalk.h (the isect record's vertices, the grid node's decode, the packed stack value, the chunk claim, the counter fold) under a walk that
// a time bound drives.

// ---- settings ----
// None: single float operations without FMA (the Makefile's -ffp-contract=off) and the compiler's correctly rounded divisions and roots, as the host oracle
// that compiles the same statements (rl_sweep.h).

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_sweep.h"
#include "rl_dev_boxwalk.h"

namespace rl {

// ---- kernel bodies ----
#include "rl_k_sweep.inl"

// ---- instances ----
RL_SWEEP_INSTANCES(RL_K_SWEEP)

} // namespace rl
