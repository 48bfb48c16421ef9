// The oriented-box range queries of RaylibAMD_OverlapBoxes (k_overlap_box; rl_k_overlap_box.inl) as a translation unit of their own, beside the triangle-overlap
// queries: k_overlap's walk written again with a box-against-triangle leaf test and a third output kind, so that rl_overlap.hip stays the code it is.

// ---- settings ----
// None: single float operations without FMA (the Makefile's -ffp-contract=off), as the host oracle that compiles the same statements (rl_box.h).

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_box.h"
#include "rl_dev_boxwalk.h"

namespace rl {

// ---- kernel bodies ----
#include "rl_k_overlap_box.inl"

// ---- instances ----
RL_OVERLAP_BOX_INSTANCES(RL_K_OVERLAP_BOX)

} // namespace rl
