// The triangle-overlap queries of RaylibAMD_OverlapTriangles (k_overlap, rl_k_overlap.inl) as a translation unit of their own: a new walk beside the ray walks
// and the nearest-point walk, and every other unit stays the code it is (tools/isa_equivalence.py).

// ---- settings ----
// None: single float operations without FMA (the Makefile's -ffp-contract=off), as the host oracle that compiles the same statements (rl_overlap.h).

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_overlap.h"

namespace rl {

// ---- kernel bodies ----
#include "rl_k_overlap.inl"

// ---- instances ----
RL_OVERLAP_INSTANCES(RL_K_OVERLAP)

} // namespace rl
