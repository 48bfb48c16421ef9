// The triangle-overlap queries of RaylibAMD_OverlapTriangles (k_overlap, rl_k_overlap.inl) as a translation unit of their own: a new walk beside the ray walks
// and the nearest-point walk, and every other unit stays the code it is (tools/isa_equivalence.py).

// ---- settings ----
// None: single float operations without FMA (the Makefile's -ffp-contract=off), as the host oracle that compiles the same statements (rl_overlap.h).

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_overlap.h"
#include "rl_contact.h"

namespace rl {

// ---- kernel bodies ----
#include "rl_k_overlap.inl"
#define RL_OVERLAP_CONTACTS_PASS   // the same text again, as k_overlap_contacts
#include "rl_k_overlap.inl"
#undef RL_OVERLAP_CONTACTS_PASS

// ---- instances ----
RL_OVERLAP_INSTANCES(RL_K_OVERLAP)
RL_OVERLAP_CONTACTS_INSTANCES(RL_K_OVERLAP_CONTACTS)

} // namespace rl
