// The triangle-overlap queries of RaylibAMD_OverlapTriangles and RaylibAMD_OverlapContacts (k_overlap, k_overlap_contacts; rl_k_overlap.inl) as a translation
// unit of their own, beside the ray walks: a walk of their own (box against box), with the shared pieces of rl_dev_boxwalk.h.

// ---- settings ----
// None: single float operations without FMA (the Makefile's -ffp-contract=off), as the host oracle that compiles the same statements (rl_overlap.h).

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_overlap.h"
#include "rl_contact.h"
#include "rl_dev_boxwalk.h"

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
