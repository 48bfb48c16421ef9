// The pool schedule of the megakernel (k_trace_pool) and its views twin as a translation unit of their own, compiled with LLVM's "iterative-ilp"
// scheduler strategy (Makefile POOLFLAGS).  Measured on MI355X, same bits: 298 k-triangle scene 48.9 -> 44.8 ms,
// colonnade 439 -> 413 ms, 2.36 M triangles at 4K 149.7 -> 130.6 ms; k_trace (Cornell) prefers the default strategy by 0.4 %, hence two units.

// ---- settings ----
// This unit keeps the compiler's IEEE divisions (RL_EXACT_DIV, rl_glibc_math.h; used in rl_dev_shade.h): the short forms were measured on k_trace only, and the pool
// kernel's register allocation has answered arithmetic savings with losses before (Makefile, POOLFLAGS).
#undef RL_EXACT_DIV
#define RL_EXACT_DIV 0
// ... and reads the texture descriptors of a scene with few textures from an LDS copy (rl_dev_scene.h TexTable)
#define RL_LDS_TEXTURE_TABLE 1

// ---- the device library ----
#include "rl_kernels.h"

namespace rl {

// ---- kernel bodies ----
#define RL_VIEWS_TWIN 0
#include "rl_k_trace_pool.inl"
#undef RL_VIEWS_TWIN
#define RL_VIEWS_TWIN 1
#include "rl_k_trace_pool.inl"
#undef RL_VIEWS_TWIN

// ---- instances (the twins first: the one-view instances keep their places at the end of the unit's code) ----
RL_POOL_INSTANCES(RL_K_TRACE_POOL_VIEWS)
RL_POOL_INSTANCES(RL_K_TRACE_POOL)

} // namespace rl
