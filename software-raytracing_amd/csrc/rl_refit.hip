// The kernels behind RaylibAMD_SceneMoveTriangles (include/raylib_amd.h; launched by rl_rt_move.hip): the moved triangles' records and the refit of every tree
// the device holds.  Nothing here walks a tree or shades; the unit shares the records' arithmetic (rl_dev_core.h V3, rl_math.h) and the grid rule (rl_grid.h).

// ---- settings ----
// None: single float operations without FMA (the Makefile's -ffp-contract=off), rtm::rcp1_ and rtm::sqrt_ (rl_math.h) for 1 / x and sqrt, IEEE double
// arithmetic in the grid rule.

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_grid.h"

namespace rl {

#include "rl_k_refit.inl"

} // namespace rl
