// The distance-field bake of RaylibAMD_BakeDistanceField (k_sdf_rows, k_sdf_parity, k_sdf_dist; rl_k_sdf.inl) as a translation unit of its own: the counting ray
// walks written on the pieces the ray walks share, and the point walk of rl_dev_boxwalk.h with k_nearest's leaf test, on rays and points made from voxel indices.

// ---- settings ----
// The candidate rule's "own box ends before tMin" is widened as in the ray queries' units: a row ray's accepted set is M1's (rl_dev_walk.h OwnBoxPassBox).
// The distances are single float operations without FMA (the Makefile's -ffp-contract=off) and the exact square root of rl_glibc_math.h, as the host oracle.
#define RL_OWN_BOX_WIDEN_TMIN 1
// The cut-out test inline: out of line it is the one call of the row kernels, and its frame their only scratch (rl_dev_scene.h AlphaTestCandidateNI)
#define RL_ALPHA_TEST_ATTR __forceinline__

// ---- the device library ----
#include "rl_kernels.h"
#include "rl_nearest.h"
#include "rl_sdf.h"
#include "rl_dev_boxwalk.h"

namespace rl {

// ---- kernel bodies ----
// (k_query's helpers and schedule constants -- NextUpF, QueryTMin, RL_QUERY_REFILL -- and its template, which this unit does not instantiate)
#include "rl_k_query.inl"
#include "rl_k_sdf.inl"

// ---- instances ----
RL_SDF_ROWS_INSTANCES(RL_K_SDF_ROWS)
RL_SDF_DIST_INSTANCES(RL_K_SDF_DIST)

} // namespace rl
