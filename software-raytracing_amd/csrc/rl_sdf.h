// The distance-field bake's grid arithmetic (include/raylib_amd.h statement V1), one statement for the host and the device: the kernels of rl_k_sdf.inl and the
// host oracle RaylibAMD_BakeDistanceFieldHost (rl_oracle.cc) compile this file.  Single float operations without FMA (the Makefile's -ffp-contract=off on either
// side); (float)i rounds to nearest.  Every operation rounds monotonically, so neither value decreases in i.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RL_SDF_HD __host__ __device__ inline
#else
#define RL_SDF_HD inline
#endif

namespace rl {

// the offset of index i's centre from the grid's origin on an axis of voxel size `spacing` -- the row ray's parameter there (V4) -- and the centre
RL_SDF_HD float SdfT(float spacing, uint32_t i) { return ((float)i + 0.5f) * spacing; }
RL_SDF_HD float SdfCentre(float origin, float spacing, uint32_t i) { return origin + SdfT(spacing, i); }

} // namespace rl
