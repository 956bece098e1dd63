// select_key.h — the key layout and the argument checks of select_dev.h's selection (not part of the ABI), apart from its kernels:
// a translation unit that builds the keys of its candidates but hands the selection to another one (kaze.hip, through
// select_int4_group of surf.hip) includes this header alone, and so carries no copy of the selection's kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "aps_internal.h"
#include "uniform_rule.h"

namespace aps {
namespace {

// The key of a non-negative f32 strength in group 0: for such floats the order of the values is the order of their u32 bit
// patterns, so the complement of the bits ascends as the strength descends.  32 significant bits (select_by_key's key_bits).
__device__ __forceinline__ unsigned long long strength_key_f32(float strength) { return (unsigned long long)(~__float_as_uint(strength)); }

// ---- uniform-N (DESIGN.md "Uniform-N selection") ------------------------------------------------------------------------------
constexpr unsigned int kSegmentBits = 14;                              // segment = group * cells + cell < 16 * 1024
constexpr unsigned int kSegmentShift = 32;                             // a composite key: segment << 32 | strength_key_f32

// the argument checks of the uniform entries, before any device work
inline void check_uniform(int n_uniform, int grid_rows, int grid_cols) {
    APS_REQUIRE(n_uniform >= 1, APS_E_ARG, "n_strongest (NumUniform) must be at least 1");
    APS_REQUIRE(grid_rows >= 1 && grid_rows <= kUniformMaxGrid && grid_cols >= 1 && grid_cols <= kUniformMaxGrid, APS_E_ARG,
                "grid_rows and grid_cols (UniformGrid) must be in 1..%d", kUniformMaxGrid);
}

}  // namespace
}  // namespace aps
