// uniform_rule.h — the rule of the uniform-N selection (DESIGN.md "Uniform-N selection") as functions of the host and the device:
// the cell of a pixel and the water-filling of a budget over the cells' counts.  select_dev.h's kernels and the host-only entries
// aps_uniform_cell / aps_uniform_quota (select.hip) call the same ones.  Integer arithmetic only.
#pragma once
#include <hip/hip_runtime.h>

namespace aps {

constexpr int kUniformMaxGrid = 32;                                    // rows and columns of the grid: 1..32
constexpr int kUniformMaxCells = kUniformMaxGrid * kUniformMaxGrid;    // the cells of a group = the threads of uniform_quota_kernel

// The cell of the 0-based pixel (py, px) of a plane_h x plane_w plane in a rows x cols grid.
__host__ __device__ inline int uniform_cell(int py, int px, int plane_h, int plane_w, int rows, int cols) {
    return (int)((long long)py * rows / plane_h) * cols + (int)((long long)px * cols / plane_w);
}

// Water-filling a budget Q <= sum c over cells with counts c_k, stated once for the host (aps_uniform_quota) and the device
// (uniform_quota_kernel).  The level: the largest t in [0, hi], hi >= max c, with S(t) = sum_k min(c_k, t) <= Q.  S is the caller's sum
// (a loop on the host, a block reduction on the device, where every thread of the block walks the same bisection).
template <class T, class SumMin>
__host__ __device__ inline T waterfill_level(T hi, T budget, SumMin S) {
    T lo = 0;  // S(0) = 0 <= Q
    while (lo < hi) {
        const T mid = lo + (hi - lo + 1) / 2;
        if (S(mid) <= budget)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
// What a cell with count c keeps at level t: min(c, t), and one more for the first r cells (ascending index) with c > t;
// above_before = the number of cells with c > t before this one.
template <class T>
__host__ __device__ inline T waterfill_keep(T c, T t, T above_before, T r) {
    return c <= t ? c : t + (above_before < r ? 1 : 0);
}

}  // namespace aps
