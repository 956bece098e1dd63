// select.hip — the host-only entries of the uniform-N selection (DESIGN.md "Uniform-N selection"): the cell of a pixel and the
// water-filling of a budget over the cells' counts, through the functions (uniform_rule.h) the device kernels of select_dev.h call.
// No device is needed.
#include <algorithm>

#include "aps_internal.h"
#include "uniform_rule.h"

using namespace aps;

extern "C" {

int aps_uniform_quota(const int64_t* counts, int n_cells, int64_t budget, int64_t* keep) {
    return guarded([&] {
        APS_REQUIRE(counts && keep, APS_E_ARG, "NULL argument");
        APS_REQUIRE(n_cells >= 1 && n_cells <= kUniformMaxCells, APS_E_ARG, "n_cells must be in 1..%d", kUniformMaxCells);
        APS_REQUIRE(budget >= 0, APS_E_ARG, "negative budget");
        int64_t total = 0, top = 0;
        for (int k = 0; k < n_cells; ++k) {
            APS_REQUIRE(counts[k] >= 0 && counts[k] < (int64_t)1 << 32, APS_E_ARG, "counts must be in 0..2^32-1");
            total += counts[k];
            top = std::max(top, counts[k]);
        }
        const int64_t Q = std::min(budget, total);
        const auto S = [&](int64_t t) {
            int64_t sum = 0;
            for (int k = 0; k < n_cells; ++k) sum += std::min(counts[k], t);
            return sum;
        };
        const int64_t t = waterfill_level<int64_t>(top, Q, S);
        const int64_t r = Q - S(t);
        int64_t above = 0;
        for (int k = 0; k < n_cells; ++k) {
            keep[k] = waterfill_keep<int64_t>(counts[k], t, above, r);
            above += counts[k] > t;
        }
    });
}

int aps_uniform_cell(int py, int px, int plane_h, int plane_w, int grid_rows, int grid_cols, int* cell) {
    return guarded([&] {
        APS_REQUIRE(cell, APS_E_ARG, "NULL argument");
        APS_REQUIRE(plane_h > 0 && plane_w > 0, APS_E_DIM, "empty plane");
        APS_REQUIRE(py >= 0 && py < plane_h && px >= 0 && px < plane_w, APS_E_ARG, "pixel outside the plane");
        APS_REQUIRE(grid_rows >= 1 && grid_rows <= kUniformMaxGrid && grid_cols >= 1 && grid_cols <= kUniformMaxGrid, APS_E_ARG,
                    "grid_rows and grid_cols (UniformGrid) must be in 1..%d", kUniformMaxGrid);
        *cell = uniform_cell(py, px, plane_h, plane_w, grid_rows, grid_cols);
    });
}

}  // extern "C"
