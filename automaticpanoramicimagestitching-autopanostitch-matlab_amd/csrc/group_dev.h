// group_dev.h — what the group entries of surf.hip and fast.hip share (aps_surf_extract_batch, aps_fast_extract_batch and the
// single-view entries, which are groups of one; not part of the ABI).
// A group's candidate bitmap is packed [view][...], so one scan orders every keypoint as (view, canonical order) and
// prefix[v * words_per_view] is the first keypoint of view v.  The rows of the views are described by one launch whose second grid
// dimension is the view; what it knows about a view is one ViewRows record in device memory:
//   plain entries      group_rows_kernel fills kp0 and rows from the scan, on the device, so that nothing visits the host before
//                      the keypoint kernel: a view's rows are written only when every view of the group fits (capacity, max_features,
//                      outputs present) - the all-or-nothing rule of the capacity protocol
//   selection entries  the host, which has read the candidate counts back, fills them
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "aps_internal.h"
#include "integral_dev.h"
#include "prims_dev.h"

namespace aps {
namespace {

// the rows of one view: outputs, its first keypoint in the group's list and the rows to write
template <class D>
struct ViewRows {
    D* desc;
    double* loc;
    float* aux;
    unsigned int kp0, rows;
};

// what group_rows_kernel tests a view's count against (a kernel argument, by value)
struct ViewLimits {
    unsigned int cap[kGroupViews];  // rows of room; 0 for a view without outputs
    int max_features;               // > 0: no view may find more
};

// n[v] = keypoints of view v, v < nv, from the scan of the packed bitmap
__global__ void view_counts_kernel(const unsigned int* __restrict__ prefix, long long words_per_view, int nv, unsigned int* __restrict__ n) {
    const int v = threadIdx.x;
    if (v < nv) n[v] = prefix[(long long)(v + 1) * words_per_view] - prefix[(long long)v * words_per_view];
}

// One wave, lane = view: the counts as view_counts_kernel gives them, and kp0 / rows of every view's record.  rows = the count when
// every view of the group fits its limits, else 0 for all of them.
template <class D>
__global__ void group_rows_kernel(const unsigned int* __restrict__ prefix, long long words_per_view, int nv, const ViewLimits lim,
                                  ViewRows<D>* __restrict__ rows, unsigned int* __restrict__ n) {
    const int v = threadIdx.x;
    unsigned int first = 0, count = 0, cap = 0;
    if (v < nv) {
        first = prefix[(long long)v * words_per_view];
        count = prefix[(long long)(v + 1) * words_per_view] - first;
#pragma unroll
        for (int k = 0; k < kGroupViews; ++k)  // (constant indices: the table stays in scalar registers)
            if (v == k) cap = lim.cap[k];
    }
    const bool fits = count <= cap && (lim.max_features <= 0 || count <= (unsigned int)lim.max_features);
    const bool all = __ballot(!fits) == 0ull;
    if (v < nv) {
        n[v] = count;
        rows[v].kp0 = first;
        rows[v].rows = all ? count : 0u;
    }
}

// the first candidate of every view in the group's list, off[v], v <= nv (a kernel argument, by value)
struct ViewOffsets {
    unsigned int off[kGroupViews + 1];
};

// kept[v] = set bits of the selection's bitmap (select_dev.h: words, prefix) among the candidates of view v
__global__ void view_kept_kernel(const unsigned long long* __restrict__ words, const unsigned int* __restrict__ prefix, const ViewOffsets O,
                                 int nv, unsigned int* __restrict__ kept) {
    const int v = threadIdx.x;
    if (v >= nv) return;
    unsigned int lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < kGroupViews; ++k)
        if (v == k) {
            lo = O.off[k];
            hi = O.off[k + 1];
        }
    const auto below = [&](unsigned int i) { return prefix[i >> 6] + (unsigned int)__popcll(words[i >> 6] & ((1ull << (i & 63)) - 1ull)); };
    kept[v] = below(hi) - below(lo);
}

// The outputs of a group on the host side: one Out per view and array, bound to `rows[v]` rows of room (0: the view is not bound),
// the device records of the views, and the strided copy-back of the logical result.  width: elements of a descriptor row;
// wide: elements of a row-major row that are written (SURF with ldd >= 128 zeroes columns 64..127 as well).
template <class D, class View>
struct GroupOut {
    std::vector<Out<D>> desc;
    std::vector<Out<double>> loc;
    std::vector<Out<float>> aux;
    Ws<ViewRows<D>> d_rows;
    ViewRows<D> h[kGroupViews];  // (the upload's source: it lives as long as the copy may read it)
    int nv, desc_layout;
    size_t width, wide;
    int64_t ldd, ldl;

    GroupOut(View* views, int nv_, const unsigned int* room, size_t width_, size_t wide_, int desc_layout_, int64_t ldd_, int64_t ldl_,
             const unsigned int* kp0, const unsigned int* rows)
        : desc(nv_), loc(nv_), aux(nv_), d_rows(nv_), nv(nv_), desc_layout(desc_layout_), width(width_), wide(wide_), ldd(ldd_), ldl(ldl_) {
        std::memset(h, 0, sizeof h);
        for (int v = 0; v < nv; ++v) {
            if (room[v]) {
                desc[v].bind(views[v].desc, desc_layout == APS_ROWMAJOR ? (size_t)(room[v] - 1) * ldd + wide : (width - 1) * (size_t)ldd + room[v]);
                loc[v].bind(views[v].loc, (size_t)ldl + room[v]);
                aux[v].bind(views[v].aux, (size_t)room[v] * 4);
            }
            h[v].desc = desc[v];
            h[v].loc = loc[v];
            h[v].aux = aux[v].present() ? aux[v].get() : nullptr;
            h[v].kp0 = kp0 ? kp0[v] : 0u;
            h[v].rows = rows ? rows[v] : 0u;
        }
        APS_HIP(hipMemcpyAsync(d_rows, h, nv * sizeof(ViewRows<D>), hipMemcpyHostToDevice, stream()));
    }
    // n[v] rows of every bound view back to the caller's arrays; the elements between the logical rows / columns stay the caller's
    void commit(const unsigned int* n) {
        for (int v = 0; v < nv; ++v) {
            if (n[v] == 0) continue;
            if (desc_layout == APS_ROWMAJOR)
                desc[v].commit_2d(wide, n[v], (size_t)ldd);
            else
                desc[v].commit_2d(n[v], width, (size_t)ldd);
            loc[v].commit_2d(n[v], 2, (size_t)ldl);
            aux[v].commit((size_t)n[v] * 4);
        }
    }
};

// The rows of room of every view - its cap (checked to lie in 0 .. 2^31 - 1 by the entry) where it has outputs to write to, else 0 -
// and the checks of the leading dimensions of the views that write, before the first launch.
template <class View>
inline void check_views(const View* views, int nv, size_t width, int desc_layout, int64_t ldd, int64_t ldl, unsigned int* room) {
    for (int v = 0; v < nv; ++v) {
        const View& V = views[v];
        room[v] = V.cap > 0 && V.desc && V.loc ? (unsigned int)V.cap : 0u;
        if (!room[v]) continue;
        if (desc_layout == APS_ROWMAJOR)
            APS_REQUIRE(ldd >= (int64_t)width, APS_E_DIM, "ldd < %d", (int)width);
        else
            APS_REQUIRE(ldd >= V.cap, APS_E_DIM, "ldd < cap");
        APS_REQUIRE(ldl >= V.cap, APS_E_DIM, "ldl < cap");
    }
}

// What the host does with the counts of a group once they are known: every view's count is set, then the first view that breaks a
// limit fails the call - max_features (`what` names the detector), capacity, a missing output - so that on APS_E_CAP every view holds
// the rows it needs.  need[v]: the rows view v would write; found[v]: what max_features is tested against.
template <class View>
inline void settle_counts(View* views, int nv, const unsigned int* need, const unsigned int* found, int max_features, const char* what) {
    for (int v = 0; v < nv; ++v) views[v].count = max_features > 0 && found[v] > (unsigned int)max_features ? found[v] : need[v];
    for (int v = 0; v < nv; ++v)
        if (max_features > 0 && found[v] > (unsigned int)max_features)
            fail(APS_E_CAP, "%s found %u features, more than params.max_features = %d", what, found[v], max_features);
    for (int v = 0; v < nv; ++v)
        if ((int64_t)need[v] > views[v].cap) fail(APS_E_CAP, "feature capacity %lld < %u features", (long long)views[v].cap, need[v]);
    for (int v = 0; v < nv; ++v) APS_REQUIRE(need[v] == 0 || (views[v].desc && views[v].loc), APS_E_ARG, "NULL output with features present");
}

}  // namespace
}  // namespace aps
