// prims_dev.h — the device primitives the detectors and the matchers share, on the calling thread's stream (not part of the ABI).
// Each states rocprim's two-call idiom (ask for the temporary bytes, take them from the workspace, run) or the read-back idiom
// (copy, synchronise) once.  rocprim instantiates its kernels on the iterator and size types it is handed - a pointer to const is
// another kernel than a pointer - so the scan and the sort take them as the caller has them.  The temporary storage goes back to the workspace when the helper returns; the workspace hands a
// thread's blocks out again in the order of that thread's one stream, so the run that reads it comes first.
#pragma once
#include <hip/hip_runtime.h>

#include "aps_internal.h"

#include <rocprim/rocprim.hpp>

namespace aps {
namespace {

// out[i] = init + in[0] + ... + in[i - 1], i < n; `in` is a pointer or an iterator (PopcOp over ballot words)
template <class InIt, class T>
inline void exclusive_scan(InIt in, T* out, T init, size_t n) {
    size_t bytes = 0;
    APS_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, init, n, rocprim::plus<T>(), stream()));
    Ws<char> tmp(bytes);
    APS_HIP(rocprim::exclusive_scan(tmp.get(), bytes, in, out, init, n, rocprim::plus<T>(), stream()));
}

// the set bits of ballot words as a scan's input (It: a pointer to 64-bit words)
template <class It>
inline auto popcounts(It words) {
    return rocprim::make_transform_iterator(words, PopcOp());
}

// stable radix sort of (key, value) by the keys' low key_bits bits: (keys, vals) -> (skeys, svals), pointers to n elements each.
// Size: the type rocprim's kernels count in; sift.hip and hamming_pairs.hip name unsigned int, which their sorts were built on.
template <class Size = size_t, class KeyIn, class KeyOut, class ValIn, class ValOut>
inline void sort_pairs(KeyIn keys, KeyOut skeys, ValIn vals, ValOut svals, unsigned int n, unsigned int key_bits) {
    size_t bytes = 0;
    APS_HIP(rocprim::radix_sort_pairs(nullptr, bytes, keys, skeys, vals, svals, (Size)n, 0u, key_bits, stream()));
    Ws<char> tmp(bytes);
    APS_HIP(rocprim::radix_sort_pairs(tmp.get(), bytes, keys, skeys, vals, svals, (Size)n, 0u, key_bits, stream()));
}

// d[0 .. k - 1] on the host: one copy, one synchronisation
template <class T>
inline void read_back(const T* d, T* h, int k) {
    APS_HIP(hipMemcpyAsync(h, d, (size_t)k * sizeof(T), hipMemcpyDeviceToHost, stream()));
    APS_HIP(hipStreamSynchronize(stream()));
}
template <class T>
inline T read_back(const T* d) {
    T v;
    read_back(d, &v, 1);
    return v;
}

// the total of an exclusive scan `pos` of `val`, n > 0 elements each: pos[n - 1] + val[n - 1], two copies under one synchronisation
template <class T>
inline T scan_total(const T* pos, const T* val, size_t n) {
    T last_pos, last_val;
    APS_HIP(hipMemcpyAsync(&last_pos, pos + n - 1, sizeof(T), hipMemcpyDeviceToHost, stream()));
    APS_HIP(hipMemcpyAsync(&last_val, val + n - 1, sizeof(T), hipMemcpyDeviceToHost, stream()));
    APS_HIP(hipStreamSynchronize(stream()));
    return last_pos + last_val;
}

}  // namespace
}  // namespace aps
