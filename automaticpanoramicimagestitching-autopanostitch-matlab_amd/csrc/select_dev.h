// select_dev.h — strongest-N selection on the device, shared by fast.hip, sift.hip and surf.hip (not part of the ABI).
// The caller has one 64-bit key per candidate, whose top 4 bits are the candidate's group and whose ascending order within a group
// is descending strength, and asks for the first keep[g] candidates of every group by (key ascending, index ascending):
//   stable radix sort (rocprim) of (key, index)
//   strongest_flag_kernel   rank within the group < keep[g], written back by candidate index
//   strongest_word_kernel   one ballot = one 64-bit word of the bitmap over the candidates, whose bit order is their order
//   exclusive scan of the words' popcounts (rocprim)
// The caller's ordered compaction (select_compact_kernel; fast.hip has its own, which moves two arrays) reads (words, prefix) as
// fast_emit_kernel / surf_emit_kernel read theirs: the kept candidates keep the order they had.  No atomics; every result is the
// same from run to run.
//
// Uniform-N (DESIGN.md "Uniform-N selection") cuts per (group, cell) instead of per group.  Every candidate also has a segment id,
// segment = group * cells + cell, below 2^14; select_uniform asks for the first keep[s] candidates of every segment, where keep comes
// from water-filling the group's budget over the counts of its cells:
//   stable radix sort by (segment, key): one sort of a composite key, or a sort by key and a second one by segment
//   uniform_bounds_kernel   start[s] of every segment in the sorted sequence, by one lower-bound search each (an empty segment: c = 0)
//   uniform_quota_kernel    one workgroup per group: the water level by bisection, the remainder by a scan, keep[s]
//   uniform_flag_kernel     rank within the segment < keep[s], written back by candidate index
//   strongest_word_kernel and the scan, as above
// Integer arithmetic only, no atomics, and no read-back: the caller knows the number kept from the budgets.
#pragma once
#include <hip/hip_runtime.h>

#include "aps_internal.h"
#include "prims_dev.h"
#include "select_key.h"
#include "uniform_rule.h"

namespace aps {
namespace {

constexpr int kSelectGroups = 16;  // the key's top 4 bits

// The cut of a sorted key sequence: group g (the key's top 4 bits) starts at start[g] and keeps its first keep[g] items.
struct StrongestCut {
    unsigned int start[kSelectGroups], keep[kSelectGroups];
};

// the cut of a single group (group 0: keys below 2^60) of n candidates that keeps the first k
inline StrongestCut single_group_cut(unsigned int n, unsigned int k) {
    StrongestCut cut;
    for (int g = 0; g < kSelectGroups; ++g) {
        cut.start[g] = g ? n : 0u;
        cut.keep[g] = g ? 0u : k;
    }
    return cut;
}

// (strength_key_f32, the key of a non-negative f32 strength in group 0: select_key.h)

// position p of the sorted sequence -> flag of the item it came from
__global__ __launch_bounds__(256) void strongest_flag_kernel(const unsigned long long* __restrict__ sorted_keys,
                                                             const unsigned int* __restrict__ sorted_vals, const StrongestCut cut,
                                                             unsigned int n, uint8_t* __restrict__ flags) {
    const unsigned int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int grp = (int)(sorted_keys[p] >> 60);
    unsigned int start = 0, keep = 0;
#pragma unroll
    for (int l = 0; l < kSelectGroups; ++l)  // (constant indices: the table stays in scalar registers)
        if (grp == l) {
            start = cut.start[l];
            keep = cut.keep[l];
        }
    flags[sorted_vals[p]] = p - start < keep ? 1 : 0;
}

// one wave per word: its ballot over 64 flags (a word beyond the n flags is zero)
__global__ __launch_bounds__(256) void strongest_word_kernel(const uint8_t* __restrict__ flags, unsigned int n, unsigned int n_words,
                                                             unsigned long long* __restrict__ words) {
    const int lane = threadIdx.x & 63;
    const unsigned int q = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (q >= n_words) return;  // (uniform in the wave)
    const unsigned int i = q * 64 + lane;
    const unsigned long long mask = __ballot(i < n && flags[i] != 0);
    if (lane == 0) words[q] = mask;
}

// flags over the candidates -> the bitmap over the indices with the exclusive scan of its popcounts: words[n / 64 + 1] and prefix alike;
// prefix[n_words] is the number kept
inline void flags_to_words(const uint8_t* flags, unsigned int n, Ws<unsigned long long>& words, Ws<unsigned int>& prefix,
                           unsigned int& n_words) {
    n_words = cdiv(n, 64);
    words.alloc((size_t)n_words + 1);  // (+1: a zero word, whose prefix is the total)
    prefix.alloc((size_t)n_words + 1);
    strongest_word_kernel<<<cdiv((size_t)n_words + 1, 4), 256, 0, stream()>>>(flags, n, n_words + 1, words);
    check_launch("strongest_word_kernel");
    exclusive_scan(popcounts(words.get()), prefix.get(), 0u, (size_t)n_words + 1);
}

// The selection proper, for any 64-bit key whose top 4 bits are the group: sorts (key, index) by ascending key (stable: equal keys keep
// ascending index), flags the first cut.keep[g] items of every group, and returns the flags as a bitmap over the indices with the exclusive
// scan of its popcounts - words[n / 64 + 1] and prefix alike; prefix[n_words] is the number kept.  No atomics; the result is deterministic.
// key_bits: the keys' significant low bits (a caller whose keys all lie below 2^key_bits spares the sort the passes over the zero bits).
inline void select_by_key(const unsigned long long* keys, const unsigned int* vals, unsigned int n, const StrongestCut& cut,
                          Ws<unsigned long long>& words, Ws<unsigned int>& prefix, unsigned int& n_words, unsigned int key_bits = 64u) {
    Ws<unsigned long long> skeys(n);
    Ws<unsigned int> svals(n);
    Ws<uint8_t> flags(n);
    sort_pairs(keys, skeys.get(), vals, svals.get(), n, key_bits);
    strongest_flag_kernel<<<cdiv(n, 256), 256, 0, stream()>>>(skeys, svals, cut, n, flags);
    check_launch("strongest_flag_kernel");
    flags_to_words(flags, n, words, prefix, n_words);
}

// Ordered compaction of the flagged records (sift.hip: oriented keypoints, surf.hip: candidates): bit k of word q is record 64 q + k,
// which becomes record prefix[q] + (set bits below k), so the kept ones keep the order they had.
template <class T>
__global__ __launch_bounds__(256) void select_compact_kernel(const unsigned long long* __restrict__ words,
                                                             const unsigned int* __restrict__ prefix, unsigned int n_words,
                                                             const T* __restrict__ in, unsigned int n, T* __restrict__ out,
                                                             unsigned int kcap) {
    const unsigned int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_words) return;
    unsigned long long bits = words[q];
    unsigned int pos = prefix[q];
    while (bits) {
        const int k = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        if (pos < kcap && q * 64 + k < n) out[pos] = in[q * 64 + k];
        ++pos;
    }
}

// ---- uniform-N (DESIGN.md "Uniform-N selection") ------------------------------------------------------------------------------
// (kSegmentBits, kSegmentShift and check_uniform, the argument checks of the uniform entries: select_key.h)

// the budgets Q_g of the groups, known on the host
struct UniformBudget {
    unsigned int q[kSelectGroups];
};

// start[s], s = 0 .. n_seg: the first position of the sorted sequence whose segment is >= s (segment = sorted[p] >> shift), so that
// segment s holds positions start[s] .. start[s + 1] - 1 and an empty one comes out as c = 0.
template <class K>
__global__ __launch_bounds__(256) void uniform_bounds_kernel(const K* __restrict__ sorted, unsigned int shift, unsigned int n,
                                                             unsigned int n_seg, unsigned int* __restrict__ start) {
    const unsigned int s = blockIdx.x * 256 + threadIdx.x;
    if (s > n_seg) return;
    unsigned int lo = 0, hi = n;
    while (lo < hi) {
        const unsigned int mid = lo + (hi - lo) / 2;
        if ((unsigned int)(sorted[mid] >> shift) < s)
            lo = mid + 1;
        else
            hi = mid;
    }
    start[s] = lo;
}

// the reduction of one value per thread over a block of 16 waves, returned to every thread
template <class Op>
__device__ __forceinline__ unsigned int block_reduce_u32(unsigned int v, Op op, unsigned int* s_part) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = op(v, (unsigned int)__shfl_xor((int)v, off));
    __syncthreads();  // (the partials of the reduction before this one have been read)
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned int acc = s_part[0];
#pragma unroll
    for (int w = 1; w < kUniformMaxCells / 64; ++w) acc = op(acc, s_part[w]);
    return acc;
}

// One workgroup per group, one thread per cell: keep[s] by water-filling the group's budget over its cells' counts.
__global__ __launch_bounds__(kUniformMaxCells) void uniform_quota_kernel(const unsigned int* __restrict__ start, unsigned int cells,
                                                                         const UniformBudget B, unsigned int* __restrict__ keep) {
    __shared__ unsigned int s_part[kUniformMaxCells / 64];
    const unsigned int k = threadIdx.x, g = blockIdx.x, s = g * cells + k;
    const int lane = k & 63, wave = k >> 6;
    const unsigned int c = k < cells ? start[s + 1] - start[s] : 0u;
    unsigned int budget = 0;
#pragma unroll
    for (int l = 0; l < kSelectGroups; ++l)  // (constant indices: the table stays in scalar registers)
        if (g == (unsigned int)l) budget = B.q[l];
    const auto add = [](unsigned int a, unsigned int b) { return a + b; };
    const auto larger = [](unsigned int a, unsigned int b) { return a > b ? a : b; };
    const unsigned int total = block_reduce_u32(c, add, s_part);
    if (budget > total) budget = total;  // (Q <= sum c is the caller's; with it this changes nothing)
    const unsigned int top = block_reduce_u32(c, larger, s_part);
    const auto S = [&](unsigned int t) { return block_reduce_u32(c < t ? c : t, add, s_part); };
    const unsigned int t = waterfill_level<unsigned int>(top, budget, S);
    const unsigned int r = budget - S(t);
    // exclusive scan of (c > t) in ascending cell order: a ballot within the wave, the waves' totals before it
    const unsigned long long above = __ballot(c > t);
    __syncthreads();
    if (lane == 0) s_part[wave] = (unsigned int)__popcll(above);
    __syncthreads();
    unsigned int before = (unsigned int)__popcll(above & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += s_part[w];
    if (k < cells) keep[s] = waterfill_keep<unsigned int>(c, t, before, r);
}

// position p of the sorted sequence -> flag of the item it came from: kept iff its rank within its segment is below keep[segment]
template <class K>
__global__ __launch_bounds__(256) void uniform_flag_kernel(const K* __restrict__ sorted, unsigned int shift,
                                                           const unsigned int* __restrict__ sorted_vals,
                                                           const unsigned int* __restrict__ start, const unsigned int* __restrict__ keep,
                                                           unsigned int n, unsigned int n_seg, uint8_t* __restrict__ flags) {
    const unsigned int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const unsigned int seg = (unsigned int)(sorted[p] >> shift);
    flags[sorted_vals[p]] = seg < n_seg && p - start[seg] < keep[seg] ? 1 : 0;
}

// the segments of the positions of a sequence sorted by key: the second sort's keys
__global__ __launch_bounds__(256) void uniform_gather_kernel(const unsigned int* __restrict__ segs, const unsigned int* __restrict__ sorted_vals,
                                                             unsigned int n, unsigned int* __restrict__ out) {
    const unsigned int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) out[p] = segs[sorted_vals[p]];
}

// bounds, quota and flags of a sequence sorted by (segment, key, index); segment = sorted[p] >> shift
template <class K>
inline void uniform_flags(const K* sorted, unsigned int shift, const unsigned int* sorted_vals, unsigned int n, unsigned int n_groups,
                          unsigned int cells, const UniformBudget& B, uint8_t* flags) {
    const unsigned int n_seg = n_groups * cells;
    Ws<unsigned int> start((size_t)n_seg + 1), keep(n_seg);  // the table of at most 16384 segments
    uniform_bounds_kernel<K><<<cdiv((size_t)n_seg + 1, 256), 256, 0, stream()>>>(sorted, shift, n, n_seg, start);
    check_launch("uniform_bounds_kernel");
    uniform_quota_kernel<<<n_groups, kUniformMaxCells, 0, stream()>>>(start, cells, B, keep);
    check_launch("uniform_quota_kernel");
    uniform_flag_kernel<K><<<cdiv(n, 256), 256, 0, stream()>>>(sorted, shift, sorted_vals, start, keep, n, n_seg, flags);
    check_launch("uniform_flag_kernel");
}

// The uniform selection: of n candidates in n_groups groups of `cells` cells, keeps B.q[g] <= (candidates of g) of every group g, spread
// over its cells by water-filling, and within a cell the first by (key ascending, index ascending).  Returns (words, prefix) as
// select_by_key does.  Two forms of the input:
//   segs == nullptr  keys[i] = segment << kSegmentShift | strength key of 32 bits: one sort of 32 + 14 bits
//   segs != nullptr  keys[i] orders the candidates by strength (any of its 64 bits), segs[i] is the segment: a stable sort by key,
//                    then one by segment
inline void select_uniform(const unsigned long long* keys, const unsigned int* segs, const unsigned int* vals, unsigned int n,
                           unsigned int n_groups, unsigned int cells, const UniformBudget& B, Ws<unsigned long long>& words,
                           Ws<unsigned int>& prefix, unsigned int& n_words) {
    Ws<unsigned long long> skeys(n);
    Ws<unsigned int> svals(n);
    Ws<uint8_t> flags(n);
    if (!segs) {
        sort_pairs(keys, skeys.get(), vals, svals.get(), n, kSegmentShift + kSegmentBits);
        uniform_flags(skeys.get(), kSegmentShift, svals.get(), n, n_groups, cells, B, flags.get());
    } else {
        Ws<unsigned int> kseg(n), sseg(n), svals2(n);
        sort_pairs(keys, skeys.get(), vals, svals.get(), n, 64u);
        uniform_gather_kernel<<<cdiv(n, 256), 256, 0, stream()>>>(segs, svals, n, kseg);
        check_launch("uniform_gather_kernel");
        const unsigned int *kseg_in = kseg, *svals_in = svals;  // (read-only as the first sort's inputs are: the same kernels)
        sort_pairs(kseg_in, sseg.get(), svals_in, svals2.get(), n, kSegmentBits);
        uniform_flags(sseg.get(), 0u, svals2.get(), n, n_groups, cells, B, flags.get());
    }
    flags_to_words(flags, n, words, prefix, n_words);
}

}  // namespace
}  // namespace aps
