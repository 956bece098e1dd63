// select_dev.h — strongest-N selection on the device, shared by fast.hip, sift.hip and surf.hip (not part of the ABI).
// The caller has one 64-bit key per candidate, whose top 4 bits are the candidate's group and whose ascending order within a group
// is descending strength, and asks for the first keep[g] candidates of every group by (key ascending, index ascending):
//   stable radix sort (rocprim) of (key, index)
//   strongest_flag_kernel   rank within the group < keep[g], written back by candidate index
//   strongest_word_kernel   one ballot = one 64-bit word of the bitmap over the candidates, whose bit order is their order
//   exclusive scan of the words' popcounts (rocprim)
// The caller's ordered compaction reads (words, prefix) as fast_emit_kernel / surf_emit_kernel read theirs: the kept candidates
// keep the order they had.  No atomics; every result is the same from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include "aps_internal.h"

#include <rocprim/rocprim.hpp>

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

// The key of a non-negative f32 strength in group 0: for such floats the order of the values is the order of their u32 bit
// patterns, so the complement of the bits ascends as the strength descends.  32 significant bits (select_by_key's key_bits).
__device__ __forceinline__ unsigned long long strength_key_f32(float strength) { return (unsigned long long)(~__float_as_uint(strength)); }

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

// The selection proper, for any 64-bit key whose top 4 bits are the group: sorts (key, index) by ascending key (stable: equal keys keep
// ascending index), flags the first cut.keep[g] items of every group, and returns the flags as a bitmap over the indices with the exclusive
// scan of its popcounts - words[n / 64 + 1] and prefix alike; prefix[n_words] is the number kept.  No atomics; the result is deterministic.
// key_bits: the keys' significant low bits (a caller whose keys all lie below 2^key_bits spares the sort the passes over the zero bits).
inline void select_by_key(const unsigned long long* keys, const unsigned int* vals, unsigned int n, const StrongestCut& cut,
                          Ws<unsigned long long>& words, Ws<unsigned int>& prefix, unsigned int& n_words, unsigned int key_bits = 64u) {
    Ws<unsigned long long> skeys(n);
    Ws<unsigned int> svals(n);
    Ws<uint8_t> flags(n);
    size_t sbytes = 0;
    APS_HIP(rocprim::radix_sort_pairs(nullptr, sbytes, keys, skeys.get(), vals, svals.get(), (size_t)n, 0u, key_bits, stream()));
    Ws<char> stmp(sbytes);
    APS_HIP(rocprim::radix_sort_pairs(stmp.get(), sbytes, keys, skeys.get(), vals, svals.get(), (size_t)n, 0u, key_bits, stream()));
    strongest_flag_kernel<<<cdiv(n, 256), 256, 0, stream()>>>(skeys, svals, cut, n, flags);
    check_launch("strongest_flag_kernel");
    n_words = cdiv(n, 64);
    words.alloc((size_t)n_words + 1);  // (+1: a zero word, whose prefix is the total)
    prefix.alloc((size_t)n_words + 1);
    strongest_word_kernel<<<cdiv((size_t)n_words + 1, 4), 256, 0, stream()>>>(flags, n, n_words + 1, words);
    check_launch("strongest_word_kernel");
    auto counts = rocprim::make_transform_iterator(words.get(), PopcOp());
    size_t tbytes = 0;
    APS_HIP(rocprim::exclusive_scan(nullptr, tbytes, counts, prefix.get(), 0u, (size_t)n_words + 1, rocprim::plus<unsigned int>(), stream()));
    Ws<char> tmp(tbytes);
    APS_HIP(rocprim::exclusive_scan(tmp.get(), tbytes, counts, prefix.get(), 0u, (size_t)n_words + 1, rocprim::plus<unsigned int>(), stream()));
}

}  // namespace
}  // namespace aps
