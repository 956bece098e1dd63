// hamming_pairs.hip — matchFeaturesScratch's binary branch (PP/featureMatching/matchFeaturesScratch.m:81-135,170-211) for a whole
// list of image pairs in one launch chain: the batched twin of aps_hamming_2nn + filter_matches(binary).  Integer arithmetic up
// to the two percent values of the keep rule.
//
//   hamming_pairs_pack_kernel    every set's bytes as rows of 8 or 16 dwords (row- or column-major input, any leading dimension)
//   hamming_pairs_search_kernel  one job = (pair, block of 256 A rows): lane = query row in registers, B through LDS in tiles of
//                                128 rows, popcount on dwords, running best / second as integers
//                                (nearest2HammingExhaustiveMEX.cpp:52-74); then the row's keep rule (:118-121,170-178,318) and,
//                                for 'Unique', the row's bid (distance << 32 | row) for its column by a 64-bit atomic minimum
//   hamming_pairs_select_kernel  a kept row is emitted iff it holds its column (:186-207: every row proposes exactly one column,
//                                so the greedy pass in ascending (distance, row) order gives a column to its smallest bid);
//                                one ballot per wave = one word of the bitmap
//   exclusive scan of the words' popcounts (rocprim): positions, the CSR offsets (hamming_pairs_ptr_kernel) and the total
//   hamming_pairs_emit_kernel    ordered compaction into (pair << 42 | distance << 32 | row, column) - by row within a pair
//   one radix sort of those keys over all pairs (rocprim; 'Unique' only): ascending (distance, row) within a pair, the order
//                                of the stable sort at :186
//   hamming_pairs_unpack_kernel  1-based indices and the metric (d / nBits) * 100 in single (:120)
//
// The distance in the key is the bit count: (d / nBits) * 100 is strictly increasing in d (neighbouring counts differ by
// 1 / nBits >= 2^-9 relative, far above single's spacing), so the order by count is the order by metric.
// The only device-to-host read the chain needs is the total (with the CSR offsets when pair_ptr is host memory).
#include <algorithm>
#include <vector>

#include "aps_internal.h"
#include "prims_dev.h"

namespace aps {
namespace {

constexpr int kRowBlock = 256;  // A rows per job = lanes per workgroup
constexpr int kTileB = 128;     // B rows per LDS tile
constexpr int kPairShift = 42, kDistShift = 32;  // sort key: pair | distance (10 bits: 0 .. 512) | 1-based row (32 bits)
constexpr int64_t kMaxPairs = (int64_t)1 << (64 - kPairShift);
constexpr int64_t kDefaultMaxColumns = (int64_t)1 << 25;  // per-column workspace of one chunk: 8 bytes each, 256 MiB

struct HpSet {  // one descriptor set for the pack kernel
    const uint8_t* src;
    long long n, ld, row0;  // rows, leading dimension, first row in the packed pool
};
struct HpPair {
    uint32_t a_row0, n_a, b_row0, n_b;  // rows of the packed pool; n_a = 0 for a pair with an empty side
    unsigned long long col0;            // the pair's first column in its chunk's per-column workspace
};
struct HpJob {
    uint32_t pair, row0;  // rows row0 .. row0 + 255 of the pair's A set
};
struct HpRule {
    float ratio, threshold, nbits;  // f32(MaxRatio), f32(MatchThreshold), f32(nBits)
    uint32_t nbits_u, full_bits;    // nBits; 8 * nbytes (the second distance of a single candidate, mex :71-74)
    int unique;
};

__global__ __launch_bounds__(256) void hamming_pairs_pack_kernel(const HpSet* __restrict__ sets, int nbytes, int layout, int nw,
                                                                 uint32_t* __restrict__ packed) {
    const HpSet s = sets[blockIdx.x];
    for (long long e = (long long)blockIdx.y * 256 + threadIdx.x; e < s.n * nw; e += (long long)gridDim.y * 256) {
        const long long i = e / nw;
        const int wv = (int)(e % nw);
        uint32_t v = 0;
        for (int b = 0; b < 4; ++b) {
            const int k = 4 * wv + b;
            if (k < nbytes) v |= (uint32_t)(layout == APS_ROWMAJOR ? s.src[i * s.ld + k] : s.src[i + (long long)k * s.ld]) << (8 * b);
        }
        packed[(s.row0 + i) * nw + wv] = v;
    }
}

template <int NW>  // dwords per packed row
__global__ __launch_bounds__(256) void hamming_pairs_search_kernel(const uint32_t* __restrict__ packed, const HpPair* __restrict__ pairs,
                                                                   const HpJob* __restrict__ jobs, long long job0, HpRule rule,
                                                                   unsigned long long* __restrict__ cand,
                                                                   unsigned long long* __restrict__ col_bid) {
    __shared__ uint4 s_b[kTileB * NW / 4];
    const long long job = job0 + blockIdx.x;
    const HpJob jb = jobs[job];
    const HpPair pr = pairs[jb.pair];
    const uint32_t row = jb.row0 + threadIdx.x;
    const bool live = row < pr.n_a;
    uint32_t a[NW];
    {
        const uint4* src = reinterpret_cast<const uint4*>(packed) + (size_t)(pr.a_row0 + (live ? row : jb.row0)) * (NW / 4);
#pragma unroll
        for (int q = 0; q < NW / 4; ++q) {
            const uint4 v = src[q];
            a[4 * q] = v.x, a[4 * q + 1] = v.y, a[4 * q + 2] = v.z, a[4 * q + 3] = v.w;
        }
    }
    uint32_t best = 0xFFFFu, second = 0xFFFFu, ibest = 0;
    const uint4* bsrc = reinterpret_cast<const uint4*>(packed) + (size_t)pr.b_row0 * (NW / 4);
    for (uint32_t j0 = 0; j0 < pr.n_b; j0 += kTileB) {
        const int cnt = (int)min(pr.n_b - j0, (uint32_t)kTileB);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * (NW / 4); e += kRowBlock) s_b[e] = bsrc[(size_t)j0 * (NW / 4) + e];
        __syncthreads();
#pragma unroll 4
        for (int jj = 0; jj < cnt; ++jj) {  // every lane reads the same LDS words: a broadcast
            uint32_t h = 0;
#pragma unroll
            for (int q = 0; q < NW / 4; ++q) {
                const uint4 b = s_b[jj * (NW / 4) + q];
                h += __popc(a[4 * q] ^ b.x) + __popc(a[4 * q + 1] ^ b.y) + __popc(a[4 * q + 2] ^ b.z) + __popc(a[4 * q + 3] ^ b.w);
            }
            // mex :63-68: strict < moves the best (ties stay with the lower index); the second is the smaller of the rest
            if (h < best) {
                second = best;
                best = h;
                ibest = j0 + jj;
            } else {
                second = min(second, h);
            }
        }
    }
    unsigned long long c = 0;
    if (live) {
        if (pr.n_b == 1) second = rule.full_bits;   // mex :71-74
        if (second == 0) second = rule.nbits_u;     // matchFeaturesScratch.m:318
        const float pb = __fmul_rn(__fdiv_rn((float)best, rule.nbits), 100.0f);    // :120
        const float ps = __fmul_rn(__fdiv_rn((float)second, rule.nbits), 100.0f);  // :121
        if (pb <= __fmul_rn(rule.ratio, ps) && pb <= rule.threshold) {             // :171-177 (linear ratio, single)
            c = ((unsigned long long)best << 32) | (ibest + 1);
            if (rule.unique) atomicMin(&col_bid[pr.col0 + ibest], ((unsigned long long)best << 32) | row);
        }
    }
    cand[job * kRowBlock + threadIdx.x] = c;  // distance << 32 | 1-based column; 0 = the row is dropped
}

__global__ __launch_bounds__(256) void hamming_pairs_select_kernel(const HpPair* __restrict__ pairs, const HpJob* __restrict__ jobs,
                                                                   long long job0, int unique,
                                                                   const unsigned long long* __restrict__ cand,
                                                                   const unsigned long long* __restrict__ col_bid,
                                                                   unsigned long long* __restrict__ bitmap) {
    const long long job = job0 + blockIdx.x;
    const unsigned long long c = cand[job * kRowBlock + threadIdx.x];
    bool sel = c != 0;
    if (sel && unique) {
        const HpJob jb = jobs[job];
        const unsigned long long bid = (c & ~0xFFFFFFFFull) | (jb.row0 + threadIdx.x);
        sel = col_bid[pairs[jb.pair].col0 + (uint32_t)c - 1] == bid;
    }
    const unsigned long long mask = __ballot(sel);
    if ((threadIdx.x & 63) == 0) bitmap[job * (kRowBlock / 64) + (threadIdx.x >> 6)] = mask;
}

// pair_ptr[p] = matches in front of pair p's first word; word_start[n_pairs] = the number of words (prefix there = the total)
__global__ __launch_bounds__(256) void hamming_pairs_ptr_kernel(const unsigned int* __restrict__ prefix, const unsigned int* __restrict__ word_start,
                                                                long long n, int64_t* __restrict__ pair_ptr) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < n) pair_ptr[p] = prefix[word_start[p]];
}

__global__ __launch_bounds__(256) void hamming_pairs_emit_kernel(const HpJob* __restrict__ jobs, const unsigned long long* __restrict__ cand,
                                                                 const unsigned long long* __restrict__ bitmap,
                                                                 const unsigned int* __restrict__ prefix,
                                                                 unsigned long long* __restrict__ keys, uint32_t* __restrict__ cols) {
    const long long job = blockIdx.x, word = job * (kRowBlock / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const unsigned long long mask = bitmap[word];
    if (!((mask >> lane) & 1)) return;
    const unsigned int pos = prefix[word] + (unsigned int)__popcll(mask & ((1ull << lane) - 1));
    const HpJob jb = jobs[job];
    const unsigned long long c = cand[job * kRowBlock + threadIdx.x];
    keys[pos] = ((unsigned long long)jb.pair << kPairShift) | ((c >> 32) << kDistShift) | (jb.row0 + threadIdx.x + 1);
    cols[pos] = (uint32_t)c;
}

__global__ __launch_bounds__(256) void hamming_pairs_unpack_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ cols,
                                                                   long long total, float nbits, uint32_t* __restrict__ idx_a,
                                                                   uint32_t* __restrict__ idx_b, float* __restrict__ metric) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const unsigned long long k = keys[e];
    idx_a[e] = (uint32_t)k;
    idx_b[e] = cols[e];
    metric[e] = __fmul_rn(__fdiv_rn((float)((k >> kDistShift) & 0x3FFu), nbits), 100.0f);
}

// A small table that may live on either side, on the host.
template <class T>
std::vector<T> host_table(const T* p, int64_t n) {
    std::vector<T> v((size_t)std::max<int64_t>(n, 0));
    if (n <= 0) return v;
    if (is_device_ptr(p))
        APS_HIP(hipMemcpy(v.data(), p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
    else
        std::copy(p, p + n, v.begin());
    return v;
}

void put_pair_ptr(int64_t* pair_ptr, const std::vector<int64_t>& hp) {
    if (is_device_ptr(pair_ptr))
        APS_HIP(hipMemcpy(pair_ptr, hp.data(), hp.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    else
        std::copy(hp.begin(), hp.end(), pair_ptr);
}

// pa / pb: NULL = every upper-triangular pair in featureMatchingPairwise.m:48's order; max_columns: the per-column slots of one chunk
void hamming_pairs_impl(const uint8_t* const* desc, const int64_t* counts, const int64_t* ld, int n_img, int nbytes, int layout,
                        const int32_t* pair_a, const int32_t* pair_b, int64_t n_pairs, const aps_hamming_match_opts* opts,
                        int64_t* pair_ptr, uint32_t* idx_a, uint32_t* idx_b, float* metric, int64_t cap, int64_t* count,
                        int64_t max_columns = kDefaultMaxColumns) {
    // ---- argument checks: nothing below this block runs on a bad call (the block itself reads tables that live on the device) ----
    APS_REQUIRE(count != nullptr && pair_ptr != nullptr, APS_E_ARG, "count/pair_ptr is NULL");
    APS_REQUIRE(n_img >= 0 && n_pairs >= 0, APS_E_ARG, "negative image or pair count");
    APS_REQUIRE(n_pairs < kMaxPairs, APS_E_DIM, "too many pairs for one call (%lld)", (long long)n_pairs);
    APS_REQUIRE(n_img == 0 || (desc && counts && ld), APS_E_ARG, "NULL descriptor table");
    APS_REQUIRE(layout == APS_ROWMAJOR || layout == APS_COLMAJOR, APS_E_TYPE, "unknown layout");
    APS_REQUIRE(nbytes > 0 && nbytes <= 64, APS_E_DIM, "byte width must be in 1..64 (ORB 32, BRISK / FREAK 64)");
    APS_REQUIRE(cap >= 0, APS_E_ARG, "negative capacity");
    APS_REQUIRE(max_columns > 0, APS_E_ARG, "the column bound must be positive");
    aps_hamming_match_opts o;
    if (opts) {
        o = *opts;
    } else {  // matchFeaturesScratch.m:59-78 defaults, MatchThreshold the binary one (:32)
        o.max_ratio = 0.6, o.match_threshold = 10.0, o.unique = 1, o.nbits = 0;
    }
    APS_REQUIRE(o.max_ratio > 0.0 && o.max_ratio <= 1.0, APS_E_ARG, "MaxRatio must be in (0,1]");
    APS_REQUIRE(o.match_threshold >= 0.0, APS_E_ARG, "MatchThreshold must be >= 0");
    APS_REQUIRE(o.nbits >= 0 && o.nbits <= 8 * nbytes, APS_E_ARG, "nbits must be 0 (= 8 * nbytes) or in 1..%d", 8 * nbytes);
    APS_REQUIRE((pair_a == nullptr) == (pair_b == nullptr), APS_E_ARG, "NULL pair list");
    const std::vector<const uint8_t*> h_desc = host_table(desc, n_img);
    const std::vector<int64_t> h_cnt = host_table(counts, n_img), h_ld = host_table(ld, n_img);
    std::vector<int32_t> pa, pb;
    if (pair_a) {
        pa = host_table(pair_a, n_pairs);
        pb = host_table(pair_b, n_pairs);
    } else {
        for (int j = 1; j < n_img; ++j)
            for (int i = 0; i < j; ++i) pa.push_back(i), pb.push_back(j);
    }
    int64_t pool_rows = 0;
    for (int i = 0; i < n_img; ++i) {
        APS_REQUIRE(h_cnt[i] >= 0, APS_E_ARG, "negative size");
        APS_REQUIRE(h_cnt[i] == 0 || h_desc[i], APS_E_ARG, "NULL descriptor set %d", i);
        APS_REQUIRE(h_cnt[i] == 0 || h_ld[i] >= (layout == APS_ROWMAJOR ? nbytes : h_cnt[i]), APS_E_DIM,
                    "leading dimension of set %d too small (Byte width mismatch.)", i);  // hamm2nn:cols
        pool_rows += h_cnt[i];
    }
    APS_REQUIRE(pool_rows < ((int64_t)1 << 31), APS_E_DIM, "too many descriptors for one call (%lld)", (long long)pool_rows);
    for (int64_t p = 0; p < n_pairs; ++p)
        APS_REQUIRE(pa[p] >= 0 && pa[p] < n_img && pb[p] >= 0 && pb[p] < n_img && pa[p] != pb[p], APS_E_ARG,
                    "pair %lld = (%d,%d) is not a valid pair of distinct images", (long long)p, pa[p], pb[p]);

    // ---- the tables: sets that meet a non-empty partner, pairs, jobs, chunks of pairs under the column bound ----
    std::vector<HpSet> sets;
    std::vector<int> set_img;  // sets[s] is image set_img[s]
    std::vector<int64_t> set_row0(n_img, -1);
    std::vector<HpPair> pairs((size_t)n_pairs);
    std::vector<HpJob> jobs;
    std::vector<unsigned int> word_start((size_t)n_pairs + 1);
    struct Chunk {
        int64_t job0, job1, cols;
    };
    std::vector<Chunk> chunks;
    int64_t pool = 0, max_rows = 0;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int ia = pa[p], ib = pb[p];
        const bool empty = h_cnt[ia] == 0 || h_cnt[ib] == 0;  // matchFeaturesScratch.m:84-88
        word_start[p] = (unsigned int)(jobs.size() * (kRowBlock / 64));
        if (empty) {
            pairs[p] = HpPair{0, 0, 0, 0, 0};
            continue;
        }
        for (int i : {ia, ib})
            if (set_row0[i] < 0) {
                set_row0[i] = pool;
                sets.push_back(HpSet{nullptr, h_cnt[i], h_ld[i], pool});
                set_img.push_back(i);
                pool += h_cnt[i];
                max_rows = std::max(max_rows, h_cnt[i]);
            }
        if (chunks.empty() || chunks.back().cols + h_cnt[ib] > max_columns) chunks.push_back(Chunk{(int64_t)jobs.size(), 0, 0});
        pairs[p] = HpPair{(uint32_t)set_row0[ia], (uint32_t)h_cnt[ia], (uint32_t)set_row0[ib], (uint32_t)h_cnt[ib],
                          (unsigned long long)chunks.back().cols};
        for (int64_t r = 0; r < h_cnt[ia]; r += kRowBlock) jobs.push_back(HpJob{(uint32_t)p, (uint32_t)r});
        chunks.back().cols += h_cnt[ib];
        chunks.back().job1 = (int64_t)jobs.size();
        APS_REQUIRE((int64_t)jobs.size() * kRowBlock < ((int64_t)1 << 31), APS_E_DIM, "too many pair-rows for one call");
    }
    const int64_t n_jobs = (int64_t)jobs.size(), n_words = n_jobs * (kRowBlock / 64);
    word_start[n_pairs] = (unsigned int)n_words;
    *count = 0;
    if (n_jobs == 0) {  // no pair has two non-empty sides: an all-zero CSR, and no device work
        put_pair_ptr(pair_ptr, std::vector<int64_t>((size_t)n_pairs + 1, 0));
        return;
    }

    ctx();
    const int nw = nbytes <= 32 ? 8 : 16;
    const uint32_t nbits = o.nbits ? (uint32_t)o.nbits : 8u * nbytes;
    const HpRule rule{(float)o.max_ratio, (float)o.match_threshold, (float)nbits, nbits, 8u * nbytes, o.unique ? 1 : 0};
    std::vector<In<uint8_t>> din(sets.size());
    for (size_t s = 0; s < sets.size(); ++s) {
        const int i = set_img[s];
        const int64_t n = h_cnt[i];
        din[s].bind(h_desc[i], layout == APS_ROWMAJOR ? (size_t)(n - 1) * h_ld[i] + nbytes : (size_t)(nbytes - 1) * h_ld[i] + n);
        sets[s].src = din[s];
    }
    Ws<HpSet> d_sets(sets.size());
    Ws<HpPair> d_pairs((size_t)n_pairs);
    Ws<HpJob> d_jobs((size_t)n_jobs);
    Ws<unsigned int> d_word_start((size_t)n_pairs + 1);
    APS_HIP(hipMemcpyAsync(d_sets, sets.data(), sets.size() * sizeof(HpSet), hipMemcpyHostToDevice, stream()));
    APS_HIP(hipMemcpyAsync(d_pairs, pairs.data(), (size_t)n_pairs * sizeof(HpPair), hipMemcpyHostToDevice, stream()));
    APS_HIP(hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n_jobs * sizeof(HpJob), hipMemcpyHostToDevice, stream()));
    APS_HIP(hipMemcpyAsync(d_word_start, word_start.data(), ((size_t)n_pairs + 1) * sizeof(unsigned int), hipMemcpyHostToDevice, stream()));
    Ws<uint32_t> packed((size_t)pool * nw);
    {
        Prof prof("hamming_pairs_pack");
        hamming_pairs_pack_kernel<<<dim3((unsigned)sets.size(), std::min(cdiv((size_t)max_rows * nw, 256), 64u)), 256, 0, stream()>>>(
            d_sets, nbytes, layout, nw, packed);
        check_launch("hamming_pairs_pack_kernel");
    }
    int64_t max_cols = 0;
    for (const Chunk& c : chunks) max_cols = std::max(max_cols, c.cols);
    Ws<unsigned long long> cand((size_t)n_jobs * kRowBlock), bitmap((size_t)n_words + 1), col_bid(rule.unique ? (size_t)max_cols : 0);
    Ws<unsigned int> prefix((size_t)n_words + 1);
    APS_HIP(hipMemsetAsync(bitmap.get() + n_words, 0, sizeof(unsigned long long), stream()));  // (a zero word, whose prefix is the total)
    for (const Chunk& c : chunks) {  // same results for any chunking: a column's bids all come from its own pair
        const unsigned g = (unsigned)(c.job1 - c.job0);
        if (rule.unique) APS_HIP(hipMemsetAsync(col_bid, 0xFF, (size_t)c.cols * sizeof(unsigned long long), stream()));
        {
            Prof prof("hamming_pairs_search");
            if (nw == 8)
                hamming_pairs_search_kernel<8><<<g, kRowBlock, 0, stream()>>>(packed, d_pairs, d_jobs, c.job0, rule, cand, col_bid);
            else
                hamming_pairs_search_kernel<16><<<g, kRowBlock, 0, stream()>>>(packed, d_pairs, d_jobs, c.job0, rule, cand, col_bid);
            check_launch("hamming_pairs_search_kernel");
        }
        Prof prof("hamming_pairs_select");
        hamming_pairs_select_kernel<<<g, kRowBlock, 0, stream()>>>(d_pairs, d_jobs, c.job0, rule.unique, cand, col_bid, bitmap);
        check_launch("hamming_pairs_select_kernel");
    }
    Out<int64_t> optr(pair_ptr, (size_t)n_pairs + 1);
    {
        Prof prof("hamming_pairs_scan");
        exclusive_scan(popcounts(bitmap.get()), prefix.get(), 0u, (size_t)n_words + 1);
        hamming_pairs_ptr_kernel<<<cdiv((size_t)n_pairs + 1, 256), 256, 0, stream()>>>(prefix, d_word_start, n_pairs + 1, optr);
        check_launch("hamming_pairs_ptr_kernel");
    }
    const unsigned int total = read_back(prefix.get() + n_words);  // the one read-back of the chain
    optr.commit();
    *count = total;
    const bool write = idx_a && idx_b && metric;  // count-only otherwise
    if (total > 0 && ((int64_t)total > cap || !write))
        fail(APS_E_CAP, "output capacity %lld < %u matches", write ? (long long)cap : 0ll, total);
    if (total == 0) return;
    Ws<unsigned long long> keys(total), sorted_keys(total);
    Ws<uint32_t> cols(total), sorted_cols(total);
    {
        Prof prof("hamming_pairs_emit");
        hamming_pairs_emit_kernel<<<(unsigned)n_jobs, kRowBlock, 0, stream()>>>(d_jobs, cand, bitmap, prefix, keys, cols);
        check_launch("hamming_pairs_emit_kernel");
    }
    const unsigned long long* k_out = keys;
    const uint32_t* c_out = cols;
    if (rule.unique) {
        Prof prof("hamming_pairs_sort");
        int end_bit = kPairShift + 1;
        while (end_bit < 64 && ((int64_t)1 << (end_bit - kPairShift)) < n_pairs) ++end_bit;
        sort_pairs<unsigned int>(keys.get(), sorted_keys.get(), cols.get(), sorted_cols.get(), total, (unsigned int)end_bit);
        k_out = sorted_keys;
        c_out = sorted_cols;
    }
    Out<uint32_t> oa(idx_a, total), ob(idx_b, total);
    Out<float> om(metric, total);
    {
        Prof prof("hamming_pairs_unpack");
        hamming_pairs_unpack_kernel<<<cdiv(total, 256), 256, 0, stream()>>>(k_out, c_out, total, rule.nbits, oa, ob, om);
        check_launch("hamming_pairs_unpack_kernel");
    }
    oa.commit();
    ob.commit();
    om.commit();
    APS_HIP(hipStreamSynchronize(stream()));
}

}  // namespace
}  // namespace aps

using namespace aps;

extern "C" {

int aps_hamming_match_pairs(const uint8_t* const* desc, const int64_t* counts, const int64_t* ld, int n_img, int nbytes, int layout,
                            const int32_t* pair_a, const int32_t* pair_b, int64_t n_pairs, const aps_hamming_match_opts* opts,
                            int64_t* pair_ptr, uint32_t* idx_a, uint32_t* idx_b, float* metric, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(n_pairs <= 0 || (pair_a && pair_b), APS_E_ARG, "NULL pair list");
        static const int32_t none = 0;  // (an empty list is still a list: not the all-pairs form)
        hamming_pairs_impl(desc, counts, ld, n_img, nbytes, layout, pair_a ? pair_a : &none, pair_b ? pair_b : &none, n_pairs, opts,
                           pair_ptr, idx_a, idx_b, metric, cap, count);
    });
}

int aps_hamming_match_pairwise(const uint8_t* const* desc, const int64_t* counts, const int64_t* ld, int n_img, int nbytes, int layout,
                               const aps_hamming_match_opts* opts, int64_t* pair_ptr, uint32_t* idx_i, uint32_t* idx_j, float* metric,
                               int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(n_img >= 0, APS_E_ARG, "negative image count");
        hamming_pairs_impl(desc, counts, ld, n_img, nbytes, layout, nullptr, nullptr, (int64_t)n_img * (n_img - 1) / 2, opts, pair_ptr,
                           idx_i, idx_j, metric, cap, count);
    });
}

// Not part of the ABI (no declaration in aps.h): aps_hamming_match_pairs with the column bound of one chunk as an argument, for
// featureMatching.match_pairs_binary_csr(max_columns=...) - tests of the chunked walk.  pair_a = pair_b = NULL: all pairs.
int aps_hamming_match_pairs_bounded(const uint8_t* const* desc, const int64_t* counts, const int64_t* ld, int n_img, int nbytes, int layout,
                                    const int32_t* pair_a, const int32_t* pair_b, int64_t n_pairs, const aps_hamming_match_opts* opts,
                                    int64_t* pair_ptr, uint32_t* idx_a, uint32_t* idx_b, float* metric, int64_t cap, int64_t* count,
                                    int64_t max_columns) {
    return guarded([&] {
        APS_REQUIRE(n_img >= 0, APS_E_ARG, "negative image count");
        hamming_pairs_impl(desc, counts, ld, n_img, nbytes, layout, pair_a, pair_b, pair_a ? n_pairs : (int64_t)n_img * (n_img - 1) / 2,
                           opts, pair_ptr, idx_a, idx_b, metric, cap, count, max_columns);
    });
}

}  // extern "C"
