// fast.hip — FAST-9 corners + FREAK 512-bit (or, on request, ORB 256-bit) descriptors on the gfx950.
// Stands behind PP/featureMatching/getFeaturePoints.m:51-52,71-74 (rgb2gray -> detectFASTFeatures(gray) -> extractFeatures, which
// describes corner points with FREAK).  The toolbox functions are closed code; the algorithms are FAST-9 of Rosten & Drummond and
// FREAK of Alahi, Ortiz & Vandergheynst, restated in DESIGN.md "FAST/FREAK contract".  Every stored value and every discrete
// decision below is integer arithmetic (gray plane, ring differences, box sums, cross-multiplied comparisons, 64-bit moments), so
// a NumPy restatement (tests/fast_mirror.py) reproduces the outputs bit for bit: no device transcendental, no float summation.
// The pattern's f64 layout is rounded to integer tables on the host, once (aps_freak_pattern hands them to the tests).
//
// Chain of one call (no host read-back until the final counts; every grid is a capacity grid).  The call works on a plan of 1..16
// levels (FastPlan; aps_fast_extract's plan is level 0 alone, aps_fast_extract_pyramid's is DESIGN.md "FAST/FREAK scale pyramid")
// and on a group of 1..16 views of one shape, which share the plan (aps_fast_extract_batch; the single-view entries are groups of
// one).  Every stage is one launch for the group: the view is the last grid dimension or is decoded from the packed item's offset,
// as the level is.  The planes, score planes, integral images and bitmap words lie packed [view][level]:
//   integral_image        level 0: the u8 gray plane, stored once, and the exact 32-bit integral image (integral_dev.h, shared with
//                         surf.hip); level l >= 1: the integral image of the resampled plane
//   fast_resample_kernel  level l >= 1 from level l - 1: bilinear, half-pixel centres, 8-bit weights, integers only (one launch per
//                         level, each reads the one before)
//   fast_detect_kernel    64 x 8 tile of a level's plane (+4 halo: 3 for the ring, 1 for suppression) into LDS, the FAST-9 score of the
//                         tile (+1 halo) into LDS, strict 3 x 3 maximum; writes the plane of kept scores (0 = no corner); one launch
//                         over the tiles of all levels
//   fast_smax_kernel      segmented maximum of the score planes (integers): s_max of the quality gate per (view, level)
//   fast_gate_kernel      quality gate per pixel; one ballot = one 64-bit word of the candidate bitmap, whose bit order IS the
//                         canonical feature order (level, row, col) within the view
//   exclusive scan of all views' words' popcounts (rocprim), fast_emit_kernel (ordered compaction, no atomics, no sort; view and
//                         level are decoded from the word's offset)
//   group_rows_kernel     (group_dev.h) every view's count, first keypoint and rows to write: all views' or, if one does not fit, none
//   freak_keypoint_kernel one wave per keypoint: 43 box sums on its level's integral image, 45-pair orientation moment, bin, 43 box
//                         sums on the bin's table, 64 lanes x 8 tests = 512 bits; lane = output byte
// aps_fast_extract_strongest (DESIGN.md "FAST/FREAK strongest-N"; one view: its selection group is a level) shares the chain up to the
// scan, reads the counts per level back, and goes on with grids of the candidates' size:
//   fast_emit_kernel      the candidate list
//   fast_harris_kernel    one wave per candidate: integer Harris response of its level's plane, and the sort key (level, -R)
//   select_by_key         (select_dev.h, shared with sift.hip and surf.hip) stable radix sort (rocprim) of (key, index),
//                         strongest_flag_kernel (rank within the level < k_l, written back by index), strongest_word_kernel (ballot),
//                         scan of the popcounts; then strongest_compact_kernel (canonical order again)
//   freak_keypoint_kernel on the kept keypoints only; strongest_aux_kernel writes f32(R) into aux[3]
// aps_fast_orb_extract and aps_fast_orb_extract_batch (DESIGN.md "FAST/ORB contract") are these chains with another describer (Describer):
//   orb_keypoint_kernel   one wave per keypoint: the 31 x 31 patch of its level's plane into LDS, the intensity-centroid moments on the
//                         way, bin, a 27 x 27 plane of 5 x 5 box sums in LDS, 64 lanes x 4 steered tests = 256 bits in 32 bytes
// aps_corner_extract and aps_corner_extract_batch (DESIGN.md "Harris corner contract") are these chains with another detector in
// fast_front, whichever the describer and the selection:
//   harris_detect_kernel  64 x 8 tile (+5 halo) into LDS, the Sobel products once per pixel, 7 x 7 sums row pass then column pass, the
//                         64-bit response, strict 3 x 3 maximum; writes the int64 plane of candidate responses and, per wave, one
//                         atomic maximum into the (view, level)'s Rmax
//   harris_gate_kernel    R q_den >= Rmax q_num in 128 bits; the ballot is the bitmap word, as fast_gate_kernel's
//   harris_aux_kernel     aux[0] = f32(R) of the described rows
// aps_fast_extract_uniform (DESIGN.md "Uniform-N selection") is the strongest-N chain with fast_segment_kernel and select_uniform in the place of
// select_by_key: the k_l rows of a level are spread over the cells of a grid on the level's plane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "aps_internal.h"
#include "group_dev.h"
#include "integral_dev.h"
#include "select_dev.h"

namespace aps {
namespace {

constexpr int kTW = 64, kTH = 8;  // detection tile: a wave's row of it is one row of 64 pixels
constexpr int kHalo = 4;          // ring radius 3 + 1 for the suppression's neighbours
constexpr int kFields = 43, kBins = 256, kPairs = 512, kOriPairs = 45;
constexpr double kPatternScale = 22.0;
constexpr int kMaxLevels = 16;
constexpr int kRW = 64, kRH = 32;  // resampling tile: a wave's row of it is one row of 64 pixels

// ---- the plan: what every kernel knows about the levels (a kernel argument, by value) -------------------------------------
struct FastLevel {
    int h, w, wpr;           // plane size; bitmap words per row = detection tiles per row (both span 64 pixels)
    unsigned int tile0;      // first detection tile of this level
    unsigned int word0;      // first bitmap word: h rows of wpr words
    long long plane0;        // first byte of the u8 plane (and of the plane of kept scores)
    long long integ0;        // first element of the (h + 1) x (w + 1) integral image
};
// A call works on nv views of one shape, which share the levels; what a view holds is packed [view][level]: view v's items of a
// level start v * (the per-view total) after FastLevel's offsets.
struct FastPlan {
    int n, nv;
    unsigned int view_tiles, view_words;  // detection tiles and bitmap words of one view
    long long view_plane, view_integ;     // plane bytes and integral-image elements of one view
    FastLevel lv[kMaxLevels];
};
static_assert(kGroupViews == APS_FAST_MAX_VIEWS, "the group's tables hold kGroupViews views");
// the level that holds item q of a packed sequence (tiles or words): `first` is the member of FastLevel that starts it
__device__ __forceinline__ int level_of(const FastPlan& P, unsigned int FastLevel::*first, unsigned int q) {
    int l = 0;
    while (l + 1 < P.n && q >= P.lv[l + 1].*first) ++l;
    return l;
}

// ---- the pattern: f64 layout -> integer tables (host, once) ---------------------------------------------------------
struct FreakHost {
    int32_t fields[kBins][kFields][3];  // dx, dy, r
    int32_t pairs[kPairs][2];
    int32_t ori_pairs[kOriPairs][2];
    int32_t ori_dir[kOriPairs][2];
    int32_t cos_sin[kBins][2];
    int margin;
};
// what the keypoint kernel reads
struct FreakDev {
    char4 field[kBins][kFields];  // dx, dy, r, 0
    int area[kFields];            // (2r + 1)^2
    uchar2 pair[kPairs];
    uchar2 ori_pair[kOriPairs];
    short2 ori_dir[kOriPairs];
    short2 cos_sin[kBins];
};

inline int32_t round_half_up_f64(double v) { return (int32_t)std::floor(v + 0.5); }
inline int ring_of(int f) { return f < 42 ? f / 6 : 7; }

const FreakHost& host_pattern() {
    static const FreakHost t = [] {
        FreakHost p;
        std::memset(&p, 0, sizeof p);
        const double bigR = 2.0 / 3.0, smallR = 2.0 / 24.0, u = (bigR - smallR) / 21.0;
        const double steps[6] = {0, 6, 11, 15, 18, 20};
        double radius[8], px0[kFields], py0[kFields];
        for (int r = 0; r < 6; ++r) radius[r] = bigR - steps[r] * u;
        radius[6] = smallR;
        radius[7] = 0.0;
        // bins 0..63 from the f64 layout; 64..255 are exact quarter turns (dx, dy) -> (-dy, dx) of them
        for (int k = 0; k < 64; ++k)
            for (int f = 0; f < kFields; ++f) {
                const int r = ring_of(f), j = f % 6;
                const double th = (f < 42 ? (double)j * M_PI / 3.0 + (r & 1) * M_PI / 6.0 : 0.0) + 2.0 * M_PI * (double)k / 256.0;
                const double x = radius[r] * kPatternScale * std::cos(th), y = radius[r] * kPatternScale * std::sin(th);
                if (k == 0) {
                    px0[f] = x;
                    py0[f] = y;
                }
                const double sigma = (f < 42 ? radius[r] : smallR) / 2.0;  // the centre has the innermost ring's size
                int32_t dx = f < 42 ? round_half_up_f64(x) : 0, dy = f < 42 ? round_half_up_f64(y) : 0;
                const int32_t hs = round_half_up_f64(sigma * kPatternScale);
                for (int q = 0; q < 4; ++q) {
                    p.fields[k + 64 * q][f][0] = dx;
                    p.fields[k + 64 * q][f][1] = dy;
                    p.fields[k + 64 * q][f][2] = hs;
                    const int32_t t2 = dx;
                    dx = -dy;
                    dy = t2;
                }
            }
        p.margin = 0;
        for (int k = 0; k < kBins; ++k)
            for (int f = 0; f < kFields; ++f)
                p.margin = std::max(p.margin, std::max(std::abs(p.fields[k][f][0]), std::abs(p.fields[k][f][1])) + p.fields[k][f][2] + 1);
        // descriptor pairs: all (a, b), a < b, by ascending (ring(a) + ring(b), a, b) - ring 0 is the outermost; the first 512
        int n = 0;
        for (int s = 0; s <= 14 && n < kPairs; ++s)
            for (int a = 0; a < kFields && n < kPairs; ++a)
                for (int b = a + 1; b < kFields && n < kPairs; ++b)
                    if (ring_of(a) + ring_of(b) == s) {
                        p.pairs[n][0] = a;
                        p.pairs[n][1] = b;
                        ++n;
                    }
        // orientation pairs: all 15 pairs of the six fields of each of the three outer rings
        n = 0;
        for (int r = 0; r < 3; ++r)
            for (int a = 6 * r; a < 6 * r + 6; ++a)
                for (int b = a + 1; b < 6 * r + 6; ++b) {
                    p.ori_pairs[n][0] = a;
                    p.ori_pairs[n][1] = b;
                    const double ex = px0[a] - px0[b], ey = py0[a] - py0[b], len = std::sqrt(ex * ex + ey * ey);
                    p.ori_dir[n][0] = round_half_up_f64(1024.0 * ex / len);
                    p.ori_dir[n][1] = round_half_up_f64(1024.0 * ey / len);
                    ++n;
                }
        for (int k = 0; k < 64; ++k) {
            int32_t c = round_half_up_f64(16384.0 * std::cos(2.0 * M_PI * (double)k / 256.0));
            int32_t s = round_half_up_f64(16384.0 * std::sin(2.0 * M_PI * (double)k / 256.0));
            for (int q = 0; q < 4; ++q) {
                p.cos_sin[k + 64 * q][0] = c;
                p.cos_sin[k + 64 * q][1] = s;
                const int32_t t2 = c;
                c = -s;
                s = t2;
            }
        }
        return p;
    }();
    return t;
}

const FreakDev& dev_pattern() {
    static const FreakDev t = [] {
        const FreakHost& h = host_pattern();
        FreakDev d;
        std::memset(&d, 0, sizeof d);
        for (int k = 0; k < kBins; ++k) {
            for (int f = 0; f < kFields; ++f) d.field[k][f] = make_char4((signed char)h.fields[k][f][0], (signed char)h.fields[k][f][1], (signed char)h.fields[k][f][2], 0);
            d.cos_sin[k] = make_short2((short)h.cos_sin[k][0], (short)h.cos_sin[k][1]);
        }
        for (int f = 0; f < kFields; ++f) d.area[f] = (2 * h.fields[0][f][2] + 1) * (2 * h.fields[0][f][2] + 1);
        for (int i = 0; i < kPairs; ++i) d.pair[i] = make_uchar2((unsigned char)h.pairs[i][0], (unsigned char)h.pairs[i][1]);
        for (int i = 0; i < kOriPairs; ++i) {
            d.ori_pair[i] = make_uchar2((unsigned char)h.ori_pairs[i][0], (unsigned char)h.ori_pairs[i][1]);
            d.ori_dir[i] = make_short2((short)h.ori_dir[i][0], (short)h.ori_dir[i][1]);
        }
        return d;
    }();
    return t;
}

// ---- detection --------------------------------------------------------------------------------------------------------
// the 16-pixel Bresenham circle of radius 3, clockwise from the top (image coordinates: x right, y down)
// (constexpr: every use has a constant index after unrolling, so the offsets fold into the LDS addresses)
constexpr int kRingDx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
constexpr int kRingDy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};

// dst (hd x wd) from src (hs x ws), hd <= hs, wd <= ws: the contract's bilinear resampling.  The first 96 threads of a 64 x 32 tile
// work out its 64 column and 32 row entries (first tap, 8-bit weight), one 64-bit division each; then a wave takes a row at a time.
// blockIdx.z is the view: its planes lie view_plane bytes after the first view's.
__global__ __launch_bounds__(256) void fast_resample_kernel(const uint8_t* __restrict__ src, int hs, int ws, uint8_t* __restrict__ dst,
                                                            int hd, int wd, long long view_plane) {
    __shared__ int2 s_x[kRW], s_y[kRH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    src += blockIdx.z * view_plane;
    dst += blockIdx.z * view_plane;
    const int x0 = blockIdx.x * kRW, y0 = blockIdx.y * kRH;
    if (tid < kRW + kRH) {
        const bool col = tid < kRW;
        const long long i = col ? x0 + tid : y0 + tid - kRW, ns = col ? ws : hs, nd = col ? wd : hd;
        int2 e = make_int2(0, 0);
        if (i < nd) {
            const long long X = (2 * i + 1) * ns - nd;  // >= 0, as ns >= nd
            const long long t0 = X / (2 * nd), f = X - 2 * nd * t0;
            e = make_int2((int)t0, (int)(256 * f / (2 * nd)));
        }
        if (col)
            s_x[tid] = e;
        else
            s_y[tid - kRW] = e;
    }
    __syncthreads();
    const int x = x0 + lane;
    if (x >= wd) return;
    const int2 ex = s_x[lane];
    const int xa = min(ex.x, ws - 1), xb = min(ex.x + 1, ws - 1);
    const unsigned int wx = (unsigned int)ex.y;
    for (int r = wave; r < kRH; r += 4) {
        const int y = y0 + r;
        if (y >= hd) break;  // (uniform in the wave)
        const int2 ey = s_y[r];
        const size_t ra = (size_t)min(ey.x, hs - 1) * ws, rb = (size_t)min(ey.x + 1, hs - 1) * ws;
        const unsigned int wy = (unsigned int)ey.y;
        const unsigned int top = (256u - wx) * src[ra + xa] + wx * src[ra + xb], bot = (256u - wx) * src[rb + xa] + wx * src[rb + xb];
        dst[(size_t)y * wd + x] = (uint8_t)(((256u - wy) * top + wy * bot + 32768u) >> 16);
    }
}

__global__ __launch_bounds__(256) void fast_detect_kernel(const uint8_t* __restrict__ planes, const FastPlan P, int thr, int margin,
                                                          uint8_t* __restrict__ kept_all) {
    __shared__ uint8_t G[kTH + 2 * kHalo][kTW + 2 * kHalo];
    __shared__ uint8_t S[kTH + 2][kTW + 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned int view = blockIdx.x / P.view_tiles, vtile = blockIdx.x - view * P.view_tiles;
    const FastLevel& L = P.lv[level_of(P, &FastLevel::tile0, vtile)];
    const unsigned int tile = vtile - L.tile0;
    const int h = L.h, w = L.w;
    const int x0 = (int)(tile % L.wpr) * kTW, y0 = (int)(tile / L.wpr) * kTH;
    const uint8_t* __restrict__ gray = planes + view * P.view_plane + L.plane0;
    uint8_t* __restrict__ kept = kept_all + view * P.view_plane + L.plane0;
    constexpr int kGW = kTW + 2 * kHalo, kGN = (kTH + 2 * kHalo) * kGW;
    for (int e = tid; e < kGN; e += 256) {
        const int r = e / kGW, cc = e % kGW, y = y0 - kHalo + r, x = x0 - kHalo + cc;
        G[r][cc] = y >= 0 && y < h && x >= 0 && x < w ? gray[(size_t)y * w + x] : (uint8_t)0;
    }
    __syncthreads();
    constexpr int kSW = kTW + 2, kSN = (kTH + 2) * kSW;
    for (int e = tid; e < kSN; e += 256) {
        const int r = e / kSW, cc = e % kSW, y = y0 - 1 + r, x = x0 - 1 + cc;
        int s = 0;
        // pixels closer than the descriptor's margin to the edge are never corners (margin >= 4: the ring stays inside the image)
        if (y >= margin && y <= h - 1 - margin && x >= margin && x <= w - 1 - margin) {
            const int ctr = G[r + 3][cc + 3];
            int d[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) d[i] = (int)G[r + 3 + kRingDy[i]][cc + 3 + kRingDx[i]] - ctr;
#pragma unroll
            for (int a = 0; a < 16; ++a) {
                int mb = 255, md = 255;
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    mb = min(mb, d[(a + j) & 15]);
                    md = min(md, -d[(a + j) & 15]);
                }
                s = max(s, max(mb, md));
            }
            if (s <= thr) s = 0;
        }
        S[r][cc] = (uint8_t)s;
    }
    __syncthreads();
    for (int rr = wave; rr < kTH; rr += 4) {
        const int y = y0 + rr, x = x0 + lane;
        if (y >= h) break;  // (uniform in the wave)
        const int v = S[rr + 1][lane + 1];
        bool keep = v > 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
                if (!(dy == 1 && dx == 1)) keep = keep && v > (int)S[rr + dy][lane + dx];
        if (x < w) kept[(size_t)y * w + x] = keep ? (uint8_t)v : (uint8_t)0;
    }
}

// s_max of the quality gate for every (view, level), smax[view * P.n + level] (zeroed by the caller): the segmented maximum of the
// packed planes of kept scores in one launch.  blockIdx.x is a chunk of kSmaxChunk bytes of the view blockIdx.y; of every level the
// chunk meets, a wave takes the maximum of its bytes (words where they are aligned) and hands it over with one atomic maximum - of
// integers, so the result does not depend on the order.
constexpr long long kSmaxChunk = 1 << 16;
__global__ __launch_bounds__(256) void fast_smax_kernel(const uint8_t* __restrict__ kept, const FastPlan P, unsigned int* __restrict__ smax) {
    const int tid = threadIdx.x, lane = tid & 63;
    const long long c0 = (long long)blockIdx.x * kSmaxChunk, c1 = min(c0 + kSmaxChunk, P.view_plane);
    const uint8_t* __restrict__ p = kept + blockIdx.y * P.view_plane;
    for (int l = 0; l < P.n; ++l) {
        const long long lo = max(c0, P.lv[l].plane0), hi = min(c1, l + 1 < P.n ? P.lv[l + 1].plane0 : P.view_plane);
        if (lo >= hi) continue;  // (uniform in the workgroup)
        // [lo, a) and [b, hi) byte by byte, [a, b) as aligned words
        const long long mis = (long long)((4 - ((uintptr_t)(p + lo) & 3)) & 3), a = min(lo + mis, hi), b = a + ((hi - a) & ~3LL);
        unsigned int m = 0;
        for (long long i = a + 4LL * tid; i < b; i += 4 * 256) {
            const unsigned int v = *reinterpret_cast<const unsigned int*>(p + i);
            m = max(max(m, v & 255u), max(max((v >> 8) & 255u, (v >> 16) & 255u), v >> 24));
        }
        if (lo + tid < a) m = max(m, (unsigned int)p[lo + tid]);
        if (b + tid < hi) m = max(m, (unsigned int)p[b + tid]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, off));
        if (lane == 0 && m) atomicMax(&smax[blockIdx.y * P.n + l], m);
    }
}

// keep iff s * q_den >= s_max * q_num, s_max being that of the view's level (d_smax[view * P.n + level]); one wave per bitmap word =
// row segment of 64 pixels, its ballot is the word
__global__ __launch_bounds__(256) void fast_gate_kernel(const uint8_t* __restrict__ kept, const FastPlan P, unsigned int n_words,
                                                        const unsigned int* __restrict__ d_smax, unsigned int q_num, unsigned int q_den,
                                                        unsigned long long* __restrict__ bitmap) {
    const int lane = threadIdx.x & 63;
    const unsigned int q = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (q >= n_words) return;  // (uniform in the wave)
    const unsigned int view = q / P.view_words, qv = q - view * P.view_words;
    const int l = level_of(P, &FastLevel::word0, qv);
    const FastLevel& L = P.lv[l];
    const unsigned int ql = qv - L.word0;
    const int y = (int)(ql / L.wpr), x = (int)(ql % L.wpr) * 64 + lane;
    const unsigned long long smax = d_smax[view * P.n + l];
    const unsigned long long s = x < L.w ? kept[view * P.view_plane + L.plane0 + (size_t)y * L.w + x] : 0;
    const unsigned long long mask = __ballot(s > 0 && s * q_den >= smax * q_num);
    if (lane == 0) bitmap[q] = mask;
}

struct Keypoint {
    int y, x, level, view;
};

// Ordered compaction: bit k of word q (of n_words, all views') becomes keypoint prefix[q] + (set bits below k) as (view, level, row,
// col); the view and the level are decoded from the word's offset.
__global__ __launch_bounds__(256) void fast_emit_kernel(const unsigned long long* __restrict__ bitmap, const unsigned int* __restrict__ prefix,
                                                        const FastPlan P, unsigned int n_words, Keypoint* __restrict__ kps, unsigned int kcap) {
    const unsigned int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_words) return;
    unsigned long long bits = bitmap[q];
    if (!bits) return;
    unsigned int pos = prefix[q];
    const unsigned int view = q / P.view_words, qv = q - view * P.view_words;
    const int l = level_of(P, &FastLevel::word0, qv);
    const unsigned int ql = qv - P.lv[l].word0;
    const int y = (int)(ql / P.lv[l].wpr), xw = (int)(ql % P.lv[l].wpr) * 64;
    while (bits) {
        const int k = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        if (pos < kcap) kps[pos] = Keypoint{y, xw + k, l, (int)view};
        ++pos;
    }
}

// ---- description ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ long long wave_max(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// One wave per keypoint; blockIdx.y is the view, whose record (group_dev.h) says where its keypoints start and how many rows it
// writes.  Every wave of the capacity grid passes every barrier; the ones beyond the view's rows do no work.
__global__ __launch_bounds__(256) void freak_keypoint_kernel(const uint32_t* __restrict__ integ, const FastPlan P, const FreakDev* __restrict__ tb,
                                                             const uint8_t* __restrict__ kept, const Keypoint* __restrict__ kps,
                                                             const ViewRows<uint8_t>* __restrict__ views, int desc_layout, long long ldd,
                                                             long long ldl) {
    __shared__ int s_S[4][kFields + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ViewRows<uint8_t> V = views[blockIdx.y];
    const unsigned int kidx = blockIdx.x * 4 + wave;  // the row of the view
    const bool active = kidx < V.rows;
    uint8_t* __restrict__ desc = V.desc;
    double* __restrict__ loc = V.loc;
    float* __restrict__ aux = V.aux;
    integ += blockIdx.y * P.view_integ;
    kept += blockIdx.y * P.view_plane;
    Keypoint kp{0, 0, 0, 0};
    if (active) kp = kps[V.kp0 + kidx];
    const FastLevel& L = P.lv[__builtin_amdgcn_readfirstlane(kp.level)];  // (one keypoint per wave)
    const uint32_t* __restrict__ I = integ + L.integ0;
    const size_t ws = (size_t)L.w + 1;
    // the 43 box sums on the table of `bin`, one field per lane (the margin keeps every box inside the image)
    auto sums = [&](int bin) {
        if (active && lane < kFields) {
            const char4 f = tb->field[bin][lane];
            const int cy = kp.y + f.y, cx = kp.x + f.x, r = f.z;
            s_S[wave][lane] = (int)box(I, ws, cy - r, cy + r, cx - r, cx + r);
        }
    };
    sums(0);
    __syncthreads();
    // ---- orientation: 45 pairs on the bin-0 table, 64-bit moment, the bin that maximises its projection ---------------
    long long mx = 0, my = 0;
    if (active && lane < kOriPairs) {
        const uchar2 p = tb->ori_pair[lane];
        const short2 dir = tb->ori_dir[lane];
        const long long D = (long long)s_S[wave][p.x] * tb->area[p.y] - (long long)s_S[wave][p.y] * tb->area[p.x];
        mx = D * dir.x;
        my = D * dir.y;
    }
    mx = wave_sum(mx);
    my = wave_sum(my);
    // lane holds bins 4 * lane .. 4 * lane + 3: the lowest lane among equals holds the lowest bin among equals
    long long best = 0;
    int best_k = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const short2 cs = tb->cos_sin[4 * lane + j];
        const long long v = mx * cs.x + my * cs.y;
        if (j == 0 || v > best) {
            best = v;
            best_k = 4 * lane + j;
        }
    }
    const long long top = wave_max(best);
    const unsigned long long tie = __ballot(best == top);
    const int bin = __shfl(best_k, __ffsll((long long)tie) - 1);
    __syncthreads();  // (the bin-0 sums are read; the slice is written again)
    sums(bin);
    __syncthreads();
    if (!active) return;
    // ---- descriptor: lane = output byte, bits 8 * lane .. 8 * lane + 7, LSB first ---------------------------------------
    unsigned int byte = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uchar2 p = tb->pair[8 * lane + t];
        const long long a = (long long)s_S[wave][p.x] * tb->area[p.y], b = (long long)s_S[wave][p.y] * tb->area[p.x];
        byte |= (a > b ? 1u : 0u) << t;
    }
    if (desc_layout == APS_ROWMAJOR)
        desc[(size_t)kidx * ldd + lane] = (uint8_t)byte;
    else
        desc[(size_t)lane * ldd + kidx] = (uint8_t)byte;
    if (lane == 0) {
        // the pixel's centre in level-0 coordinates, 1-based: one division, one addition (level 0: x + 1 exactly)
        loc[kidx] = (double)((2LL * kp.x + 1) * P.lv[0].w) / (double)(2LL * L.w) + 0.5;
        loc[(size_t)ldl + kidx] = (double)((2LL * kp.y + 1) * P.lv[0].h) / (double)(2LL * L.h) + 0.5;
        if (aux) {
            aux[(size_t)kidx * 4 + 0] = (float)kept[L.plane0 + (size_t)kp.y * L.w + kp.x];
            aux[(size_t)kidx * 4 + 1] = (float)bin;
            aux[(size_t)kidx * 4 + 2] = (float)kp.level;
            aux[(size_t)kidx * 4 + 3] = 0.0f;
        }
    }
}

// ---- strongest-N: Harris response and selection (DESIGN.md "FAST/FREAK strongest-N") ------------------------------------------
constexpr int kHarrisWin = 7, kHarrisPatch = kHarrisWin + 2;  // window of the sums; with the Sobel taps a 9 x 9 patch, reach 4
constexpr long long kHarrisBias = 1LL << 54;                  // R + 2^54 > 0
constexpr unsigned long long kKeyMask = (1ULL << 60) - 1;     // key = group << 60 | (2^60 - 1 - (R + 2^54)): ascending key = descending R

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One wave per candidate: its level's 9 x 9 patch into LDS, lanes 0..48 one window pixel each (Sobel Ix, Iy), three wave sums
// (49 * 1020^2 < 2^26: int32), R in 64 bits on lane 0.  Writes the response, the sort key and the candidate's index as the sort's value.
// Every wave of the grid passes the barrier; the ones beyond n do no work.  margin >= 4 keeps the patch inside the plane.
__global__ __launch_bounds__(256) void fast_harris_kernel(const uint8_t* __restrict__ planes, const FastPlan P, const Keypoint* __restrict__ kps,
                                                          unsigned int n, long long* __restrict__ resp, unsigned long long* __restrict__ keys,
                                                          unsigned int* __restrict__ vals) {
    __shared__ int s_g[4][kHarrisPatch * kHarrisPatch + 3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned int kidx = blockIdx.x * 4 + wave;
    const bool active = kidx < n;
    Keypoint kp{0, 0, 0, 0};
    if (active) kp = kps[kidx];
    const FastLevel& L = P.lv[__builtin_amdgcn_readfirstlane(kp.level)];  // (one candidate per wave)
    const uint8_t* __restrict__ g = planes + kp.view * P.view_plane + L.plane0;
    if (active) {
        for (int e = lane; e < kHarrisPatch * kHarrisPatch; e += 64) {
            const int r = e / kHarrisPatch, c = e % kHarrisPatch;
            s_g[wave][e] = g[(size_t)(kp.y - 4 + r) * L.w + (kp.x - 4 + c)];
        }
    }
    __syncthreads();
    int a = 0, b = 0, c = 0;
    if (active && lane < kHarrisWin * kHarrisWin) {
        const int* p = &s_g[wave][(lane / kHarrisWin) * kHarrisPatch + lane % kHarrisWin];  // top-left of the pixel's 3 x 3
        const int g00 = p[0], g01 = p[1], g02 = p[2];
        const int g10 = p[kHarrisPatch], g12 = p[kHarrisPatch + 2];
        const int g20 = p[2 * kHarrisPatch], g21 = p[2 * kHarrisPatch + 1], g22 = p[2 * kHarrisPatch + 2];
        const int ix = (g02 + 2 * g12 + g22) - (g00 + 2 * g10 + g20);
        const int iy = (g20 + 2 * g21 + g22) - (g00 + 2 * g01 + g02);
        a = ix * ix;
        b = iy * iy;
        c = ix * iy;
    }
    const long long A = wave_sum_i32(a), B = wave_sum_i32(b), Cxy = wave_sum_i32(c);
    if (active && lane == 0) {
        const long long R = 25 * (A * B - Cxy * Cxy) - (A + B) * (A + B);
        resp[kidx] = R;
        keys[kidx] = (unsigned long long)kp.level << 60 | (kKeyMask - (unsigned long long)(R + kHarrisBias));
        vals[kidx] = kidx;
    }
}

// the first candidate of every level and the total, gathered for the one read-back of the counts: out[l], l = 0 .. P.n
__global__ void strongest_counts_kernel(const unsigned int* __restrict__ prefix, const FastPlan P, unsigned int n_words,
                                        unsigned int* __restrict__ out) {
    const int l = threadIdx.x;
    if (l < P.n)
        out[l] = prefix[P.lv[l].word0];
    else if (l == P.n)
        out[l] = prefix[n_words];
}

// Uniform-N (DESIGN.md "Uniform-N selection"): the segment of every candidate = level * cells + the cell of its level pixel in the
// rows x cols grid over the level's plane.
__global__ __launch_bounds__(256) void fast_segment_kernel(const Keypoint* __restrict__ kps, const FastPlan P, unsigned int n, int rows, int cols,
                                                           unsigned int* __restrict__ segs) {
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Keypoint kp = kps[i];
    int h = 1, w = 1;
#pragma unroll
    for (int l = 0; l < kMaxLevels; ++l)  // (constant indices: the plan stays in scalar registers)
        if (kp.level == l) {
            h = P.lv[l].h;
            w = P.lv[l].w;
        }
    segs[i] = (unsigned int)(kp.level * rows * cols + uniform_cell(kp.y, kp.x, h, w, rows, cols));
}

static_assert(kMaxLevels == kSelectGroups, "a level is a group of the selection (select_dev.h: StrongestCut, strongest_flag_kernel)");

// Ordered compaction of the flagged candidates, as fast_emit_kernel's: canonical order is kept.
__global__ __launch_bounds__(256) void strongest_compact_kernel(const unsigned long long* __restrict__ words, const unsigned int* __restrict__ prefix,
                                                                unsigned int n_words, const Keypoint* __restrict__ cand,
                                                                const long long* __restrict__ resp, Keypoint* __restrict__ kps,
                                                                long long* __restrict__ kresp, unsigned int kcap) {
    const unsigned int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_words) return;
    unsigned long long bits = words[q];
    unsigned int pos = prefix[q];
    while (bits) {
        const int k = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        if (pos < kcap) {
            kps[pos] = cand[q * 64 + k];
            kresp[pos] = resp[q * 64 + k];
        }
        ++pos;
    }
}

// aux[3] of the described rows: f32(R), round to nearest
__global__ __launch_bounds__(256) void strongest_aux_kernel(const long long* __restrict__ kresp, unsigned int n, float* __restrict__ aux) {
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) aux[(size_t)i * 4 + 3] = (float)kresp[i];
}

// ---- Harris corners: the dense detector (DESIGN.md "Harris corner contract") ----------------------------------------------------
constexpr int kHarrisR = kHarrisWin / 2;    // the window's reach: 3
constexpr int kHarrisHalo = kHarrisR + 2;   // Sobel 1 + window 3 + suppression 1
constexpr int kHarrisReach = kHarrisR + 1;  // of the response alone: the pixels whose 9 x 9 patch lies inside the plane have one

// 64 x 8 tile of a level's plane, tiles and grid as fast_detect_kernel's.  Stages, each over its own region of LDS:
//   G   (8 + 10) x (64 + 10)  the gray tile, 0 outside the plane
//   Pa, Pb, Pc  (8 + 8) x (64 + 8)   ix^2, iy^2, ix iy of the Sobel taps, once per pixel
//   Ha, Hb, Hc  (8 + 8) x (64 + 2)   their sums over 7 columns
//   R   (8 + 2) x (64 + 2)    the sums over 7 rows -> A, B, C (int32: 49 * 1020^2 < 2^26) -> R = 25 (A B - C^2) - (A + B)^2, int64;
//                             item e of the pass reads H[e + dy * 66]: consecutive lanes, consecutive banks, rows included
//   suppression               a band pixel stays iff R > 0 and R > the eight neighbours' R
// kDense = false: `out` is the plane of candidates (R at candidates, else 0) and every wave hands its largest candidate R to
// rmax[view * P.n + level] (zeroed by the caller) with one atomic maximum - of integers, so the result does not depend on the order.
// kDense = true (aps_harris_planes): `out` is R wherever the 9 x 9 patch lies inside the plane, else 0; rmax is not touched.
// Integers only.  A band pixel's neighbours all have their patch inside the plane (margin >= kHarrisHalo), so the zeros outside
// the plane reach no value that a band pixel is compared with.
template <bool kDense>
__global__ __launch_bounds__(256) void harris_detect_kernel(const uint8_t* __restrict__ planes, const FastPlan P, int margin,
                                                            long long* __restrict__ out_all, unsigned long long* __restrict__ rmax) {
    constexpr int kGH = kTH + 2 * kHarrisHalo, kGW = kTW + 2 * kHarrisHalo;  // 18 x 74
    constexpr int kPH = kTH + 2 * kHarrisReach, kPW = kTW + 2 * kHarrisReach;  // 16 x 72
    constexpr int kRH2 = kTH + 2, kRW2 = kTW + 2;                              // 10 x 66
    __shared__ uint8_t G[kGH][kGW];
    __shared__ int Pa[kPH * kPW], Pb[kPH * kPW], Pc[kPH * kPW];
    __shared__ int Ha[kPH * kRW2], Hb[kPH * kRW2], Hc[kPH * kRW2];
    __shared__ long long R[kRH2][kRW2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned int view = blockIdx.x / P.view_tiles, vtile = blockIdx.x - view * P.view_tiles;
    const int l = level_of(P, &FastLevel::tile0, vtile);
    const FastLevel& L = P.lv[l];
    const unsigned int tile = vtile - L.tile0;
    const int h = L.h, w = L.w;
    const int x0 = (int)(tile % L.wpr) * kTW, y0 = (int)(tile / L.wpr) * kTH;
    const uint8_t* __restrict__ gray = planes + view * P.view_plane + L.plane0;
    long long* __restrict__ out = out_all + view * P.view_plane + L.plane0;
    // the pixels that can hold a value: the band, or for the dense plane the pixels with a patch (both uniform in the workgroup)
    const int edge = kDense ? kHarrisReach : margin;
    if (y0 + kTH - 1 < edge || y0 > h - 1 - edge || x0 + kTW - 1 < edge || x0 > w - 1 - edge) {
        for (int rr = wave; rr < kTH; rr += 4) {
            const int y = y0 + rr, x = x0 + lane;
            if (y >= h) break;  // (uniform in the wave)
            if (x < w) out[(size_t)y * w + x] = 0;
        }
        return;
    }
    for (int e = tid; e < kGH * kGW; e += 256) {
        const int r = e / kGW, cc = e % kGW, y = y0 - kHarrisHalo + r, x = x0 - kHarrisHalo + cc;
        G[r][cc] = y >= 0 && y < h && x >= 0 && x < w ? gray[(size_t)y * w + x] : (uint8_t)0;
    }
    __syncthreads();
    for (int e = tid; e < kPH * kPW; e += 256) {
        const int r = e / kPW, cc = e % kPW;  // product (r, cc) is pixel (y0 - 4 + r, x0 - 4 + cc): G[r + 1][cc + 1]
        const int g00 = G[r][cc], g01 = G[r][cc + 1], g02 = G[r][cc + 2];
        const int g10 = G[r + 1][cc], g12 = G[r + 1][cc + 2];
        const int g20 = G[r + 2][cc], g21 = G[r + 2][cc + 1], g22 = G[r + 2][cc + 2];
        const int ix = (g02 + 2 * g12 + g22) - (g00 + 2 * g10 + g20);
        const int iy = (g20 + 2 * g21 + g22) - (g00 + 2 * g01 + g02);
        Pa[e] = ix * ix;
        Pb[e] = iy * iy;
        Pc[e] = ix * iy;
    }
    __syncthreads();
    for (int e = tid; e < kPH * kRW2; e += 256) {
        const int r = e / kRW2, cc = e % kRW2, p = r * kPW + cc;  // columns cc .. cc + 6 of the products: centred on x0 - 1 + cc
        int a = 0, b = 0, c = 0;
#pragma unroll
        for (int d = 0; d < kHarrisWin; ++d) {
            a += Pa[p + d];
            b += Pb[p + d];
            c += Pc[p + d];
        }
        Ha[e] = a;
        Hb[e] = b;
        Hc[e] = c;
    }
    __syncthreads();
    for (int e = tid; e < kRH2 * kRW2; e += 256) {
        int a = 0, b = 0, c = 0;  // rows r .. r + 6 of the column sums: centred on y0 - 1 + r
#pragma unroll
        for (int d = 0; d < kHarrisWin; ++d) {
            a += Ha[e + d * kRW2];
            b += Hb[e + d * kRW2];
            c += Hc[e + d * kRW2];
        }
        const long long A = a, B = b, Cxy = c;
        R[e / kRW2][e % kRW2] = 25 * (A * B - Cxy * Cxy) - (A + B) * (A + B);
    }
    __syncthreads();
    long long best = 0;
    for (int rr = wave; rr < kTH; rr += 4) {
        const int y = y0 + rr, x = x0 + lane;
        if (y >= h) break;  // (uniform in the wave)
        const long long v = R[rr + 1][lane + 1];
        bool keep = y >= edge && y <= h - 1 - edge && x >= edge && x <= w - 1 - edge;
        if (!kDense) {
            keep = keep && v > 0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx)
                    if (!(dy == 1 && dx == 1)) keep = keep && v > R[rr + dy][lane + dx];
            if (keep && v > best) best = v;
        }
        if (x < w) out[(size_t)y * w + x] = keep ? v : 0;
    }
    if (!kDense) {
        // every wave of every tile would queue on the one address: the atomic is issued only where the maximum as it stands is
        // smaller (a stale reading costs a needless atomic, never a wrong result)
        best = wave_max(best);
        unsigned long long* top = &rmax[view * P.n + l];
        if (lane == 0 && best > 0 && (unsigned long long)best > __hip_atomic_load(top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(top, (unsigned long long)best);
    }
}

// a >= b for the 128-bit products a = a0 * a1, b = b0 * b1
__device__ __forceinline__ bool product_ge(unsigned long long a0, unsigned long long a1, unsigned long long b0, unsigned long long b1) {
    const unsigned long long ah = __umul64hi(a0, a1), al = a0 * a1, bh = __umul64hi(b0, b1), bl = b0 * b1;
    return ah > bh || (ah == bh && al >= bl);
}

// keep iff R * q_den >= Rmax * q_num, exactly (the products pass 2^64), Rmax being that of the view's level; one wave per bitmap
// word = row segment of 64 pixels, its ballot is the word - as fast_gate_kernel
__global__ __launch_bounds__(256) void harris_gate_kernel(const long long* __restrict__ cand, const FastPlan P, unsigned int n_words,
                                                          const unsigned long long* __restrict__ d_rmax, unsigned int q_num, unsigned int q_den,
                                                          unsigned long long* __restrict__ bitmap) {
    const int lane = threadIdx.x & 63;
    const unsigned int q = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (q >= n_words) return;  // (uniform in the wave)
    const unsigned int view = q / P.view_words, qv = q - view * P.view_words;
    const int l = level_of(P, &FastLevel::word0, qv);
    const FastLevel& L = P.lv[l];
    const unsigned int ql = qv - L.word0;
    const int y = (int)(ql / L.wpr), x = (int)(ql % L.wpr) * 64 + lane;
    const unsigned long long top = d_rmax[view * P.n + l];
    const long long r = x < L.w ? cand[view * P.view_plane + L.plane0 + (size_t)y * L.w + x] : 0;
    const unsigned long long mask = __ballot(r > 0 && product_ge((unsigned long long)r, q_den, top, q_num));
    if (lane == 0) bitmap[q] = mask;
}

// aux[0] of the described rows of a Harris chain: f32(R), round to nearest, from the candidate plane (a kept row is a candidate).
// The view in blockIdx.y and its record, as the keypoint kernels.
__global__ __launch_bounds__(256) void harris_aux_kernel(const long long* __restrict__ cand, const FastPlan P, const Keypoint* __restrict__ kps,
                                                         const ViewRows<uint8_t>* __restrict__ views) {
    const ViewRows<uint8_t> V = views[blockIdx.y];
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V.rows || !V.aux) return;
    const Keypoint kp = kps[V.kp0 + i];
    int w = 1;
    long long plane0 = 0;
#pragma unroll
    for (int l = 0; l < kMaxLevels; ++l)  // (constant indices: the plan stays in scalar registers)
        if (kp.level == l) {
            w = P.lv[l].w;
            plane0 = P.lv[l].plane0;
        }
    V.aux[(size_t)i * 4] = (float)cand[blockIdx.y * P.view_plane + plane0 + (size_t)kp.y * w + kp.x];
}

// ---- ORB: intensity-centroid orientation and steered BRIEF, 256 bits (DESIGN.md "FAST/ORB contract") -------------------------
constexpr int kOrbTests = 256, kOrbBytes = 32;
constexpr int kOrbDiscR = 15, kOrbDisc = 709;        // the moments' disc u^2 + v^2 <= 225 and its pixels
constexpr int kOrbRadius = 13, kOrbBoxR = 2;         // test points lie in x^2 + y^2 <= 169, steered or not; S is a 5 x 5 box sum
constexpr int kOrbReach = kOrbRadius + kOrbBoxR + 1;
constexpr int kOrbPatch = 2 * kOrbDiscR + 1, kOrbPatchLd = 32;  // the 31 x 31 patch in LDS, rows of 32 bytes
constexpr int kOrbSums = 2 * kOrbRadius + 1;                    // the 27 x 27 plane of box sums
constexpr int kFreakMargin = 23;  // host_pattern().margin: the candidates are those of the FREAK entries (orb_describe checks it)
static_assert(kOrbReach == 16 && kOrbReach <= kFreakMargin, "the descriptor's reach stays within the margin of the candidates");
static_assert(kOrbDiscR <= kFreakMargin, "the staged patch stays inside the level's plane");
static_assert(kOrbRadius + kOrbBoxR <= kOrbDiscR, "every box sum lies within the staged patch");
static_assert(kOrbPatch <= kOrbPatchLd && 2 * kOrbSums <= 64 && kOrbTests == 4 * 64, "orb_keypoint_kernel's lane maps");

// what the keypoint kernel reads: the steered tests of bins 0..63 (the quarter turns are applied in the kernel) and FREAK's cos_sin
struct OrbDev {
    char4 test[64][kOrbTests];  // dxa, dya, dxb, dyb
    short2 cos_sin[kBins];
};
struct OrbTables {
    int32_t tests[kOrbTests][4];  // xa, ya, xb, yb
    OrbDev dev;
    int reach;
    OrbTables() {
        std::memset(this, 0, sizeof *this);
        // the contract's generator: a stated deviation from the trained table, as FREAK's pairs are
        unsigned long long s = 1;
        const auto draw = [&] {
            s = (1103515245ULL * s + 12345ULL) & 0x7fffffffULL;
            return (int)((s >> 16) % 27) - 13;
        };
        for (int n = 0; n < kOrbTests;) {
            const int xa = draw(), ya = draw(), xb = draw(), yb = draw();
            bool ok = xa * xa + ya * ya <= kOrbRadius * kOrbRadius && xb * xb + yb * yb <= kOrbRadius * kOrbRadius &&
                      (xa - xb) * (xa - xb) + (ya - yb) * (ya - yb) >= 16;
            for (int i = 0; ok && i < n; ++i) {
                const int32_t* t = tests[i];
                ok = !((t[0] == xa && t[1] == ya && t[2] == xb && t[3] == yb) || (t[0] == xb && t[1] == yb && t[2] == xa && t[3] == ya));
            }
            if (!ok) continue;
            tests[n][0] = xa, tests[n][1] = ya, tests[n][2] = xb, tests[n][3] = yb;
            ++n;
        }
        const FreakHost& h = host_pattern();
        int far = 0;
        for (int k = 0; k < kBins; ++k) dev.cos_sin[k] = make_short2((short)h.cos_sin[k][0], (short)h.cos_sin[k][1]);
        for (int k = 0; k < 64; ++k)
            for (int i = 0; i < kOrbTests; ++i) {
                int d[4];
                for (int j = 0; j < 4; j += 2) {
                    const int x = tests[i][j], y = tests[i][j + 1], c = h.cos_sin[k][0], sn = h.cos_sin[k][1];
                    d[j] = (x * c - y * sn + (1 << 13)) >> 14;  // (arithmetic shift)
                    d[j + 1] = (x * sn + y * c + (1 << 13)) >> 14;
                    far = std::max(far, std::max(std::abs(d[j]), std::abs(d[j + 1])));
                }
                dev.test[k][i] = make_char4((signed char)d[0], (signed char)d[1], (signed char)d[2], (signed char)d[3]);
            }
        reach = far + kOrbBoxR + 1;
    }
};
const OrbTables& orb_tables() {
    static const OrbTables t;
    return t;
}

// One wave per keypoint, the view in blockIdx.y and the row in blockIdx.x * 4 + wave, as freak_keypoint_kernel.  Every wave of the
// capacity grid passes every barrier; the ones beyond the view's rows do no work.  A wave's stages, each on its own slice of LDS:
//   the 31 x 31 patch of the level's plane, byte loads (lane = column, two rows at a time), with the two moments taken from the
//     loaded values on the way - every byte lies in rows y - 15 .. y + 15 and columns x - 15 .. x + 15 of the level's plane, which
//     the margin (23 >= 15) keeps inside it, so no load leaves the view's planes whatever the plane's byte offset
//   the bin, as FREAK's: 4 bins per lane, wave maximum, ballot
//   the 27 x 27 plane of 5 x 5 box sums (u16, <= 6375): 54 lanes, a column and half of the rows each, sliding down the patch
//   4 tests per lane on the bin's table (bins 64..255: the quarter turn of bin & 63's), a nibble each; even lanes write the byte
__global__ __launch_bounds__(256) void orb_keypoint_kernel(const uint8_t* __restrict__ planes, const FastPlan P, const OrbDev* __restrict__ tb,
                                                           const uint8_t* __restrict__ kept, const Keypoint* __restrict__ kps,
                                                           const ViewRows<uint8_t>* __restrict__ views, int desc_layout, long long ldd,
                                                           long long ldl) {
    __shared__ uint8_t s_g[4][kOrbPatch * kOrbPatchLd];
    __shared__ unsigned short s_S[4][kOrbSums * kOrbSums + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ViewRows<uint8_t> V = views[blockIdx.y];
    const unsigned int kidx = blockIdx.x * 4 + wave;  // the row of the view
    const bool active = kidx < V.rows;
    uint8_t* __restrict__ desc = V.desc;
    double* __restrict__ loc = V.loc;
    float* __restrict__ aux = V.aux;
    planes += blockIdx.y * P.view_plane;
    kept += blockIdx.y * P.view_plane;
    Keypoint kp{0, 0, 0, 0};
    if (active) kp = kps[V.kp0 + kidx];
    const FastLevel& L = P.lv[__builtin_amdgcn_readfirstlane(kp.level)];  // (one keypoint per wave)
    // ---- the patch and the moments: m10 = sum u g, m01 = sum v g over the disc (|m| <= 255 * 4528 < 2^21) -----------------
    int m10 = 0, m01 = 0;
    {
        const int c = lane & 31, r0 = lane >> 5;
        if (active && c < kOrbPatch) {
            const uint8_t* __restrict__ src = planes + L.plane0 + (size_t)(kp.y - kOrbDiscR + r0) * L.w + (kp.x - kOrbDiscR + c);
#pragma unroll
            for (int i = 0; i < (kOrbPatch + 1) / 2; ++i) {
                const int r = r0 + 2 * i;
                if (r < kOrbPatch) {
                    const int v = src[(size_t)(2 * i) * L.w];
                    s_g[wave][r * kOrbPatchLd + c] = (uint8_t)v;
                    const int du = c - kOrbDiscR, dv = r - kOrbDiscR;
                    if (du * du + dv * dv <= kOrbDiscR * kOrbDiscR) {
                        m10 += du * v;
                        m01 += dv * v;
                    }
                }
            }
        }
    }
    const long long mx = wave_sum_i32(m10), my = wave_sum_i32(m01);
    // lane holds bins 4 * lane .. 4 * lane + 3: the lowest lane among equals holds the lowest bin among equals
    long long best = 0;
    int best_k = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const short2 cs = tb->cos_sin[4 * lane + j];
        const long long v = mx * cs.x + my * cs.y;
        if (j == 0 || v > best) {
            best = v;
            best_k = 4 * lane + j;
        }
    }
    const long long top = wave_max(best);
    const unsigned long long tie = __ballot(best == top);
    const int bin = __shfl(best_k, __ffsll((long long)tie) - 1);
    __syncthreads();  // (the patch is written)
    // ---- S[r][c] = the box sum centred on patch pixel (r + 2, c + 2), offset (c - 13, r - 13) from the keypoint ------------
    if (active && lane < 2 * kOrbSums) {
        const int c = lane < kOrbSums ? lane : lane - kOrbSums, ra = lane < kOrbSums ? 0 : (kOrbSums + 1) / 2;
        const uint8_t* p = &s_g[wave][c];
        const auto hsum = [&](int r) {
            const uint8_t* q = p + r * kOrbPatchLd;
            return (int)q[0] + q[1] + q[2] + q[3] + q[4];
        };
        int h0 = hsum(ra), h1 = hsum(ra + 1), h2 = hsum(ra + 2), h3 = hsum(ra + 3);
#pragma unroll
        for (int i = 0; i < (kOrbSums + 1) / 2; ++i) {
            const int r = ra + i;
            if (r < kOrbSums) {
                const int h4 = hsum(r + 4);
                s_S[wave][r * kOrbSums + c] = (unsigned short)(h0 + h1 + h2 + h3 + h4);
                h0 = h1, h1 = h2, h2 = h3, h3 = h4;
            }
        }
    }
    __syncthreads();
    if (!active) return;
    // ---- descriptor: bit i = S(a_i) < S(b_i); lane holds tests 4 * lane .. 4 * lane + 3, bits (4 * lane) % 8 .. of byte lane / 2 ------
    const int q = bin >> 6, cq = q == 0 ? 1 : q == 2 ? -1 : 0, sq = q == 1 ? 1 : q == 3 ? -1 : 0;  // the quarter turn (dx, dy) -> (-dy, dx), q times
    const uint4 raw = *reinterpret_cast<const uint4*>(&tb->test[bin & 63][4 * lane]);
    const unsigned int words[4] = {raw.x, raw.y, raw.z, raw.w};
    const auto sum_at = [&](int dx, int dy) {
        const int x = dx * cq - dy * sq, y = dx * sq + dy * cq;
        return (int)s_S[wave][(y + kOrbRadius) * kOrbSums + x + kOrbRadius];
    };
    unsigned int nib = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const unsigned int w = words[t];
        const int a = sum_at((signed char)(w & 255u), (signed char)((w >> 8) & 255u));
        const int b = sum_at((signed char)((w >> 16) & 255u), (signed char)(w >> 24));
        nib |= (a < b ? 1u : 0u) << t;
    }
    const unsigned int byte = nib | (unsigned int)__shfl_xor((int)nib, 1) << 4;
    if (!(lane & 1)) {
        if (desc_layout == APS_ROWMAJOR)
            desc[(size_t)kidx * ldd + (lane >> 1)] = (uint8_t)byte;
        else
            desc[(size_t)(lane >> 1) * ldd + kidx] = (uint8_t)byte;
    }
    if (lane == 0) {
        // the pixel's centre in level-0 coordinates, as freak_keypoint_kernel's
        loc[kidx] = (double)((2LL * kp.x + 1) * P.lv[0].w) / (double)(2LL * L.w) + 0.5;
        loc[(size_t)ldl + kidx] = (double)((2LL * kp.y + 1) * P.lv[0].h) / (double)(2LL * L.h) + 0.5;
        if (aux) {
            aux[(size_t)kidx * 4 + 0] = (float)kept[L.plane0 + (size_t)kp.y * L.w + kp.x];
            aux[(size_t)kidx * 4 + 1] = (float)bin;
            aux[(size_t)kidx * 4 + 2] = (float)kp.level;
            aux[(size_t)kidx * 4 + 3] = 0.0f;
        }
    }
}

// ---- host: the plan and the chain ----------------------------------------------------------------------------------------
struct HostPlan {
    FastPlan dev;
    size_t plane_bytes, integ_elems;  // of all levels of one view
    unsigned int n_tiles, n_words;    // of all levels of all views
};

// Level 0 is the image; level l is level l - 1 divided by num / den, each side rounded half up.  The plan ends before the first level
// that has no pixel at least `margin` from every edge, or at n_levels.  nv views share it.
HostPlan make_plan(int h, int w, int n_levels, long long num, long long den, int nv = 1) {
    HostPlan hp;
    std::memset(&hp, 0, sizeof hp);
    const int least = 2 * host_pattern().margin + 1;
    for (int l = 0; l < n_levels; ++l) {
        if (l) {
            h = (int)((2 * h * den + num) / (2 * num));
            w = (int)((2 * w * den + num) / (2 * num));
            if (std::min(h, w) < least) break;
        }
        FastLevel& L = hp.dev.lv[l];
        L.h = h;
        L.w = w;
        L.wpr = (int)cdiv(w, 64);
        L.tile0 = hp.n_tiles;
        L.word0 = hp.n_words;
        L.plane0 = (long long)hp.plane_bytes;
        L.integ0 = (long long)hp.integ_elems;
        hp.n_tiles += (unsigned int)L.wpr * cdiv(h, kTH);
        hp.n_words += (unsigned int)L.wpr * (unsigned int)h;
        hp.plane_bytes += (size_t)h * w;
        hp.integ_elems += (size_t)(h + 1) * (w + 1);
        hp.dev.n = l + 1;
    }
    hp.dev.nv = nv;
    hp.dev.view_tiles = hp.n_tiles;
    hp.dev.view_words = hp.n_words;
    hp.dev.view_plane = (long long)hp.plane_bytes;
    hp.dev.view_integ = (long long)hp.integ_elems;
    hp.n_tiles *= (unsigned int)nv;
    hp.n_words *= (unsigned int)nv;
    return hp;
}

// the checks of the FAST entries on their group of views (the single-view entries: a group of one), which come before any device work
void check_args(const aps_fast_view* views, int nv, int height, int width, int channels, int img_layout, const aps_fast_params& prm,
                int desc_layout) {
    APS_REQUIRE(views, APS_E_ARG, "NULL argument");
    APS_REQUIRE(nv >= 1 && nv <= kGroupViews, APS_E_ARG, "n_views must be in 1..%d", kGroupViews);
    for (int v = 0; v < nv; ++v) APS_REQUIRE(views[v].img, APS_E_ARG, "NULL argument");
    APS_REQUIRE(height > 0 && width > 0, APS_E_DIM, "empty image");
    APS_REQUIRE(channels == 1 || channels == 3, APS_E_DIM, "channels must be 1 or 3");
    APS_REQUIRE(img_layout == APS_IMG_U8_HWC || img_layout == APS_IMG_U8_MATLAB, APS_E_TYPE, "unknown image layout");
    APS_REQUIRE(desc_layout == APS_ROWMAJOR || desc_layout == APS_COLMAJOR, APS_E_TYPE, "unknown descriptor layout");
    APS_REQUIRE(prm.threshold >= 0 && prm.threshold <= 255, APS_E_ARG, "threshold (floor(MinContrast * 255)) must be in 0..255");
    APS_REQUIRE(prm.quality_den > 0 && prm.quality_den <= (1 << 24) && prm.quality_num >= 0 && prm.quality_num <= prm.quality_den, APS_E_ARG,
                "MinQuality must be a rational in [0, 1] with a denominator of at most 2^24");
    for (int v = 0; v < nv; ++v) APS_REQUIRE(views[v].cap >= 0 && views[v].cap < (int64_t)1 << 31, APS_E_ARG, "capacity out of range");
    // the integral image holds exact 32-bit sums: the whole image at full brightness has to fit
    APS_REQUIRE(integral_fits(height, width), APS_E_ARG,
                "FAST: %d x %d pixels exceed the 32-bit integral image (height * width * 255 must stay below 2^32)", height, width);
}

void check_pyramid(int n_levels, int scale_num, int scale_den) {
    APS_REQUIRE(n_levels >= 1 && n_levels <= kMaxLevels, APS_E_ARG, "n_levels (NumLevels) must be in 1..%d", kMaxLevels);
    APS_REQUIRE(scale_den > 0 && scale_num > scale_den && (long long)scale_num <= 2LL * scale_den, APS_E_ARG,
                "ScaleFactor = scale_num / scale_den must lie in (1, 2]");
}

// The planes and integral images of all levels of all views, in the order of their dependences, on the calling thread's stream: one
// chain of launches whatever the number of views.  imgs: the views' images on the device; T: scratch of nv level-0 planes;
// I: nv * hp.integ_elems; planes: nv * hp.plane_bytes.
void build_levels(const ViewImgs& imgs, int channels, int img_layout, const HostPlan& hp, uint8_t* planes, uint32_t* T, uint32_t* I) {
    const int nv = hp.dev.nv;
    const size_t t_pitch = (size_t)hp.dev.lv[0].h * hp.dev.lv[0].w;
    for (int l = 0; l < hp.dev.n; ++l) {
        const FastLevel& L = hp.dev.lv[l];
        if (l) {
            const FastLevel& S = hp.dev.lv[l - 1];
            Prof prof("fast_resample");
            fast_resample_kernel<<<dim3(cdiv(L.w, kRW), cdiv(L.h, kRH), nv), 256, 0, stream()>>>(planes + S.plane0, S.h, S.w, planes + L.plane0, L.h,
                                                                                              L.w, hp.dev.view_plane);
            check_launch("fast_resample_kernel");
        }
        Prof prof("fast_integral");
        if (l == 0) {
            integral_image(imgs, nv, L.h, L.w, channels, img_layout, T, t_pitch, I, hp.integ_elems, planes, hp.plane_bytes);
        } else {
            ViewImgs lv;
            std::memset(&lv, 0, sizeof lv);
            for (int v = 0; v < nv; ++v) lv.p[v] = planes + v * hp.plane_bytes + L.plane0;
            integral_image(lv, nv, L.h, L.w, 1, APS_IMG_U8_HWC, T, t_pitch, I + L.integ0, hp.integ_elems, nullptr, 0);
        }
    }
}

// the views' images on the device, staged where they live on the host
struct StagedImgs {
    std::vector<In<uint8_t>> dimg;
    ViewImgs imgs;
    StagedImgs(const aps_fast_view* views, int nv, size_t bytes) : dimg(nv) {
        std::memset(&imgs, 0, sizeof imgs);
        for (int v = 0; v < nv; ++v) {
            dimg[v].bind(views[v].img, bytes);
            imgs.p[v] = dimg[v];
        }
    }
};

// What the chain holds once the candidates are known: the levels, the plane of kept scores, the candidate bitmap (bit order = the
// views one after the other, each in canonical order) and the exclusive scan of its popcounts; prefix[v * view_words] is the first
// candidate of view v, prefix[n_words] the number of all.
struct FastFront {
    Ws<uint32_t> T, I;
    Ws<uint8_t> planes, kept;
    Ws<unsigned int> smax, prefix;
    Ws<unsigned long long> bitmap;
    // a Harris front holds the int64 plane of candidate responses and the levels' maxima in the place of kept and smax
    Ws<long long> cand;
    Ws<unsigned long long> rmax;
    const unsigned int* d_total() const { return prefix.get() + prefix.n - 1; }
    // the u8 plane the describers read aux[0] from: a Harris front has no score plane, its rows' aux[0] is written after the
    // description (harris_aux), so there the describers read a byte of the level planes, which are of the same size
    const uint8_t* scores() const { return cand.get() ? planes.get() : kept.get(); }
};

// levels, detection, gate and scan of the group on the calling thread's stream; no read-back
void fast_front(const aps_fast_view* views, int channels, int img_layout, const aps_fast_params* params, const HostPlan& hp, FastFront& F,
                int corner = APS_CORNER_FAST) {
    const FastPlan& P = hp.dev;
    const int H = P.lv[0].h, W = P.lv[0].w, margin = host_pattern().margin, nv = P.nv;
    const size_t n_words = hp.n_words;
    StagedImgs staged(views, nv, (size_t)H * W * channels);
    F.T.alloc((size_t)nv * H * W);
    F.I.alloc(nv * hp.integ_elems);
    F.planes.alloc(nv * hp.plane_bytes);
    build_levels(staged.imgs, channels, img_layout, hp, F.planes, F.T, F.I);
    F.bitmap.alloc(n_words + 1);  // (+1: a zero word, whose prefix is the total)
    F.prefix.alloc(n_words + 1);
    APS_HIP(hipMemsetAsync(F.bitmap.get() + n_words, 0, sizeof(unsigned long long), stream()));
    if (corner == APS_CORNER_HARRIS) {
        static_assert(kFreakMargin >= kHarrisHalo, "the neighbours of a band pixel have their whole patch inside the plane");
        APS_REQUIRE(margin >= kHarrisHalo, APS_E_INTERNAL, "margin %d", margin);
        F.cand.alloc(nv * hp.plane_bytes);
        F.rmax.alloc((size_t)nv * P.n);
        {
            Prof prof("harris_detect");
            APS_HIP(hipMemsetAsync(F.rmax.get(), 0, (size_t)nv * P.n * sizeof(unsigned long long), stream()));
            harris_detect_kernel<false><<<hp.n_tiles, 256, 0, stream()>>>(F.planes, P, margin, F.cand, F.rmax);
            check_launch("harris_detect_kernel");
            harris_gate_kernel<<<cdiv(n_words, 4), 256, 0, stream()>>>(F.cand, P, hp.n_words, F.rmax, (unsigned int)params->quality_num,
                                                                       (unsigned int)params->quality_den, F.bitmap);
            check_launch("harris_gate_kernel");
        }
        Prof prof("fast_scan");
        exclusive_scan(popcounts(F.bitmap.get()), F.prefix.get(), 0u, n_words + 1);
        return;
    }
    F.kept.alloc(nv * hp.plane_bytes);
    F.smax.alloc((size_t)nv * P.n);
    const Ws<uint8_t>&planes = F.planes, &kept = F.kept;
    const Ws<unsigned int>&smax = F.smax, &prefix = F.prefix;
    const Ws<unsigned long long>& bitmap = F.bitmap;
    {
        Prof prof("fast_detect");
        fast_detect_kernel<<<hp.n_tiles, 256, 0, stream()>>>(planes, P, params->threshold, margin, kept);
        check_launch("fast_detect_kernel");
        APS_HIP(hipMemsetAsync(smax.get(), 0, (size_t)nv * P.n * sizeof(unsigned int), stream()));
        fast_smax_kernel<<<dim3(cdiv(hp.plane_bytes, (size_t)kSmaxChunk), nv), 256, 0, stream()>>>(kept, P, smax);
        check_launch("fast_smax_kernel");
        fast_gate_kernel<<<cdiv(n_words, 4), 256, 0, stream()>>>(kept, P, hp.n_words, smax, (unsigned int)params->quality_num,
                                                                 (unsigned int)params->quality_den, bitmap);
        check_launch("fast_gate_kernel");
    }
    {
        Prof prof("fast_scan");
        exclusive_scan(popcounts(bitmap.get()), prefix.get(), 0u, n_words + 1);
    }
}

// the rows of the views in `kps` (view v's at its record's kp0) -> every view's desc, loc and aux: one launch, the view in the grid
void freak_describe(const HostPlan& hp, const FastFront& F, const Keypoint* kps, GroupOut<uint8_t, aps_fast_view>& out, unsigned int most) {
    Ws<FreakDev> d_tb(1);
    Prof prof("freak_keypoint");  // (with the upload of the pattern tables)
    APS_HIP(hipMemcpyAsync(d_tb, &dev_pattern(), sizeof(FreakDev), hipMemcpyHostToDevice, stream()));
    freak_keypoint_kernel<<<dim3(cdiv(most, 4), out.nv), 256, 0, stream()>>>(F.I, hp.dev, d_tb, F.scores(), kps, out.d_rows, out.desc_layout,
                                                                            (long long)out.ldd, (long long)out.ldl);
    check_launch("freak_keypoint_kernel");
}

// the same for ORB: the level planes in the integral images' place
void orb_describe(const HostPlan& hp, const FastFront& F, const Keypoint* kps, GroupOut<uint8_t, aps_fast_view>& out, unsigned int most) {
    APS_REQUIRE(host_pattern().margin >= kFreakMargin && orb_tables().reach == kOrbReach, APS_E_INTERNAL, "ORB tables reach %d pixels, margin %d",
                orb_tables().reach, host_pattern().margin);
    Ws<OrbDev> d_tb(1);
    Prof prof("orb_keypoint");  // (with the upload of the pattern tables)
    APS_HIP(hipMemcpyAsync(d_tb, &orb_tables().dev, sizeof(OrbDev), hipMemcpyHostToDevice, stream()));
    orb_keypoint_kernel<<<dim3(cdiv(most, 4), out.nv), 256, 0, stream()>>>(F.planes, hp.dev, d_tb, F.scores(), kps, out.d_rows, out.desc_layout,
                                                                          (long long)out.ldd, (long long)out.ldl);
    check_launch("orb_keypoint_kernel");
}

// what a chain knows about its descriptor: the bytes of a row and the launch that writes the rows
struct Describer {
    size_t width;
    void (*describe)(const HostPlan&, const FastFront&, const Keypoint*, GroupOut<uint8_t, aps_fast_view>&, unsigned int);
};
constexpr Describer kFreak = {64, freak_describe}, kOrb = {kOrbBytes, orb_describe};

// aux[0] of the rows a Harris chain has described (the describers leave a byte of the level planes there): f32(R)
void harris_aux(const HostPlan& hp, const FastFront& F, const Keypoint* kps, GroupOut<uint8_t, aps_fast_view>& out, unsigned int most) {
    harris_aux_kernel<<<dim3(cdiv(most, 256), out.nv), 256, 0, stream()>>>(F.cand, hp.dev, kps, out.d_rows);
    check_launch("harris_aux_kernel");
}

// aps_fast_extract, aps_fast_extract_pyramid, aps_fast_extract_batch and the ORB entries without a selection behind their argument
// checks (check_args, check_pyramid), on the plan's group of views.  One read-back: the views' counts.
void fast_chain(aps_fast_view* views, int channels, int img_layout, const aps_fast_params* params, const HostPlan& hp, int desc_layout,
                int64_t ldd, int64_t ldl, const Describer& D = kFreak, int corner = APS_CORNER_FAST) {
    ctx();
    const FastPlan& P = hp.dev;
    const int H = P.lv[0].h, W = P.lv[0].w, margin = host_pattern().margin, nv = P.nv;
    for (int v = 0; v < nv; ++v) views[v].count = 0;
    unsigned int room[kGroupViews], n[kGroupViews];
    check_views(views, nv, D.width, desc_layout, ldd, ldl, room);
    if (H < 2 * margin + 1 || W < 2 * margin + 1) return;  // no pixel is far enough from the edge: no features, no error
    FastFront F;
    fast_front(views, channels, img_layout, params, hp, F, corner);
    GroupOut<uint8_t, aps_fast_view> out(views, nv, room, D.width, D.width, desc_layout, ldd, ldl, nullptr, nullptr);
    ViewLimits lim = {};
    size_t kcap = 0;
    for (int v = 0; v < nv; ++v) kcap += lim.cap[v] = room[v];
    lim.max_features = params->max_features;
    Ws<unsigned int> d_n(nv);
    group_rows_kernel<uint8_t><<<1, 64, 0, stream()>>>(F.prefix, (long long)P.view_words, nv, lim, out.d_rows, d_n);
    check_launch("group_rows_kernel");
    if (kcap) {  // (views that fit have at most kcap keypoints between them; when one does not fit, no row is written)
        Ws<Keypoint> kps(kcap);
        {
            Prof prof("fast_emit");
            fast_emit_kernel<<<cdiv(hp.n_words, 256), 256, 0, stream()>>>(F.bitmap, F.prefix, P, hp.n_words, kps,
                                                                          (unsigned int)std::min<size_t>(kcap, 0xffffffffu));
            check_launch("fast_emit_kernel");
        }
        D.describe(hp, F, kps, out, *std::max_element(room, room + nv));
        if (corner == APS_CORNER_HARRIS) harris_aux(hp, F, kps, out, *std::max_element(room, room + nv));
    }
    read_back(d_n.get(), n, nv);  // the one read-back of the chain
    settle_counts(views, nv, n, n, params->max_features, corner == APS_CORNER_HARRIS ? "Harris" : "FAST");
    out.commit(n);
}

// the single-view entries: a group of one, *count from the view whether the chain returns or fails
template <class Chain>
void fast_single(const uint8_t* img, uint8_t* desc, double* loc, float* aux, int64_t cap, int64_t* count, Chain&& chain) {
    aps_fast_view view = {img, desc, loc, aux, cap, *count};
    try {
        chain(&view);
    } catch (...) {
        *count = view.count;
        throw;
    }
    *count = view.count;
}

// ---- strongest-N on the host -----------------------------------------------------------------------------------------------
// q_l = floor(N weight_l / W), weight_l = h_l + w_l; the remainder r < L goes one each to levels 0 .. r - 1
void strongest_quota(const FastPlan& P, long long N, long long* q) {
    long long W = 0, given = 0;
    for (int l = 0; l < P.n; ++l) W += P.lv[l].h + P.lv[l].w;
    for (int l = 0; l < P.n; ++l) given += q[l] = N * (P.lv[l].h + P.lv[l].w) / W;
    for (int l = 0; l < N - given; ++l) ++q[l];
}

// The candidate list of a call (fast_front's bitmap, emitted in canonical order), the response of every candidate and its sort key.
struct Candidates {
    unsigned int M = 0, first[kMaxLevels + 1] = {};  // level l holds candidates first[l] .. first[l + 1] - 1
    Ws<Keypoint> kps;
    Ws<long long> resp;
    Ws<unsigned long long> keys;
    Ws<unsigned int> vals;
};

// Reads the counts per level back (the first read-back of the strongest-N chain): the grids and the sort below are sized by M.
void harris_candidates(const HostPlan& hp, const FastFront& F, Candidates& Cd) {
    const FastPlan& P = hp.dev;
    Ws<unsigned int> d_first((size_t)kMaxLevels + 1);
    strongest_counts_kernel<<<1, 64, 0, stream()>>>(F.prefix, P, hp.n_words, d_first);
    check_launch("strongest_counts_kernel");
    read_back(d_first.get(), Cd.first, P.n + 1);
    const unsigned int M = Cd.M = Cd.first[P.n];
    if (!M) return;
    Cd.kps.alloc(M);
    Cd.resp.alloc(M);
    Cd.keys.alloc(M);
    Cd.vals.alloc(M);
    {
        Prof prof("fast_emit");
        fast_emit_kernel<<<cdiv(hp.n_words, 256), 256, 0, stream()>>>(F.bitmap, F.prefix, P, hp.n_words, Cd.kps, M);
        check_launch("fast_emit_kernel");
    }
    Prof prof("fast_harris");
    fast_harris_kernel<<<cdiv(M, 4), 256, 0, stream()>>>(F.planes, P, Cd.kps, M, Cd.resp, Cd.keys, Cd.vals);
    check_launch("fast_harris_kernel");
}

// aps_fast_extract_strongest and, with grid_rows > 0, aps_fast_extract_uniform (each level's k_l spread over the cells of its plane)
// behind their argument checks.  Two read-backs: the counts per level (harris_candidates), then the final count.
void strongest_chain(const uint8_t* img, int channels, int img_layout, const aps_fast_params* params, const HostPlan& hp, long long N,
                     int grid_rows, int grid_cols, uint8_t* desc, int desc_layout, int64_t ldd, double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count,
                     const Describer& D = kFreak, int corner = APS_CORNER_FAST) {
    ctx();
    *count = 0;
    const FastPlan& P = hp.dev;
    const int H = P.lv[0].h, W = P.lv[0].w, margin = host_pattern().margin;
    if (H < 2 * margin + 1 || W < 2 * margin + 1) return;  // no pixel is far enough from the edge: no features, no error
    aps_fast_view view = {img, desc, loc, aux, cap, 0};  // (the chain's kernels take a group: this is a group of one)
    FastFront F;
    fast_front(&view, channels, img_layout, params, hp, F, corner);
    Candidates Cd;
    harris_candidates(hp, F, Cd);
    const unsigned int M = Cd.M;
    // k_l: everything, or the quotas with the carry from the coarsest level down (host arithmetic on the counts read back)
    StrongestCut cut;
    unsigned int K = 0;
    {
        long long q[kMaxLevels] = {}, c = 0;
        strongest_quota(P, N, q);
        for (int l = kMaxLevels - 1; l >= 0; --l) {
            const long long Ml = l < P.n ? Cd.first[l + 1] - Cd.first[l] : 0;
            const long long kl = l >= P.n ? 0 : (long long)M <= N ? Ml : std::min(Ml, q[l] + c);
            if (l < P.n) c = q[l] + c - kl;
            cut.start[l] = l < P.n ? Cd.first[l] : M;
            cut.keep[l] = (unsigned int)kl;
            K += (unsigned int)kl;
        }
    }
    *count = K;
    if (params->max_features > 0 && K > (unsigned int)params->max_features)
        fail(APS_E_CAP, "%s kept %u features, more than params.max_features = %d", corner == APS_CORNER_HARRIS ? "Harris" : "FAST", K,
             params->max_features);
    if ((int64_t)K > cap) fail(APS_E_CAP, "feature capacity %lld < %u features", (long long)cap, K);
    if (K == 0) return;
    APS_REQUIRE(desc && loc, APS_E_ARG, "NULL output with features present");
    if (desc_layout == APS_ROWMAJOR)
        APS_REQUIRE(ldd >= (int64_t)D.width, APS_E_DIM, "ldd < %d", (int)D.width);
    else
        APS_REQUIRE(ldd >= cap, APS_E_DIM, "ldd < cap");
    APS_REQUIRE(ldl >= cap, APS_E_DIM, "ldl < cap");
    // the kept keypoints, in canonical order, and their responses
    Ws<Keypoint> sel_kps;
    Ws<long long> sel_resp;
    Ws<unsigned long long> words;
    Ws<unsigned int> prefix;
    const Keypoint* kps = Cd.kps;
    const long long* kresp = Cd.resp;
    const unsigned int* d_total = F.d_total();
    if (K < M) {
        Prof prof("fast_select");
        unsigned int n_words = 0;
        if (grid_rows > 0) {  // uniform-N: a stable sort by (level, -R), then one by segment; the budgets are the k_l
            Ws<unsigned int> segs(M);
            fast_segment_kernel<<<cdiv(M, 256), 256, 0, stream()>>>(Cd.kps, P, M, grid_rows, grid_cols, segs);
            check_launch("fast_segment_kernel");
            UniformBudget budget;
            for (int l = 0; l < kMaxLevels; ++l) budget.q[l] = cut.keep[l];
            select_uniform(Cd.keys, segs, Cd.vals, M, (unsigned int)P.n, (unsigned int)(grid_rows * grid_cols), budget, words, prefix, n_words);
        } else {
            select_by_key(Cd.keys, Cd.vals, M, cut, words, prefix, n_words);
        }
        sel_kps.alloc(K);
        sel_resp.alloc(K);
        strongest_compact_kernel<<<cdiv(n_words, 256), 256, 0, stream()>>>(words, prefix, n_words, Cd.kps, Cd.resp, sel_kps, sel_resp, K);
        check_launch("strongest_compact_kernel");
        kps = sel_kps;
        kresp = sel_resp;
        d_total = prefix.get() + n_words;
    }
    const unsigned int first = 0;
    GroupOut<uint8_t, aps_fast_view> out(&view, 1, &K, D.width, D.width, desc_layout, ldd, ldl, &first, &K);
    D.describe(hp, F, kps, out, K);
    if (corner == APS_CORNER_HARRIS) harris_aux(hp, F, kps, out, K);
    if (out.aux[0].present()) {
        strongest_aux_kernel<<<cdiv(K, 256), 256, 0, stream()>>>(kresp, K, out.aux[0]);
        check_launch("strongest_aux_kernel");
    }
    const unsigned int n = read_back(d_total);  // the second read-back: the count the device kept is the count the host worked out
    APS_REQUIRE(n == K, APS_E_INTERNAL, "strongest-N kept %u rows on the device, %u on the host", n, K);
    out.commit(&K);
}

// aps_fast_orb_extract and aps_corner_extract behind their NULL checks: the checks of the selection and of the FAST entries, then
// the chain of `select` with the describer and the corner detector
void select_entry(const uint8_t* img, int height, int width, int channels, int img_layout, const aps_fast_orb_params* params,
                         const Describer& D, int corner, uint8_t* desc, int desc_layout, int64_t ldd, double* loc, int64_t ldl, float* aux,
                         int64_t cap, int64_t* count) {
    const aps_fast_pyramid_params& pyr = params->pyramid;
    APS_REQUIRE(params->select >= 0 && params->select <= 2, APS_E_ARG, "select must be 0 (none), 1 (strongest-N) or 2 (uniform-N)");
    if (params->select == 1) APS_REQUIRE(params->n_select >= 1, APS_E_ARG, "n_select (NumStrongest) must be at least 1");
    if (params->select == 2) check_uniform(params->n_select, params->grid_rows, params->grid_cols);
    if (params->select == 0) {
        fast_single(img, desc, loc, aux, cap, count, [&](aps_fast_view* view) {
            check_args(view, 1, height, width, channels, img_layout, pyr.fast, desc_layout);
            check_pyramid(pyr.n_levels, pyr.scale_num, pyr.scale_den);
            fast_chain(view, channels, img_layout, &pyr.fast, make_plan(height, width, pyr.n_levels, pyr.scale_num, pyr.scale_den), desc_layout,
                       ldd, ldl, D, corner);
        });
        return;
    }
    const aps_fast_view view = {img, desc, loc, aux, cap, 0};
    check_args(&view, 1, height, width, channels, img_layout, pyr.fast, desc_layout);
    check_pyramid(pyr.n_levels, pyr.scale_num, pyr.scale_den);
    const bool grid = params->select == 2;
    strongest_chain(img, channels, img_layout, &pyr.fast, make_plan(height, width, pyr.n_levels, pyr.scale_num, pyr.scale_den), params->n_select,
                    grid ? params->grid_rows : 0, grid ? params->grid_cols : 0, desc, desc_layout, ldd, loc, ldl, aux, cap, count, D, corner);
}

// the describer of an APS_DESC_* value (the corner entries check the range first)
const Describer& describer_of(int descriptor) { return descriptor == APS_DESC_ORB ? kOrb : kFreak; }
void check_corner(const aps_corner_params* params) {
    APS_REQUIRE(params, APS_E_ARG, "NULL argument");
    APS_REQUIRE(params->corner == APS_CORNER_FAST || params->corner == APS_CORNER_HARRIS, APS_E_ARG, "corner must be APS_CORNER_FAST or APS_CORNER_HARRIS");
    APS_REQUIRE(params->descriptor == APS_DESC_FREAK || params->descriptor == APS_DESC_ORB, APS_E_ARG, "descriptor must be APS_DESC_FREAK or APS_DESC_ORB");
}

}  // namespace
}  // namespace aps

using namespace aps;

extern "C" {

int aps_freak_pattern(int32_t* fields, int32_t* pairs, int32_t* ori_pairs, int32_t* ori_dir, int32_t* cos_sin, int* margin) {
    return guarded([&] {
        const FreakHost& p = host_pattern();
        if (fields) std::memcpy(fields, p.fields, sizeof p.fields);
        if (pairs) std::memcpy(pairs, p.pairs, sizeof p.pairs);
        if (ori_pairs) std::memcpy(ori_pairs, p.ori_pairs, sizeof p.ori_pairs);
        if (ori_dir) std::memcpy(ori_dir, p.ori_dir, sizeof p.ori_dir);
        if (cos_sin) std::memcpy(cos_sin, p.cos_sin, sizeof p.cos_sin);
        if (margin) *margin = p.margin;
    });
}

int aps_fast_extract(const uint8_t* img, int height, int width, int channels, int img_layout,
                     const aps_fast_params* params, uint8_t* desc, int desc_layout, int64_t ldd,
                     double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(params && count, APS_E_ARG, "NULL argument");
        fast_single(img, desc, loc, aux, cap, count, [&](aps_fast_view* view) {
            check_args(view, 1, height, width, channels, img_layout, *params, desc_layout);
            fast_chain(view, channels, img_layout, params, make_plan(height, width, 1, 1, 1), desc_layout, ldd, ldl);
        });
    });
}

int aps_fast_extract_pyramid(const uint8_t* img, int height, int width, int channels, int img_layout,
                             const aps_fast_pyramid_params* params, uint8_t* desc, int desc_layout, int64_t ldd,
                             double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(params && count, APS_E_ARG, "NULL argument");
        fast_single(img, desc, loc, aux, cap, count, [&](aps_fast_view* view) {
            check_args(view, 1, height, width, channels, img_layout, params->fast, desc_layout);
            check_pyramid(params->n_levels, params->scale_num, params->scale_den);
            fast_chain(view, channels, img_layout, &params->fast,
                       make_plan(height, width, params->n_levels, params->scale_num, params->scale_den), desc_layout, ldd, ldl);
        });
    });
}

int aps_fast_extract_batch(aps_fast_view* views, int n_views, int height, int width, int channels, int img_layout,
                           const aps_fast_pyramid_params* params, int desc_layout, int64_t ldd, int64_t ldl) {
    return guarded([&] {
        APS_REQUIRE(params, APS_E_ARG, "NULL argument");
        check_args(views, n_views, height, width, channels, img_layout, params->fast, desc_layout);
        check_pyramid(params->n_levels, params->scale_num, params->scale_den);
        fast_chain(views, channels, img_layout, &params->fast,
                   make_plan(height, width, params->n_levels, params->scale_num, params->scale_den, n_views), desc_layout, ldd, ldl);
    });
}

int aps_fast_orb_extract(const uint8_t* img, int height, int width, int channels, int img_layout, const aps_fast_orb_params* params,
                         uint8_t* desc, int desc_layout, int64_t ldd, double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(params && count, APS_E_ARG, "NULL argument");
        select_entry(img, height, width, channels, img_layout, params, kOrb, APS_CORNER_FAST, desc, desc_layout, ldd, loc, ldl, aux, cap, count);
    });
}

int aps_corner_extract(const uint8_t* img, int height, int width, int channels, int img_layout, const aps_corner_params* params,
                       uint8_t* desc, int desc_layout, int64_t ldd, double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(count, APS_E_ARG, "NULL argument");
        check_corner(params);
        select_entry(img, height, width, channels, img_layout, &params->chain, describer_of(params->descriptor), params->corner, desc, desc_layout,
                     ldd, loc, ldl, aux, cap, count);
    });
}

int aps_corner_extract_batch(aps_fast_view* views, int n_views, int height, int width, int channels, int img_layout,
                             const aps_corner_params* params, int desc_layout, int64_t ldd, int64_t ldl) {
    return guarded([&] {
        check_corner(params);
        APS_REQUIRE(params->chain.select == 0, APS_E_ARG, "the group form has no selection: select must be 0");
        const aps_fast_pyramid_params& pyr = params->chain.pyramid;
        check_args(views, n_views, height, width, channels, img_layout, pyr.fast, desc_layout);
        check_pyramid(pyr.n_levels, pyr.scale_num, pyr.scale_den);
        fast_chain(views, channels, img_layout, &pyr.fast, make_plan(height, width, pyr.n_levels, pyr.scale_num, pyr.scale_den, n_views), desc_layout,
                   ldd, ldl, describer_of(params->descriptor), params->corner);
    });
}

int aps_harris_planes(const uint8_t* img, int height, int width, int channels, int img_layout, const aps_fast_pyramid_params* params,
                      int64_t* out, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(params && count, APS_E_ARG, "NULL argument");
        const aps_fast_view view = {img, nullptr, nullptr, nullptr, 0, 0};
        check_args(&view, 1, height, width, channels, img_layout, params->fast, APS_ROWMAJOR);
        check_pyramid(params->n_levels, params->scale_num, params->scale_den);
        const HostPlan hp = make_plan(height, width, params->n_levels, params->scale_num, params->scale_den);
        *count = (int64_t)hp.plane_bytes;  // one response per pixel of every level
        if (!out) return;                  // (the size alone: no device work)
        APS_REQUIRE(cap >= *count, APS_E_CAP, "response capacity %lld < %lld pixels", (long long)cap, (long long)*count);
        ctx();
        StagedImgs staged(&view, 1, (size_t)height * width * channels);
        Ws<uint32_t> T((size_t)height * width), I(hp.integ_elems);
        Ws<uint8_t> planes(hp.plane_bytes);
        static_assert(sizeof(long long) == sizeof(int64_t), "responses are stored as 64-bit integers");
        Out<long long> resp(reinterpret_cast<long long*>(out), hp.plane_bytes);
        build_levels(staged.imgs, channels, img_layout, hp, planes, T, I);
        harris_detect_kernel<true><<<hp.n_tiles, 256, 0, stream()>>>(planes, hp.dev, 0, resp, nullptr);
        check_launch("harris_detect_kernel");
        resp.commit();
        APS_HIP(hipStreamSynchronize(stream()));
    });
}

int aps_fast_orb_extract_batch(aps_fast_view* views, int n_views, int height, int width, int channels, int img_layout,
                               const aps_fast_pyramid_params* params, int desc_layout, int64_t ldd, int64_t ldl) {
    return guarded([&] {
        APS_REQUIRE(params, APS_E_ARG, "NULL argument");
        check_args(views, n_views, height, width, channels, img_layout, params->fast, desc_layout);
        check_pyramid(params->n_levels, params->scale_num, params->scale_den);
        fast_chain(views, channels, img_layout, &params->fast,
                   make_plan(height, width, params->n_levels, params->scale_num, params->scale_den, n_views), desc_layout, ldd, ldl, kOrb);
    });
}

int aps_orb_pattern(int32_t* tests, int32_t* table, int32_t* disc, int* reach) {
    return guarded([&] {
        const OrbTables& t = orb_tables();
        if (tests) std::memcpy(tests, t.tests, sizeof t.tests);
        for (int k = 0; table && k < kBins; ++k)
            for (int i = 0; i < kOrbTests; ++i) {
                const char4 e = t.dev.test[k & 63][i];
                int d[4] = {e.x, e.y, e.z, e.w};
                for (int q = 0; q < k >> 6; ++q)  // exact quarter turns (dx, dy) -> (-dy, dx)
                    for (int j = 0; j < 4; j += 2) {
                        const int dx = d[j];
                        d[j] = -d[j + 1];
                        d[j + 1] = dx;
                    }
                for (int j = 0; j < 4; ++j) table[((size_t)k * kOrbTests + i) * 4 + j] = d[j];
            }
        int n = 0;
        for (int v = -kOrbDiscR; disc && v <= kOrbDiscR; ++v)  // ascending (v, u)
            for (int u = -kOrbDiscR; u <= kOrbDiscR; ++u)
                if (u * u + v * v <= kOrbDiscR * kOrbDiscR) {
                    disc[2 * n] = u;
                    disc[2 * n + 1] = v;
                    ++n;
                }
        APS_REQUIRE(!disc || n == kOrbDisc, APS_E_INTERNAL, "the disc holds %d pixels", n);
        if (reach) *reach = t.reach;
    });
}

int aps_fast_pyramid_plan(int height, int width, int n_levels, int scale_num, int scale_den, int* heights, int* widths, int* n_used) {
    return guarded([&] {
        APS_REQUIRE(n_used, APS_E_ARG, "NULL argument");
        APS_REQUIRE(height > 0 && width > 0, APS_E_DIM, "empty image");
        check_pyramid(n_levels, scale_num, scale_den);
        const HostPlan hp = make_plan(height, width, n_levels, scale_num, scale_den);
        *n_used = hp.dev.n;
        for (int l = 0; l < hp.dev.n; ++l) {
            if (heights) heights[l] = hp.dev.lv[l].h;
            if (widths) widths[l] = hp.dev.lv[l].w;
        }
    });
}

int aps_fast_extract_strongest(const uint8_t* img, int height, int width, int channels, int img_layout,
                               const aps_fast_strongest_params* params, uint8_t* desc, int desc_layout, int64_t ldd,
                               double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(params && count, APS_E_ARG, "NULL argument");
        const aps_fast_pyramid_params& pyr = params->pyramid;
        APS_REQUIRE(params->n_strongest >= 1, APS_E_ARG, "n_strongest (NumStrongest) must be at least 1");
        const aps_fast_view view = {img, desc, loc, aux, cap, 0};
        check_args(&view, 1, height, width, channels, img_layout, pyr.fast, desc_layout);
        check_pyramid(pyr.n_levels, pyr.scale_num, pyr.scale_den);
        strongest_chain(img, channels, img_layout, &pyr.fast, make_plan(height, width, pyr.n_levels, pyr.scale_num, pyr.scale_den),
                        params->n_strongest, 0, 0, desc, desc_layout, ldd, loc, ldl, aux, cap, count);
    });
}

int aps_fast_extract_uniform(const uint8_t* img, int height, int width, int channels, int img_layout,
                             const aps_fast_uniform_params* params, uint8_t* desc, int desc_layout, int64_t ldd,
                             double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(params && count, APS_E_ARG, "NULL argument");
        const aps_fast_pyramid_params& pyr = params->strongest.pyramid;
        check_uniform(params->strongest.n_strongest, params->grid_rows, params->grid_cols);
        const aps_fast_view view = {img, desc, loc, aux, cap, 0};
        check_args(&view, 1, height, width, channels, img_layout, pyr.fast, desc_layout);
        check_pyramid(pyr.n_levels, pyr.scale_num, pyr.scale_den);
        strongest_chain(img, channels, img_layout, &pyr.fast, make_plan(height, width, pyr.n_levels, pyr.scale_num, pyr.scale_den),
                        params->strongest.n_strongest, params->grid_rows, params->grid_cols, desc, desc_layout, ldd, loc, ldl, aux, cap, count);
    });
}

int aps_fast_strongest_quota(int height, int width, int n_levels, int scale_num, int scale_den, int n_strongest, int* quota, int* n_used) {
    return guarded([&] {
        APS_REQUIRE(n_used, APS_E_ARG, "NULL argument");
        APS_REQUIRE(height > 0 && width > 0, APS_E_DIM, "empty image");
        APS_REQUIRE(n_strongest >= 1, APS_E_ARG, "n_strongest (NumStrongest) must be at least 1");
        check_pyramid(n_levels, scale_num, scale_den);
        const HostPlan hp = make_plan(height, width, n_levels, scale_num, scale_den);
        long long q[kMaxLevels] = {};
        strongest_quota(hp.dev, n_strongest, q);
        *n_used = hp.dev.n;
        for (int l = 0; quota && l < hp.dev.n; ++l) quota[l] = (int)q[l];
    });
}

int aps_fast_harris(const uint8_t* img, int height, int width, int channels, int img_layout, const aps_fast_pyramid_params* params,
                    int64_t* response, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(params && count, APS_E_ARG, "NULL argument");
        const aps_fast_view view = {img, nullptr, nullptr, nullptr, cap, 0};
        check_args(&view, 1, height, width, channels, img_layout, params->fast, APS_ROWMAJOR);
        check_pyramid(params->n_levels, params->scale_num, params->scale_den);
        const HostPlan hp = make_plan(height, width, params->n_levels, params->scale_num, params->scale_den);
        ctx();
        *count = 0;
        if (std::min(height, width) < 2 * host_pattern().margin + 1) return;
        FastFront F;
        fast_front(&view, channels, img_layout, &params->fast, hp, F);
        Candidates Cd;
        harris_candidates(hp, F, Cd);
        *count = Cd.M;
        if (!response || !Cd.M) {  // (the count alone)
            APS_HIP(hipStreamSynchronize(stream()));
            return;
        }
        APS_REQUIRE(cap >= (int64_t)Cd.M, APS_E_CAP, "response capacity %lld < %u candidates", (long long)cap, Cd.M);
        static_assert(sizeof(long long) == sizeof(int64_t), "responses are stored as 64-bit integers");
        APS_HIP(hipMemcpyAsync(response, Cd.resp.get(), (size_t)Cd.M * sizeof(int64_t),
                               is_device_ptr(response) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream()));
        APS_HIP(hipStreamSynchronize(stream()));
    });
}

int aps_fast_pyramid_planes(const uint8_t* img, int height, int width, int channels, int img_layout,
                            const aps_fast_pyramid_params* params, uint8_t* out, int64_t cap_bytes, int64_t* bytes) {
    return guarded([&] {
        APS_REQUIRE(params && bytes, APS_E_ARG, "NULL argument");
        const aps_fast_view view = {img, nullptr, nullptr, nullptr, 0, 0};
        check_args(&view, 1, height, width, channels, img_layout, params->fast, APS_ROWMAJOR);
        check_pyramid(params->n_levels, params->scale_num, params->scale_den);
        const HostPlan hp = make_plan(height, width, params->n_levels, params->scale_num, params->scale_den);
        *bytes = (int64_t)hp.plane_bytes;
        if (!out) return;  // (the size alone: no device work)
        APS_REQUIRE(cap_bytes >= *bytes, APS_E_CAP, "plane capacity %lld < %lld bytes", (long long)cap_bytes, (long long)*bytes);
        ctx();
        StagedImgs staged(&view, 1, (size_t)height * width * channels);
        Ws<uint32_t> T((size_t)height * width), I(hp.integ_elems);
        Out<uint8_t> planes(out, hp.plane_bytes);
        build_levels(staged.imgs, channels, img_layout, hp, planes, T, I);
        planes.commit();
        APS_HIP(hipStreamSynchronize(stream()));
    });
}

}  // extern "C"
