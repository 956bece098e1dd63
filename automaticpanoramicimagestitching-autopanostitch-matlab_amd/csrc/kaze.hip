// kaze.hip — KAZE detector + 64-D M-SURF descriptor on the gfx950.
// Stands behind PP/featureMatching/getFeaturePoints.m:63-64,71-74 (rgb2gray -> detectKAZEFeatures -> extractFeatures).  The toolbox
// functions are closed code; the algorithm is KAZE of Alcantarilla, Bartoli, Davison (ECCV 2012) restated in DESIGN.md "KAZE contract",
// which fixes every operation and summation order below so that a NumPy restatement (tests/kaze_mirror.py) reproduces the outputs
// bit for bit.  The rule is the SURF contract's: f32 chains with one rounding per written operation (-ffp-contract=off, IEEE / and
// sqrtf), every Gaussian, FED step size, level sigma and window direction from host tables (f64 -> f32), no device transcendental
// in any stored value or discrete decision (atan2f only feeds aux's angle_deg).  One border rule for every plane stencil: an index
// outside the plane is clamped to the nearest row / column; the tiles are loaded that way, so a stencil reads its tile unclamped.
//
// Every level is a full-resolution f32 plane.  Chain of one call (one host read-back: the final count; the contrast factor stays on
// the device):
//   kaze_gray_kernel        rgb2gray's integer plane (integral_dev.h: gray_at) * f32(1/255)
//   kaze_smooth_kernel<1>   sigma 1 blur -> 3x3 Scharr -> gradient magnitude plane and its maximum (integer atomicMax on the bits)
//   kaze_hist_kernel        300-bin histogram of the magnitudes (integer counts), kaze_contrast_kernel: the 70th percentile -> k, k^2
//   kaze_blur_kernel<7>     level 0 = sigma 1.6 blur of the input
//   per level i:
//     kaze_smooth_kernel<0> sigma 1 blur -> Ls; 3x3 Scharr of Ls -> conductivity c = 1 / (1 + |grad|^2 / k^2)   (one tile, one pass)
//     kaze_scharr_kernel<0> Ls -> Lx, Ly at step round(sigma_i): the level's stored derivative planes
//     kaze_scharr_kernel<1> Lx, Ly -> Lxx, Lxy, Lyy at the same step -> scale-normalised determinant: the level's response plane
//     kaze_fed_kernel       n_i explicit diffusion steps L <- L + tau_j/2 * div(c grad L), c fixed, between two ping-pong planes
//   kaze_detect_kernel      64 x 8 tile (+1 halo) of three response planes into LDS, threshold, strict 3x3x3 maximum, margin and the
//                           refinement's verdict; one ballot = one 64-bit word of the candidate bitmap, whose bit order IS the
//                           canonical feature order (level, row, col)
//   exclusive scan of the words' popcounts (rocprim), group_rows_kernel (group_dev.h: a group of one view), kaze_emit_kernel
//   kaze_keypoint_kernel    one wave per keypoint: the 27 responses again, refinement, orientation, descriptor, outputs
//
// aps_kaze_extract_select (DESIGN.md "KAZE selection and Upright") shares the chain up to the scan (kaze_front).  With a selection
// it reads the candidate count back, lists all candidates and continues with
//   kaze_key_kernel         the metric of every candidate as the selection's key, under its grid cell for uniform-N
//   select_int4_group       (surf.hip's copies of select_dev.h's kernels) stable radix sort, flags, ballot words, scan, water-filling
//                           for uniform-N, select_compact_kernel (canonical order again)
//   kaze_keypoint_kernel    on the kept candidates only
// and a second read-back, the count the device kept.  Upright is the keypoint kernel's second instantiation, without the
// orientation stage.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "aps_internal.h"
#include "group_dev.h"
#include "select_key.h"  // (the key's layout and the uniform entries' checks; the selection itself is surf.hip's select_int4_group)

namespace aps {
namespace {

constexpr int kMaxLevels = 40;     // 4 octaves x 10 sublevels
constexpr int kTW = 64, kTH = 16;  // tile of the plane kernels: 256 threads, 4 pixels each
constexpr int kDH = 8;             // rows of the detection tile: a wave's ballot covers one row of it
constexpr int kR0 = 7, kR1 = 4;    // radii of the sigma 1.6 and sigma 1 Gaussians: ceil(4 sigma)
constexpr int kBins = 300;         // histogram of the contrast factor
constexpr int kOriN = 109;         // disc samples of the orientation: integer (di, dj), di^2 + dj^2 < 36
constexpr int kWin = 64;           // positions of the pi/3 sliding window
constexpr int kGrid = 24;          // descriptor samples per side: u, v = -12 .. 11

struct GaussW {
    float w[8];  // w[k], k = 0 .. radius: exp(-k^2 / (2 sigma^2)) / sum, f64 -> f32
};

struct KazePlan {
    int n_levels, h, w, wpr;  // wpr: 64-bit bitmap words per row
    long long n_words;        // (n_levels - 2) * h * wpr
    size_t pitch;             // elements of one plane
    float sigma[kMaxLevels];  // 1.6 * 2^(i / S)
    int step[kMaxLevels];     // round(sigma_i): the derivative step
    int margin[kMaxLevels];   // ceil(5 sigma_{i+1}) + 2: detection, refinement and orientation stay inside the plane
    float inv[kMaxLevels];    // f32(1 / (32 step)): the Scharr normalisation
    float norm4[kMaxLevels];  // f32(sigma_i^4): the scale normalisation of the determinant
};

// host tables (f64 -> f32) of the keypoint kernel, uploaded with every call
struct KazeTables {
    float ori_g[kOriN];  // exp(-(di^2 + dj^2) / (2 * 2.5^2))
    int ori_di[kOriN], ori_dj[kOriN];
    float win_c[kWin], win_s[kWin];  // window directions; quarter turns are exact images of the first quadrant
    float g1[81];  // exp(-((a - 4)^2 + (b - 4)^2) / (2 * 2.5^2)): a sample (row a, column b) of a 9 x 9 sub-region about its centre
    float g2[16];  // exp(-((R - 1.5)^2 + (C - 1.5)^2) / (2 * 1.5^2)): sub-region (R, C) of the 4 x 4 grid
};

const KazeTables& host_tables() {
    static const KazeTables t = [] {
        KazeTables s;
        int n = 0;
        for (int di = -5; di <= 5; ++di)
            for (int dj = -5; dj <= 5; ++dj)
                if (di * di + dj * dj < 36) {
                    s.ori_di[n] = di;
                    s.ori_dj[n] = dj;
                    s.ori_g[n] = (float)std::exp(-(double)(di * di + dj * dj) / 12.5);
                    ++n;
                }
        for (int wi = 0; wi < kWin; ++wi) {
            const int q = wi / 16, r = wi % 16;
            float c = (float)std::cos(2.0 * M_PI * (double)r / 64.0), sn = (float)std::sin(2.0 * M_PI * (double)r / 64.0);
            for (int k = 0; k < q; ++k) {  // one exact quarter turn: (c, s) -> (-s, c)
                const float t2 = c;
                c = -sn;
                sn = t2;
            }
            s.win_c[wi] = c;
            s.win_s[wi] = sn;
        }
        for (int a = 0; a < 9; ++a)
            for (int b = 0; b < 9; ++b) s.g1[a * 9 + b] = (float)std::exp(-(double)((a - 4) * (a - 4) + (b - 4) * (b - 4)) / 12.5);
        for (int R = 0; R < 4; ++R)
            for (int C = 0; C < 4; ++C) {
                const double dr = (double)R - 1.5, dc = (double)C - 1.5;
                s.g2[R * 4 + C] = (float)std::exp(-(dr * dr + dc * dc) / 4.5);
            }
        return s;
    }();
    return t;
}

GaussW gauss_weights(double sigma, int radius) {
    double w[8], sum = 0.0;
    for (int k = 0; k <= radius; ++k) {
        w[k] = std::exp(-(double)(k * k) / (2.0 * sigma * sigma));
        sum += k == 0 ? w[k] : 2.0 * w[k];
    }
    GaussW g = {};
    for (int k = 0; k <= radius; ++k) g.w[k] = (float)(w[k] / sum);
    return g;
}

// One FED cycle of stopping time T with tau_max = 0.25 (Grewenig, Weickert, Bruhn 2010): n = ceil(sqrt(3 T / tau_max + 1/4) - 1/2)
// steps tau_j = 3 T / (2 (n^2 + n) cos^2(pi (2 j + 1) / (4 n + 2))), applied in the kappa-cycle order (kappa = n / 2 over the next
// prime above n) that keeps the cycle's rounding error small.  Returns f32(tau_j / 2) in the order of application.
std::vector<float> fed_half_taus(double T) {
    const double tau_max = 0.25;
    const int n = (int)(std::ceil(std::sqrt(3.0 * T / tau_max + 0.25) - 0.5 - 1.0e-8) + 0.5);
    std::vector<double> tau(n);
    const double scale = 3.0 * T / (tau_max * (double)(n * (n + 1))), c = 1.0 / (4.0 * (double)n + 2.0);
    for (int j = 0; j < n; ++j) {
        const double hc = std::cos(M_PI * (2.0 * (double)j + 1.0) * c);
        tau[j] = scale * tau_max / (2.0 * hc * hc);
    }
    const auto is_prime = [](int p) {
        for (int d = 2; d * d <= p; ++d)
            if (p % d == 0) return false;
        return p >= 2;
    };
    int prime = n + 1;
    while (!is_prime(prime)) ++prime;
    const int kappa = std::max(1, n / 2);
    std::vector<float> out(n);
    for (int k = 0, l = 0; l < n; ++k, ++l) {
        int index;
        while ((index = ((k + 1) * kappa) % prime - 1) >= n) ++k;
        out[l] = (float)(0.5 * tau[index]);
    }
    return out;
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// tile[r * ts + c] = P[clamp(y0 - halo + r)][clamp(x0 - halo + c)], r < rows, c < cols: the one border rule of the chain
__device__ __forceinline__ void load_tile(const float* __restrict__ P, int h, int w, int y0, int x0, int halo, float* tile, int rows, int cols,
                                          int ts) {
    for (int e = threadIdx.x; e < rows * cols; e += 256) {
        const int r = e / cols, c = e - r * cols;
        tile[r * ts + c] = P[(size_t)clampi(y0 - halo + r, h - 1) * w + clampi(x0 - halo + c, w - 1)];
    }
}

// the Scharr pair of a tile at step s about (r, c): differences first, so that a constant gives exact zeros, and the outer rows
// (columns) summed before the weights, so that a mirrored plane gives mirrored values
__device__ __forceinline__ float scharr_x(const float* t, int ts, int r, int c, int s, float inv) {
    const float da = t[(r - s) * ts + c + s] - t[(r - s) * ts + c - s];
    const float db = t[r * ts + c + s] - t[r * ts + c - s];
    const float dc = t[(r + s) * ts + c + s] - t[(r + s) * ts + c - s];
    return (3.0f * (da + dc) + 10.0f * db) * inv;
}
__device__ __forceinline__ float scharr_y(const float* t, int ts, int r, int c, int s, float inv) {
    const float ea = t[(r + s) * ts + c - s] - t[(r - s) * ts + c - s];
    const float eb = t[(r + s) * ts + c] - t[(r - s) * ts + c];
    const float ec = t[(r + s) * ts + c + s] - t[(r - s) * ts + c + s];
    return (3.0f * (ea + ec) + 10.0f * eb) * inv;
}

__global__ __launch_bounds__(256) void kaze_gray_kernel(const uint8_t* __restrict__ img, int h, int w, int c, int layout, float* __restrict__ P) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)h * w) return;
    const int y = (int)(i / w), x = (int)(i % w);
    P[i] = (float)gray_at(img, h, w, c, layout, y, x) * 0.00392156862745098f;  // f32(1/255)
}

// Separable Gaussian of radius R, rows first: acc = w0 x0, then acc = acc + wk (x[-k] + x[+k]) for k = 1 .. R.
template <int R>
__global__ __launch_bounds__(256) void kaze_blur_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w, GaussW g) {
    constexpr int kRows = kTH + 2 * R, kCols = kTW + 2 * R;
    __shared__ float s_in[kRows * (kCols + 1)];
    __shared__ float s_h[kRows * (kTW + 1)];
    const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    load_tile(in, h, w, y0, x0, R, s_in, kRows, kCols, kCols + 1);
    __syncthreads();
    for (int e = threadIdx.x; e < kRows * kTW; e += 256) {
        const int r = e / kTW, c = e % kTW;
        const float* p = s_in + r * (kCols + 1) + c + R;
        float acc = g.w[0] * p[0];
#pragma unroll
        for (int k = 1; k <= R; ++k) acc = acc + g.w[k] * (p[-k] + p[k]);
        s_h[r * (kTW + 1) + c] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kTH * kTW; e += 256) {
        const int r = e / kTW, c = e % kTW, y = y0 + r, x = x0 + c;
        if (y >= h || x >= w) continue;
        const float* p = s_h + (r + R) * (kTW + 1) + c;
        float acc = g.w[0] * p[0];
#pragma unroll
        for (int k = 1; k <= R; ++k) acc = acc + g.w[k] * (p[-k * (kTW + 1)] + p[k * (kTW + 1)]);
        out[(size_t)y * w + x] = acc;
    }
}

// One tile, one pass: sigma 1 blur of `in` (halo 4 + 1) -> Ls, then the 3 x 3 Scharr pair of Ls.
//   MODE 0  Ls is stored and out2 = 1 / (1 + (Lx^2 + Ly^2) / k^2), k^2 = stats[0]: the level's conductivity
//   MODE 1  out2 = sqrtf(Lx^2 + Ly^2) and *hmax = the largest of them (as the bits of a non-negative f32): the contrast factor's input
// The blurred tile holds garbage outside the plane; the Scharr pair reads it at clamped coordinates.
template <int MODE>
__global__ __launch_bounds__(256) void kaze_smooth_kernel(const float* __restrict__ in, float* __restrict__ Ls, float* __restrict__ out2, int h,
                                                          int w, GaussW g, const float* __restrict__ stats, unsigned int* __restrict__ hmax) {
    constexpr int kHalo = kR1 + 1, kRows = kTH + 2 * kHalo, kCols = kTW + 2 * kHalo, kSW = kTW + 2, kSH = kTH + 2;
    __shared__ float s_in[kRows * (kCols + 1)];
    __shared__ float s_h[kRows * (kSW + 1)];
    __shared__ float s_s[kSH * (kSW + 1)];
    __shared__ unsigned int s_max;
    const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    if (MODE == 1 && threadIdx.x == 0) s_max = 0u;
    load_tile(in, h, w, y0, x0, kHalo, s_in, kRows, kCols, kCols + 1);
    __syncthreads();
    for (int e = threadIdx.x; e < kRows * kSW; e += 256) {  // column c is x0 - 1 + c
        const int r = e / kSW, c = e % kSW;
        const float* p = s_in + r * (kCols + 1) + c + kR1;
        float acc = g.w[0] * p[0];
#pragma unroll
        for (int k = 1; k <= kR1; ++k) acc = acc + g.w[k] * (p[-k] + p[k]);
        s_h[r * (kSW + 1) + c] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kSH * kSW; e += 256) {  // row r is y0 - 1 + r
        const int r = e / kSW, c = e % kSW;
        const float* p = s_h + (r + kR1) * (kSW + 1) + c;
        float acc = g.w[0] * p[0];
#pragma unroll
        for (int k = 1; k <= kR1; ++k) acc = acc + g.w[k] * (p[-k * (kSW + 1)] + p[k * (kSW + 1)]);
        s_s[r * (kSW + 1) + c] = acc;
    }
    __syncthreads();
    const float k2 = MODE == 0 ? stats[0] : 1.0f;
    unsigned int top = 0u;
    for (int e = threadIdx.x; e < kTH * kTW; e += 256) {
        const int r = e / kTW, c = e % kTW, y = y0 + r, x = x0 + c;
        if (y >= h || x >= w) continue;
        constexpr int ts = kSW + 1;
        const int rm = clampi(y - 1, h - 1) - (y0 - 1), rc = r + 1, rp = clampi(y + 1, h - 1) - (y0 - 1);
        const int cm = clampi(x - 1, w - 1) - (x0 - 1), cc = c + 1, cp = clampi(x + 1, w - 1) - (x0 - 1);
        const float da = s_s[rm * ts + cp] - s_s[rm * ts + cm], db = s_s[rc * ts + cp] - s_s[rc * ts + cm], dc = s_s[rp * ts + cp] - s_s[rp * ts + cm];
        const float lx = (3.0f * (da + dc) + 10.0f * db) * 0.03125f;
        const float ea = s_s[rp * ts + cm] - s_s[rm * ts + cm], eb = s_s[rp * ts + cc] - s_s[rm * ts + cc], ec = s_s[rp * ts + cp] - s_s[rm * ts + cp];
        const float ly = (3.0f * (ea + ec) + 10.0f * eb) * 0.03125f;
        const float g2 = lx * lx + ly * ly;
        if (MODE == 0) {
            Ls[(size_t)y * w + x] = s_s[rc * ts + cc];
            out2[(size_t)y * w + x] = 1.0f / (1.0f + g2 / k2);
        } else {
            const float m = sqrtf(g2);
            out2[(size_t)y * w + x] = m;
            top = max(top, __float_as_uint(m));
        }
    }
    if (MODE == 1) {
        atomicMax(&s_max, top);
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(hmax, s_max);
    }
}

// hist[b] += the magnitudes m > 0 with b = min(299, int((m / hmax) * 300)): integer counts, exact in any order
__global__ __launch_bounds__(256) void kaze_hist_kernel(const float* __restrict__ mag, size_t n, const unsigned int* __restrict__ hmax,
                                                        unsigned int* __restrict__ hist) {
    __shared__ unsigned int s[kBins];
    for (int b = threadIdx.x; b < kBins; b += 256) s[b] = 0u;
    __syncthreads();
    const float top = __uint_as_float(*hmax);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float m = mag[i];
        if (m > 0.0f) {
            int b = (int)((m / top) * 300.0f);
            if (b > kBins - 1) b = kBins - 1;
            atomicAdd(&s[b], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kBins; b += 256)
        if (s[b]) atomicAdd(&hist[b], s[b]);
}

// The contrast factor: the bins are walked until they hold floor(0.7 * points) magnitudes; k = hmax * (bins walked / 300), or
// f32(0.03) when none is walked (a flat image).  stats = [k^2, k].
__global__ void kaze_contrast_kernel(const unsigned int* __restrict__ hmax, const unsigned int* __restrict__ hist, float* __restrict__ stats) {
    if (threadIdx.x || blockIdx.x) return;
    unsigned long long points = 0;
    for (int b = 0; b < kBins; ++b) points += hist[b];
    const unsigned long long want = points * 7ull / 10ull;
    unsigned long long seen = 0;
    int k = 0;
    for (; seen < want && k < kBins; ++k) seen += hist[k];
    float kc = 0.03f;
    if (k > 0) kc = __uint_as_float(*hmax) * ((float)k / 300.0f);
    stats[0] = kc * kc;
    stats[1] = kc;
}

// The Scharr pair at step s on tiles with halo s (dynamic LDS: (kTH + 2 s) x (kTW + 2 s + 1) floats per tile).
//   MODE 0  in0 = Ls -> o0 = Lx, o1 = Ly
//   MODE 1  in0 = Lx, in1 = Ly -> o0 = (Lxx * Lyy - Lxy * Lxy) * norm4 with Lxx = d/dx Lx, Lxy = d/dy Lx, Lyy = d/dy Ly
template <int MODE>
__global__ __launch_bounds__(256) void kaze_scharr_kernel(const float* __restrict__ in0, const float* __restrict__ in1, float* __restrict__ o0,
                                                          float* __restrict__ o1, int h, int w, int s, float inv, float norm4) {
    extern __shared__ float smem[];
    const int rows = kTH + 2 * s, cols = kTW + 2 * s, ts = cols + 1;
    float* t0 = smem;
    float* t1 = smem + rows * ts;
    const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    load_tile(in0, h, w, y0, x0, s, t0, rows, cols, ts);
    if (MODE == 1) load_tile(in1, h, w, y0, x0, s, t1, rows, cols, ts);
    __syncthreads();
    for (int e = threadIdx.x; e < kTH * kTW; e += 256) {
        const int r = e / kTW, c = e % kTW, y = y0 + r, x = x0 + c;
        if (y >= h || x >= w) continue;
        if (MODE == 0) {
            o0[(size_t)y * w + x] = scharr_x(t0, ts, r + s, c + s, s, inv);
            o1[(size_t)y * w + x] = scharr_y(t0, ts, r + s, c + s, s, inv);
        } else {
            const float lxx = scharr_x(t0, ts, r + s, c + s, s, inv), lxy = scharr_y(t0, ts, r + s, c + s, s, inv);
            const float lyy = scharr_y(t1, ts, r + s, c + s, s, inv);
            const float t1p = lxx * lyy, t2p = lxy * lxy;
            o0[(size_t)y * w + x] = (t1p - t2p) * norm4;
        }
    }
}

// One explicit diffusion step: out = L + half_tau * ((xpos - xneg) + (ypos - yneg)), xpos = (c + cE) (LE - L), xneg = (cW + c) (L - LW),
// ypos = (c + cS) (LS - L), yneg = (cN + c) (L - LN); the clamped border makes the outward flux zero.
__global__ __launch_bounds__(256) void kaze_fed_kernel(const float* __restrict__ L, const float* __restrict__ C, float* __restrict__ out, int h,
                                                       int w, float half_tau) {
    constexpr int ts = kTW + 3;
    __shared__ float sL[(kTH + 2) * ts], sC[(kTH + 2) * ts];
    const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    load_tile(L, h, w, y0, x0, 1, sL, kTH + 2, kTW + 2, ts);
    load_tile(C, h, w, y0, x0, 1, sC, kTH + 2, kTW + 2, ts);
    __syncthreads();
    for (int e = threadIdx.x; e < kTH * kTW; e += 256) {
        const int r = e / kTW, c = e % kTW, y = y0 + r, x = x0 + c;
        if (y >= h || x >= w) continue;
        const int q = (r + 1) * ts + c + 1;
        const float l = sL[q], cc = sC[q];
        const float xpos = (cc + sC[q + 1]) * (sL[q + 1] - l), xneg = (sC[q - 1] + cc) * (l - sL[q - 1]);
        const float ypos = (cc + sC[q + ts]) * (sL[q + ts] - l), yneg = (sC[q - ts] + cc) * (l - sL[q - ts]);
        const float flux = (xpos - xneg) + (ypos - yneg);
        out[(size_t)y * w + x] = l + half_tau * flux;
    }
}

// 3-D quadratic refinement of a[dz][dy][dx] (index = (dz+1)*9 + (dy+1)*3 + (dx+1)): the SURF contract's adjugate solve, restated here
// because surf.hip keeps its own inside its translation unit.  false when the Hessian is singular or any offset exceeds 1.
template <class A>
__device__ __forceinline__ bool kaze_refine(const A& a, float& ox, float& oy, float& os) {
    const float v2 = a[13] + a[13];
    const float gx = (a[14] - a[12]) * 0.5f, gy = (a[16] - a[10]) * 0.5f, gs = (a[22] - a[4]) * 0.5f;
    const float hxx = (a[14] + a[12]) - v2, hyy = (a[16] + a[10]) - v2, hss = (a[22] + a[4]) - v2;
    const float hxy = ((a[17] - a[15]) - (a[11] - a[9])) * 0.25f;
    const float hxs = ((a[23] - a[21]) - (a[5] - a[3])) * 0.25f;
    const float hys = ((a[25] - a[19]) - (a[7] - a[1])) * 0.25f;
    const float c00 = hyy * hss - hys * hys, c01 = hxs * hys - hxy * hss, c02 = hxy * hys - hxs * hyy;
    const float c11 = hxx * hss - hxs * hxs, c12 = hxy * hxs - hxx * hys, c22 = hxx * hyy - hxy * hxy;
    const float D = (hxx * c00 + hxy * c01) + hxs * c02;
    if (D == 0.0f) return false;
    ox = -((c00 * gx + c01 * gy) + c02 * gs) / D;
    oy = -((c01 * gx + c11 * gy) + c12 * gs) / D;
    os = -((c02 * gx + c12 * gy) + c22 * gs) / D;
    return fabsf(ox) <= 1.0f && fabsf(oy) <= 1.0f && fabsf(os) <= 1.0f;
}

// grid (wpr, ceil(h / kDH), n_levels - 2): level m = 1 + blockIdx.z
__global__ __launch_bounds__(256) void kaze_detect_kernel(const float* __restrict__ Rp, KazePlan plan, float thr,
                                                          unsigned long long* __restrict__ bitmap) {
    __shared__ float R[3][kDH + 2][kTW + 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = 1 + blockIdx.z, h = plan.h, w = plan.w;
    const int j0 = blockIdx.x * kTW - 1, i0 = blockIdx.y * kDH - 1;
    constexpr int kTile = (kDH + 2) * (kTW + 2);
    for (int e = tid; e < 3 * kTile; e += 256) {
        const int lv = e / kTile, r = (e % kTile) / (kTW + 2), c = e % (kTW + 2);
        const int i = i0 + r, j = j0 + c;
        float v = 0.0f;
        if (i >= 0 && i < h && j >= 0 && j < w) v = Rp[(size_t)(m - 1 + lv) * plan.pitch + (size_t)i * w + j];
        R[lv][r][c] = v;
    }
    __syncthreads();
    const int mg = plan.margin[m];
    for (int rr = wave; rr < kDH; rr += 4) {
        const int i = blockIdx.y * kDH + rr, j = blockIdx.x * kTW + lane;
        if (i >= h) break;  // (uniform in the wave)
        bool ok = false;
        const float v = R[1][rr + 1][lane + 1];
        if (j < w && v > thr && i >= mg && i <= h - 1 - mg && j >= mg && j <= w - 1 - mg) {
            bool mx = true;
            float a[27];
#pragma unroll
            for (int dz = 0; dz < 3; ++dz)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const float q = R[dz][rr + dy][lane + dx];
                        a[dz * 9 + dy * 3 + dx] = q;
                        if (!(dz == 1 && dy == 1 && dx == 1)) mx = mx && v > q;
                    }
            if (mx) {
                float ox, oy, os;
                ok = kaze_refine(a, ox, oy, os);
            }
        }
        const unsigned long long mask = __ballot(ok);
        if (lane == 0) bitmap[((long long)(m - 1) * h + i) * plan.wpr + blockIdx.x] = mask;
    }
}

// Ordered compaction: bit k of word q becomes keypoint prefix[q] + (set bits below k) as (level, row, col, 0).
__global__ __launch_bounds__(256) void kaze_emit_kernel(const unsigned long long* __restrict__ bitmap, const unsigned int* __restrict__ prefix,
                                                        KazePlan plan, int4* __restrict__ kps, unsigned int kcap) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= plan.n_words) return;
    unsigned long long bits = bitmap[q];
    if (!bits) return;
    unsigned int pos = prefix[q];
    const int jw = (int)(q % plan.wpr);
    const long long row = q / plan.wpr;
    const int i = (int)(row % plan.h), m = 1 + (int)(row / plan.h);
    while (bits) {
        const int k = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        if (pos < kcap) kps[pos] = make_int4(m, i, jw * 64 + k, 0);
        ++pos;
    }
}

__device__ __forceinline__ int round_half_up(float v) { return (int)floorf(v + 0.5f); }

// bilinear sample of plane P at (Y, X): rows first along x, then along y; the four taps are clamped to the plane
__device__ __forceinline__ float bilinear(const float* __restrict__ P, int h, int w, int y0, int y1, int x0, int x1, float ay, float ax) {
    const float p00 = P[(size_t)y0 * w + x0], p01 = P[(size_t)y0 * w + x1], p10 = P[(size_t)y1 * w + x0], p11 = P[(size_t)y1 * w + x1];
    const float top = p00 + ax * (p01 - p00), bot = p10 + ax * (p11 - p10);
    return top + ay * (bot - top);
}

// One wave per keypoint (blockIdx.y: the view of group_dev.h's records, always 0 here).  Every wave of the capacity grid passes every
// barrier; the ones beyond the rows do no work.  UPRIGHT: no orientation stage; the descriptor stage is the same code at
// (c, sn) = (1.0f, 0.0f), which the compiler may fold only as IEEE arithmetic allows, and angle_deg is +0.0.
template <bool UPRIGHT>
__global__ __launch_bounds__(256) void kaze_keypoint_kernel(const float* __restrict__ Rp, const float* __restrict__ Dx, const float* __restrict__ Dy,
                                                            KazePlan plan, const KazeTables* __restrict__ tb, const int4* __restrict__ kps,
                                                            const ViewRows<float>* __restrict__ views, int desc_layout, long long ldd,
                                                            long long ldl) {
    __shared__ float s_a[4][32];
    __shared__ float s_x[4][kGrid * kGrid], s_y[4][kGrid * kGrid];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ViewRows<float> V = views[blockIdx.y];
    const unsigned int kidx = blockIdx.x * 4 + wave;
    const bool active = kidx < V.rows;
    float* __restrict__ desc = V.desc;
    double* __restrict__ loc = V.loc;
    float* __restrict__ aux = V.aux;
    const int h = plan.h, w = plan.w;
    int4 kp = make_int4(1, 1, 1, 0);
    if (active) kp = kps[V.kp0 + kidx];
    const int m = kp.x;
    if (active && lane < 27) {
        const int dz = lane / 9 - 1, dy = (lane % 9) / 3 - 1, dx = lane % 3 - 1;
        s_a[wave][lane] = Rp[(size_t)(m + dz) * plan.pitch + (size_t)(kp.y + dy) * w + (kp.z + dx)];
    }
    __syncthreads();
    float ox = 0.0f, oy = 0.0f, os = 0.0f;
    if (active) kaze_refine(s_a[wave], ox, oy, os);  // (accepted by the detection kernel: same values, same arithmetic)
    const float metric = s_a[wave][13];
    const float px = (float)kp.z + ox, py = (float)kp.y + oy;
    const float sg = plan.sigma[m];
    const float s = os >= 0.0f ? sg + os * (plan.sigma[m + 1] - sg) : sg + os * (sg - plan.sigma[m - 1]);
    const float* __restrict__ Lx = Dx + (size_t)m * plan.pitch;
    const float* __restrict__ Ly = Dy + (size_t)m * plan.pitch;
    __syncthreads();
    // ---- orientation --------------------------------------------------------------------------------------------------
    float c = 1.0f, sn = 0.0f, angle = 0.0f;
    if (!UPRIGHT && active) {
        for (int k = lane; k < kOriN; k += 64) {
            const float X = px + (float)tb->ori_dj[k] * s, Y = py + (float)tb->ori_di[k] * s;
            const size_t at = (size_t)clampi(round_half_up(Y), h - 1) * w + clampi(round_half_up(X), w - 1);
            const float g = tb->ori_g[k];
            s_x[wave][k] = g * Lx[at];
            s_y[wave][k] = g * Ly[at];
        }
    }
    if (!UPRIGHT) __syncthreads();
    if (!UPRIGHT && active) {
        // lane = window; members are summed in sample order 0..108
        const float cw = tb->win_c[lane], sw = tb->win_s[lane];
        float sx = 0.0f, sy = 0.0f;
        for (int k = 0; k < kOriN; ++k) {
            const float vx = s_x[wave][k], vy = s_y[wave][k];
            const float dotp = vx * cw + vy * sw, crs = vx * sw - vy * cw;
            const bool member = dotp > 0.0f && fabsf(crs) <= 0.57735026f * dotp;
            sx = sx + (member ? vx : 0.0f);
            sy = sy + (member ? vy : 0.0f);
        }
        const float score = sx * sx + sy * sy;
        float best = score;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) best = fmaxf(best, __shfl_xor(best, off));
        const unsigned long long tie = __ballot(score == best);
        const int win = __ffsll((long long)tie) - 1;  // the lowest window among equals
        const float bx = __shfl(sx, win), by = __shfl(sy, win);
        if (best > 0.0f) {
            const float n = sqrtf(bx * bx + by * by);
            c = bx / n;
            sn = by / n;
            angle = atan2f(by, bx) * 57.29577951308232f;
            if (angle < 0.0f) angle += 360.0f;
        }
    }
    if (!UPRIGHT) __syncthreads();
    // ---- descriptor ---------------------------------------------------------------------------------------------------
    if (active) {
        for (int q = lane; q < kGrid * kGrid; q += 64) {
            const int r = q / kGrid, cc = q % kGrid;
            const float fu = (float)(cc - 12) * s, fv = (float)(r - 12) * s;
            const float X = px + (c * fu - sn * fv), Y = py + (sn * fu + c * fv);
            const float xf = floorf(X), yf = floorf(Y);
            const float ax = X - xf, ay = Y - yf;
            const int xi = (int)xf, yi = (int)yf;
            const int x0 = clampi(xi, w - 1), x1 = clampi(xi + 1, w - 1), y0 = clampi(yi, h - 1), y1 = clampi(yi + 1, h - 1);
            const float fx = bilinear(Lx, h, w, y0, y1, x0, x1, ay, ax), fy = bilinear(Ly, h, w, y0, y1, x0, x1, ay, ax);
            s_x[wave][q] = c * fx + sn * fy;
            s_y[wave][q] = c * fy - sn * fx;
        }
    }
    __syncthreads();
    if (!active) return;
    // lane = output column: sub-region (R, C) = (lane >> 4, (lane >> 2) & 3), component lane & 3 of (sum dx, sum dy, sum |dx|, sum |dy|);
    // its 9 x 9 samples start at row 5 R, column 5 C of the 24 x 24 grid and are summed rows first
    const int sr = lane >> 2, comp = lane & 3, sri = sr >> 2, srj = sr & 3;
    const float* src = (comp & 1) ? s_y[wave] : s_x[wave];
    float acc = 0.0f;
    for (int a = 0; a < 9; ++a)
        for (int b = 0; b < 9; ++b) {
            const float t = tb->g1[a * 9 + b] * src[(sri * 5 + a) * kGrid + srj * 5 + b];
            acc = acc + (comp >= 2 ? fabsf(t) : t);
        }
    acc = acc * tb->g2[sri * 4 + srj];
    float sq = acc * acc;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sq = sq + __shfl_xor(sq, off);
    const float nrm = sqrtf(sq);
    const float out = nrm > 0.0f ? acc / nrm : 0.0f;
    if (desc_layout == APS_ROWMAJOR) {
        desc[(size_t)kidx * ldd + lane] = out;
        if (ldd >= 128) desc[(size_t)kidx * ldd + 64 + lane] = 0.0f;  // resident rows feed the 128-wide matchers as they are
    } else {
        desc[(size_t)lane * ldd + kidx] = out;
    }
    if (lane == 0) {
        loc[kidx] = (double)px + 1.0;
        loc[(size_t)ldl + kidx] = (double)py + 1.0;
        if (aux) {
            aux[(size_t)kidx * 4 + 0] = s;
            aux[(size_t)kidx * 4 + 1] = angle;
            aux[(size_t)kidx * 4 + 2] = metric;
            aux[(size_t)kidx * 4 + 3] = (float)m;
        }
    }
}

// the view record of group_dev.h's helpers: this entry is a group of one
struct KazeView {
    const uint8_t* img;
    float* desc;
    double* loc;
    float* aux;
    int64_t cap, count;
};

// the checks of the entry, which come before any device work
void check_args(const uint8_t* img, int height, int width, int channels, int img_layout, const aps_kaze_params* params, int desc_layout,
                int64_t cap) {
    APS_REQUIRE(img && params, APS_E_ARG, "NULL argument");
    APS_REQUIRE(height > 0 && width > 0, APS_E_DIM, "empty image");
    APS_REQUIRE(channels == 1 || channels == 3, APS_E_DIM, "channels must be 1 or 3");
    APS_REQUIRE(img_layout == APS_IMG_U8_HWC || img_layout == APS_IMG_U8_MATLAB, APS_E_TYPE, "unknown image layout");
    APS_REQUIRE(desc_layout == APS_ROWMAJOR || desc_layout == APS_COLMAJOR, APS_E_TYPE, "unknown descriptor layout");
    APS_REQUIRE(params->num_octaves >= 1 && params->num_octaves <= 4, APS_E_ARG, "NumOctaves must be in 1..4");
    APS_REQUIRE(params->num_scale_levels >= 3 && params->num_scale_levels <= 10, APS_E_ARG, "NumScaleLevels must be in 3..10");
    APS_REQUIRE(params->threshold >= 0, APS_E_ARG, "Threshold must be >= 0");
    APS_REQUIRE(params->diffusion == APS_KAZE_DIFFUSION_SHARPEDGE || params->diffusion == APS_KAZE_DIFFUSION_EDGE ||
                    params->diffusion == APS_KAZE_DIFFUSION_REGION,
                APS_E_ARG, "unknown Diffusion value %d", params->diffusion);
    APS_REQUIRE(params->diffusion == APS_KAZE_DIFFUSION_REGION, APS_E_ARG,
                "Diffusion 'sharpedge' and 'edge' are not built (they need exp on the device); only 'region' is");
    APS_REQUIRE(cap >= 0 && cap < (int64_t)1 << 31, APS_E_ARG, "capacity out of range");
    APS_REQUIRE((int64_t)height * width < (int64_t)1 << 31, APS_E_ARG, "KAZE: %d x %d pixels exceed the 2^31 elements of a plane", height, width);
}

// ---- selection (DESIGN.md "KAZE selection and Upright") ---------------------------------------------------------------------
// The key of every candidate and its index as the sort's value.  The strength is the candidate's metric: the plane element that
// kaze_keypoint_kernel puts in s_a[wave][13], so the same bits.  rows == 0: strongest-N, the key of group 0.  rows > 0: uniform-N, the
// same key under the segment = the cell of the detection pixel (kp.y, kp.z), the unrefined one that kaze_emit_kernel lists, in the
// rows x cols grid over the image (surf_uniform_key_kernel's composite).
__global__ __launch_bounds__(256) void kaze_key_kernel(const float* __restrict__ Rp, KazePlan plan, const int4* __restrict__ cand, unsigned int n,
                                                       int rows, int cols, unsigned long long* __restrict__ keys,
                                                       unsigned int* __restrict__ vals) {
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 kp = cand[i];
    const float metric = Rp[(size_t)kp.x * plan.pitch + (size_t)kp.y * plan.w + kp.z];
    const unsigned int cell = rows > 0 ? (unsigned int)uniform_cell(kp.y, kp.z, plan.h, plan.w, rows, cols) : 0u;
    keys[i] = (unsigned long long)cell << kSegmentShift | strength_key_f32(metric);
    vals[i] = i;
}

// What both entries hold once the candidates are known: the planes the keypoint kernel reads, the candidate bitmap, whose bit order
// is the canonical order, and the exclusive scan of its popcounts; prefix[plan.n_words] is the number of candidates.  The scratch
// planes of the scale space stay allocated with the rest until the chain returns.
struct KazeFront {
    KazePlan plan;
    In<uint8_t> dimg;
    Ws<float> P0, La, Lb, Cc, Ls, Dx, Dy, Rr, stats;
    Ws<unsigned int> hist, prefix;
    Ws<unsigned long long> bitmap;
};

// plan, scale space, detection and scan on the calling thread's stream; no read-back.  false: no pixel of level 1 lies inside its
// margin.
bool kaze_front(const KazeView* view, int H, int W, int channels, int img_layout, const aps_kaze_params* params, KazeFront& F) {
    const int S = params->num_scale_levels, nl = params->num_octaves * S;
    static_assert(4 * 10 <= kMaxLevels, "the levels of the largest call");
    KazePlan& plan = F.plan;
    std::memset(&plan, 0, sizeof plan);
    plan.n_levels = nl;
    plan.h = H;
    plan.w = W;
    plan.wpr = (int)cdiv(W, 64);
    plan.pitch = (size_t)H * W;
    plan.n_words = (long long)(nl - 2) * H * plan.wpr;
    std::vector<double> sig(nl + 1);
    for (int i = 0; i <= nl; ++i) sig[i] = 1.6 * std::pow(2.0, (double)i / (double)S);
    for (int i = 0; i < nl; ++i) {
        plan.sigma[i] = (float)sig[i];
        plan.step[i] = (int)std::floor(sig[i] + 0.5);
        plan.margin[i] = (int)std::ceil(5.0 * sig[i + 1]) + 2;
        plan.inv[i] = (float)(1.0 / (32.0 * (double)plan.step[i]));
        plan.norm4[i] = (float)(sig[i] * sig[i] * sig[i] * sig[i]);
    }
    if (std::min(H, W) < 2 * plan.margin[1] + 1) return false;
    const size_t N = plan.pitch;
    const GaussW g0 = gauss_weights(1.6, kR0), g1 = gauss_weights(1.0, kR1);
    F.dimg.bind(view->img, N * channels);
    const In<uint8_t>& dimg = F.dimg;
    Ws<float>&P0 = F.P0, &La = F.La, &Lb = F.Lb, &Cc = F.Cc, &Ls = F.Ls, &Dx = F.Dx, &Dy = F.Dy, &Rr = F.Rr, &stats = F.stats;
    for (Ws<float>* plane : {&P0, &La, &Lb, &Cc, &Ls}) plane->alloc(N);
    for (Ws<float>* planes : {&Dx, &Dy, &Rr}) planes->alloc((size_t)nl * N);
    stats.alloc(2);
    Ws<unsigned int>& hist = F.hist;  // [0]: the bits of the largest gradient magnitude
    hist.alloc(1 + kBins);
    const dim3 tiles(cdiv(W, kTW), cdiv(H, kTH));
    {
        Prof prof("kaze_contrast");
        APS_HIP(hipMemsetAsync(hist.get(), 0, (1 + kBins) * sizeof(unsigned int), stream()));
        kaze_gray_kernel<<<cdiv(N, 256), 256, 0, stream()>>>(dimg, H, W, channels, img_layout, P0);
        check_launch("kaze_gray_kernel");
        kaze_smooth_kernel<1><<<tiles, 256, 0, stream()>>>(P0, nullptr, Cc, H, W, g1, nullptr, hist);
        check_launch("kaze_smooth_kernel<1>");
        kaze_hist_kernel<<<std::min(1024u, cdiv(N, 256)), 256, 0, stream()>>>(Cc, N, hist, hist.get() + 1);
        check_launch("kaze_hist_kernel");
        kaze_contrast_kernel<<<1, 64, 0, stream()>>>(hist, hist.get() + 1, stats);
        check_launch("kaze_contrast_kernel");
    }
    {
        Prof prof("kaze_blur0");
        kaze_blur_kernel<kR0><<<tiles, 256, 0, stream()>>>(P0, La, H, W, g0);
        check_launch("kaze_blur_kernel");
    }
    float* cur = La;
    float* nxt = Lb;
    for (int i = 0; i < nl; ++i) {
        const int s = plan.step[i];
        const size_t tile_bytes = (size_t)(kTH + 2 * s) * (kTW + 2 * s + 1) * sizeof(float);
        {
            Prof prof("kaze_smooth");
            kaze_smooth_kernel<0><<<tiles, 256, 0, stream()>>>(cur, Ls, Cc, H, W, g1, stats, nullptr);
            check_launch("kaze_smooth_kernel<0>");
        }
        {
            Prof prof("kaze_deriv");
            kaze_scharr_kernel<0><<<tiles, 256, tile_bytes, stream()>>>(Ls, nullptr, Dx.get() + i * N, Dy.get() + i * N, H, W, s, plan.inv[i], 0.0f);
            check_launch("kaze_scharr_kernel<0>");
        }
        {
            Prof prof("kaze_response");
            kaze_scharr_kernel<1><<<tiles, 256, 2 * tile_bytes, stream()>>>(Dx.get() + i * N, Dy.get() + i * N, Rr.get() + i * N, nullptr, H, W, s,
                                                                            plan.inv[i], plan.norm4[i]);
            check_launch("kaze_scharr_kernel<1>");
        }
        if (i + 1 < nl) {
            Prof prof("kaze_fed");
            for (const float half_tau : fed_half_taus(0.5 * sig[i + 1] * sig[i + 1] - 0.5 * sig[i] * sig[i])) {
                kaze_fed_kernel<<<tiles, 256, 0, stream()>>>(cur, Cc, nxt, H, W, half_tau);
                std::swap(cur, nxt);
            }
            check_launch("kaze_fed_kernel");
        }
    }
    Ws<unsigned long long>& bitmap = F.bitmap;
    Ws<unsigned int>& prefix = F.prefix;
    bitmap.alloc((size_t)plan.n_words + 1);  // (+1: a zero word, whose prefix is the total)
    prefix.alloc((size_t)plan.n_words + 1);
    APS_HIP(hipMemsetAsync(bitmap.get() + plan.n_words, 0, sizeof(unsigned long long), stream()));
    {
        Prof prof("kaze_detect");
        kaze_detect_kernel<<<dim3(plan.wpr, cdiv(H, kDH), nl - 2), 256, 0, stream()>>>(Rr, plan, (float)params->threshold, bitmap);
        check_launch("kaze_detect_kernel");
    }
    exclusive_scan(popcounts(bitmap.get()), prefix.get(), 0u, (size_t)plan.n_words + 1);
    return true;
}

// the first `kcap` set bits of the candidate bitmap -> kps, in canonical order
void kaze_emit(const KazeFront& F, int4* kps, unsigned int kcap) {
    kaze_emit_kernel<<<cdiv((size_t)F.plan.n_words, 256), 256, 0, stream()>>>(F.bitmap, F.prefix, F.plan, kps, kcap);
    check_launch("kaze_emit_kernel");
}

// the rows of the view's record in `kps` -> desc, loc and aux: one launch of `most` waves
void kaze_describe(const KazeFront& F, const int4* kps, GroupOut<float, KazeView>& out, unsigned int most, bool upright) {
    Ws<KazeTables> d_tb(1);
    APS_HIP(hipMemcpyAsync(d_tb, &host_tables(), sizeof(KazeTables), hipMemcpyHostToDevice, stream()));
    {
        Prof prof("kaze_keypoint");
        const dim3 grid(cdiv(most, 4), 1);
        if (upright)
            kaze_keypoint_kernel<true><<<grid, 256, 0, stream()>>>(F.Rr, F.Dx, F.Dy, F.plan, d_tb, kps, out.d_rows, out.desc_layout,
                                                                   (long long)out.ldd, (long long)out.ldl);
        else
            kaze_keypoint_kernel<false><<<grid, 256, 0, stream()>>>(F.Rr, F.Dx, F.Dy, F.plan, d_tb, kps, out.d_rows, out.desc_layout,
                                                                    (long long)out.ldd, (long long)out.ldl);
        check_launch("kaze_keypoint_kernel");
    }
}

inline size_t kaze_row_width(int desc_layout, int64_t ldd) { return desc_layout == APS_ROWMAJOR && ldd >= 128 ? 128 : 64; }

// aps_kaze_extract, and aps_kaze_extract_select without a selection, behind their argument checks.  One read-back: the count.
void kaze_chain(KazeView* view, int H, int W, int channels, int img_layout, const aps_kaze_params* params, bool upright, int desc_layout,
                int64_t ldd, int64_t ldl) {
    ctx();
    view->count = 0;
    unsigned int room[1], n[1];
    check_views(view, 1, 64, desc_layout, ldd, ldl, room);
    KazeFront F;
    if (!kaze_front(view, H, W, channels, img_layout, params, F)) return;  // no features, no error
    GroupOut<float, KazeView> out(view, 1, room, 64, kaze_row_width(desc_layout, ldd), desc_layout, ldd, ldl, nullptr, nullptr);
    ViewLimits lim = {};
    lim.cap[0] = room[0];
    lim.max_features = params->max_features;
    Ws<unsigned int> d_n(1);
    group_rows_kernel<float><<<1, 64, 0, stream()>>>(F.prefix, F.plan.n_words, 1, lim, out.d_rows, d_n);
    check_launch("group_rows_kernel");
    if (room[0]) {
        Ws<int4> kps(room[0]);
        kaze_emit(F, kps, room[0]);
        kaze_describe(F, kps, out, room[0], upright);
    }
    read_back(d_n.get(), n, 1);  // the one read-back of the chain
    settle_counts(view, 1, n, n, params->max_features, "KAZE");
    out.commit(n);
}

// aps_kaze_extract_select with a selection, behind its argument checks: the N strongest candidates, or with grid_rows > 0 N spread
// over the cells of the grid.  Two read-backs: the candidate count, which sizes the sort and the grid below, then the count the
// device kept.  Only the kept candidates reach the keypoint kernel.
void kaze_select_chain(KazeView* view, int H, int W, int channels, int img_layout, const aps_kaze_params* params, long long N, int grid_rows,
                       int grid_cols, bool upright, int desc_layout, int64_t ldd, int64_t ldl) {
    ctx();
    view->count = 0;
    unsigned int room[1];
    check_views(view, 1, 64, desc_layout, ldd, ldl, room);
    KazeFront F;
    if (!kaze_front(view, H, W, channels, img_layout, params, F)) return;
    const unsigned int M = read_back(F.prefix.get() + F.plan.n_words);  // the first read-back: the candidates
    const unsigned int K = (unsigned int)std::min<long long>(M, N), row0 = 0;
    settle_counts(view, 1, &K, &M, params->max_features, "KAZE");
    if (K == 0) return;
    Ws<int4> cand(M), sel;
    kaze_emit(F, cand, M);
    const int4* kps = cand;  // the kept keypoints, in canonical order
    Ws<unsigned int> d_kept(1);
    if (K < M) {
        Prof prof("kaze_select");
        Ws<unsigned long long> keys(M);
        Ws<unsigned int> vals(M);
        kaze_key_kernel<<<cdiv(M, 256), 256, 0, stream()>>>(F.Rr, F.plan, cand, M, grid_rows, grid_cols, keys, vals);
        check_launch("kaze_key_kernel");
        sel.alloc(K);
        select_int4_group(keys, vals, cand, M, K, (unsigned int)(grid_rows * grid_cols), sel, d_kept);
        kps = sel;
    }
    GroupOut<float, KazeView> out(view, 1, &K, 64, kaze_row_width(desc_layout, ldd), desc_layout, ldd, ldl, &row0, &K);
    kaze_describe(F, kps, out, K, upright);
    if (K < M) {  // the second read-back: the count the device kept is the count the host worked out
        const unsigned int kept = read_back(d_kept.get());
        APS_REQUIRE(kept == K, APS_E_INTERNAL, "the selection kept %u rows on the device, %u on the host", kept, K);
    }
    out.commit(&K);
}

}  // namespace
}  // namespace aps

using namespace aps;

extern "C" {

int aps_kaze_extract(const uint8_t* img, int height, int width, int channels, int img_layout, const aps_kaze_params* params, float* desc,
                     int desc_layout, int64_t ldd, double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(count, APS_E_ARG, "NULL argument");
        check_args(img, height, width, channels, img_layout, params, desc_layout, cap);
        KazeView view = {img, desc, loc, aux, cap, 0};
        try {
            kaze_chain(&view, height, width, channels, img_layout, params, false, desc_layout, ldd, ldl);
        } catch (...) {
            *count = view.count;
            throw;
        }
        *count = view.count;
    });
}

int aps_kaze_extract_select(const uint8_t* img, int height, int width, int channels, int img_layout, const aps_kaze_select_params* params,
                            float* desc, int desc_layout, int64_t ldd, double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(count && params, APS_E_ARG, "NULL argument");
        APS_REQUIRE(params->select >= 0 && params->select <= 2, APS_E_ARG, "select must be 0 (none), 1 (strongest-N) or 2 (uniform-N)");
        if (params->select == 1) APS_REQUIRE(params->n_select >= 1, APS_E_ARG, "n_select (NumStrongest) must be at least 1");
        if (params->select == 2) check_uniform(params->n_select, params->grid_rows, params->grid_cols);
        APS_REQUIRE(params->upright == 0 || params->upright == 1, APS_E_ARG, "upright must be 0 or 1");
        check_args(img, height, width, channels, img_layout, &params->kaze, desc_layout, cap);
        const bool uniform = params->select == 2;
        KazeView view = {img, desc, loc, aux, cap, 0};
        try {
            if (params->select == 0)
                kaze_chain(&view, height, width, channels, img_layout, &params->kaze, params->upright != 0, desc_layout, ldd, ldl);
            else
                kaze_select_chain(&view, height, width, channels, img_layout, &params->kaze, params->n_select, uniform ? params->grid_rows : 0,
                                  uniform ? params->grid_cols : 0, params->upright != 0, desc_layout, ldd, ldl);
        } catch (...) {
            *count = view.count;
            throw;
        }
        *count = view.count;
    });
}

}  // extern "C"
