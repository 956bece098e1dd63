// surf.hip — SURF detector + 64-D descriptor on the gfx950.
// Stands behind PP/featureMatching/getFeaturePoints.m:54-55,71-74 (rgb2gray -> detectSURFFeatures(gray, 'NumOctaves', 8) ->
// extractFeatures).  The toolbox functions are closed code; the algorithm is SURF of Bay, Ess, Tuytelaars, Van Gool (2008)
// restated in DESIGN.md "SURF contract", which fixes every operation and summation order below so that a NumPy restatement
// (tests/surf_mirror.py) reproduces the outputs bit for bit.  The design rule that makes this possible: integers wherever
// the algorithm allows (gray plane, integral image, every box and Haar sum), short f32 chains with a written order
// elsewhere, Gaussian weights and window directions from host tables (f64 -> f32), and no device transcendental in any
// stored value or discrete decision (atan2f only feeds aux's angle_deg).
//
// Chain of one call (no host read-back until the final count; every grid is a capacity grid):
//   integral_image        gray plane and the exact 32-bit integral image (integral_dev.h: row scan, column scan, column carry)
//   surf_detect_kernel   per octave: all levels of a 64 x 8 tile (+1 halo) into LDS, threshold, strict 3x3x3 maximum and the
//                         refinement's verdict; one ballot = one 64-bit word of the candidate bitmap, whose bit order IS the
//                         canonical feature order (octave, level, row, col)
//   exclusive scan of the words' popcounts (rocprim), surf_emit_kernel (ordered compaction, no atomics)
//   surf_keypoint_kernel  one wave per keypoint: the 27 responses again, refinement, orientation, descriptor, outputs
// aps_surf_extract_strongest (DESIGN.md "Strongest-N for SIFT and SURF") shares the chain up to the scan, reads the candidate count
// back, and goes on with grids of the candidates' size:
//   surf_emit_kernel      the candidate list
//   surf_metric_kernel    the centre response of every candidate = its metric, as the sort key
//   select_by_key         (select_dev.h) stable radix sort, flags, ballot words, scan; select_compact_kernel (canonical order again)
//   surf_keypoint_kernel  on the kept keypoints only
// aps_surf_extract_uniform (DESIGN.md "Uniform-N selection") is that chain with surf_uniform_key_kernel and select_uniform in the place
// of surf_metric_kernel and select_by_key.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "aps_internal.h"
#include "integral_dev.h"
#include "select_dev.h"

namespace aps {
namespace {

constexpr int kMaxOct = 12;   // octaves of one call (the reference asks for 8)
constexpr int kMaxLev = 8;    // scale levels per octave (the reference's default is 4)
constexpr int kTW = 64, kTH = 8;  // detection tile (samples): a wave's ballot covers one row of it
constexpr int kOriN = 109;        // disc samples of the orientation: integer (di, dj), di^2 + dj^2 < 36
constexpr int kWin = 64;          // positions of the pi/3 sliding window, 360/64 degrees apart

struct SurfOct {
    int step, gh, gw, wpr;  // sampling step (pixels), sample grid, 64-bit bitmap words per grid row
    int size[kMaxLev];      // filter side per level
    float inv[kMaxLev];     // f32(1 / ((2l-1) * l)), l = size / 3: one lobe of Dxx / Dyy; rounded from f64 on the host
    float inv_xy[kMaxLev];  // f32(1 / (l * l)): one box of Dxy
    long long word0;        // first bitmap word of this octave: planes level 1 .. nlv-2, each gh rows of wpr words
};
struct SurfPlan {
    int n_oct, nlv, h, w;
    SurfOct oct[kMaxOct];
};

// host tables (f64 -> f32), uploaded with every call
struct SurfTables {
    float ori_g[kOriN];     // exp(-(di^2 + dj^2) / (2 * 2^2))
    int ori_di[kOriN], ori_dj[kOriN];
    float win_c[kWin], win_s[kWin];  // window directions; quarter turns are exact images of the first quadrant
    float desc_g[400];      // exp(-(fu^2 + fv^2) / (2 * 3.3^2)), fu, fv = (index - 10 + 0.5)
};

const SurfTables& host_tables() {
    static const SurfTables t = [] {
        SurfTables s;
        int n = 0;
        for (int di = -5; di <= 5; ++di)
            for (int dj = -5; dj <= 5; ++dj)
                if (di * di + dj * dj < 36) {
                    s.ori_di[n] = di;
                    s.ori_dj[n] = dj;
                    s.ori_g[n] = (float)std::exp(-(double)(di * di + dj * dj) / 8.0);
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
        for (int r = 0; r < 20; ++r)
            for (int c = 0; c < 20; ++c) {
                const double fu = (double)(c - 10) + 0.5, fv = (double)(r - 10) + 0.5;
                s.desc_g[r * 20 + c] = (float)std::exp(-(fu * fu + fv * fv) / (2.0 * 3.3 * 3.3));
            }
        return s;
    }();
    return t;
}

// det of the box-filter Hessian at pixel (y, x) for filter side S (0 where the filter leaves the image); *trace = Dxx + Dyy.
__device__ __forceinline__ float surf_response(const uint32_t* __restrict__ I, int h, int w, int y, int x, int S, float inv, float inv_xy, float* trace) {
    const int b = (S - 1) >> 1, l = S / 3, hl = (l - 1) >> 1;
    if (trace) *trace = 0.0f;
    if (y - b < 0 || y + b > h - 1 || x - b < 0 || x + b > w - 1) return 0.0f;
    const size_t ws = (size_t)w + 1;
    const int Dxx = (int)(box(I, ws, y - (l - 1), y + (l - 1), x - b, x + b) - 3u * box(I, ws, y - (l - 1), y + (l - 1), x - hl, x + hl));
    const int Dyy = (int)(box(I, ws, y - b, y + b, x - (l - 1), x + (l - 1)) - 3u * box(I, ws, y - hl, y + hl, x - (l - 1), x + (l - 1)));
    const int Dxy = (int)(box(I, ws, y - l, y - 1, x - l, x - 1) + box(I, ws, y + 1, y + l, x + 1, x + l) -
                          box(I, ws, y - l, y - 1, x + 1, x + l) - box(I, ws, y + 1, y + l, x - l, x - 1));
    const float dxx = (float)Dxx * inv, dyy = (float)Dyy * inv, dxy = (float)Dxy * inv_xy;
    if (trace) *trace = dxx + dyy;
    const float t1 = dxx * dyy, t2 = dxy * dxy, t3 = 0.81f * t2;
    return t1 - t3;
}

// 3-D quadratic refinement of a[dz][dy][dx] (index = (dz+1)*9 + (dy+1)*3 + (dx+1)): offsets (ox, oy, os) in sample / level
// units; false when the Hessian is singular or any offset exceeds 1 in magnitude.  One rounding per written operation.
template <class A>
__device__ __forceinline__ bool surf_refine(const A& a, float& ox, float& oy, float& os) {
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

__global__ __launch_bounds__(256) void surf_detect_kernel(const uint32_t* __restrict__ I, int h, int w, SurfOct oc, int nlv, float thr,
                                                          unsigned long long* __restrict__ bitmap) {
    __shared__ float R[kMaxLev][kTH + 2][kTW + 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * kTW - 1, i0 = blockIdx.y * kTH - 1;
    constexpr int kTile = (kTH + 2) * (kTW + 2);
    for (int e = tid; e < nlv * kTile; e += 256) {
        const int lv = e / kTile, r = (e % kTile) / (kTW + 2), c = e % (kTW + 2);
        const int i = i0 + r, j = j0 + c;
        float v = 0.0f;
        if (i >= 0 && i < oc.gh && j >= 0 && j < oc.gw) v = surf_response(I, h, w, i * oc.step, j * oc.step, oc.size[lv], oc.inv[lv], oc.inv_xy[lv], nullptr);
        R[lv][r][c] = v;
    }
    __syncthreads();
    for (int rr = wave; rr < kTH; rr += 4) {
        const int i = blockIdx.y * kTH + rr, j = blockIdx.x * kTW + lane;
        if (i >= oc.gh) break;  // (uniform in the wave)
        for (int m = 1; m <= nlv - 2; ++m) {
            bool ok = false;
            const float v = R[m][rr + 1][lane + 1];
            const int y = i * oc.step, x = j * oc.step, reach = oc.step + ((oc.size[m + 1] - 1) >> 1);
            if (j < oc.gw && v > thr && y - reach >= 0 && y + reach <= h - 1 && x - reach >= 0 && x + reach <= w - 1) {
                bool mx = true;
                float a[27];
#pragma unroll
                for (int dz = 0; dz < 3; ++dz)
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) {
                            const float q = R[m - 1 + dz][rr + dy][lane + dx];
                            a[dz * 9 + dy * 3 + dx] = q;
                            if (!(dz == 1 && dy == 1 && dx == 1)) mx = mx && v > q;
                        }
                if (mx) {
                    float ox, oy, os;
                    ok = surf_refine(a, ox, oy, os);
                }
            }
            const unsigned long long mask = __ballot(ok);
            if (lane == 0) bitmap[oc.word0 + ((long long)(m - 1) * oc.gh + i) * oc.wpr + blockIdx.x] = mask;
        }
    }
}

// Ordered compaction: bit k of word q becomes keypoint prefix[q] + (set bits below k) as (octave, level, row, col).
__global__ __launch_bounds__(256) void surf_emit_kernel(const unsigned long long* __restrict__ bitmap, const unsigned int* __restrict__ prefix,
                                                        long long n_words, SurfPlan plan, int4* __restrict__ kps, unsigned int kcap) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_words) return;
    unsigned long long bits = bitmap[q];
    if (!bits) return;
    unsigned int pos = prefix[q];
    int o = 0;
    while (o + 1 < plan.n_oct && q >= plan.oct[o + 1].word0) ++o;
    const SurfOct& oc = plan.oct[o];
    const long long rel = q - oc.word0;
    const int jw = (int)(rel % oc.wpr), row = (int)(rel / oc.wpr), i = row % oc.gh, m = 1 + row / oc.gh;
    while (bits) {
        const int k = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        if (pos < kcap) kps[pos] = make_int4(o, m, i, jw * 64 + k);
        ++pos;
    }
}

__device__ __forceinline__ int round_half_up(float v) { return (int)floorf(v + 0.5f); }

// Haar responses (integers) at pixel (iy, ix) with half side hs: dx = right - left over rows iy-hs..iy+hs, the centre column
// left out; dy = below - above over columns ix-hs..ix+hs.  false (and zeros) where the window leaves the image.
__device__ __forceinline__ bool haar(const uint32_t* __restrict__ I, int h, int w, int iy, int ix, int hs, int& dx, int& dy) {
    dx = dy = 0;
    if (iy - hs < 0 || iy + hs > h - 1 || ix - hs < 0 || ix + hs > w - 1) return false;
    const size_t ws = (size_t)w + 1;
    dx = (int)(box(I, ws, iy - hs, iy + hs, ix + 1, ix + hs) - box(I, ws, iy - hs, iy + hs, ix - hs, ix - 1));
    dy = (int)(box(I, ws, iy + 1, iy + hs, ix - hs, ix + hs) - box(I, ws, iy - hs, iy - 1, ix - hs, ix + hs));
    return true;
}

// One wave per keypoint.  Every wave of the capacity grid passes every barrier; the ones beyond the count do no work.
__global__ __launch_bounds__(256) void surf_keypoint_kernel(const uint32_t* __restrict__ I, SurfPlan plan, const SurfTables* __restrict__ tb,
                                                            const int4* __restrict__ kps, const unsigned int* __restrict__ d_total,
                                                            unsigned int kcap, int upright, float* __restrict__ desc, int desc_layout,
                                                            long long ldd, double* __restrict__ loc, long long ldl, float* __restrict__ aux) {
    __shared__ float s_a[4][32];
    __shared__ float s_x[4][400], s_y[4][400];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned int kidx = blockIdx.x * 4 + wave;
    const unsigned int total = min(*d_total, kcap);
    const bool active = kidx < total;
    const int h = plan.h, w = plan.w;
    int4 kp = make_int4(0, 1, 0, 0);
    if (active) kp = kps[kidx];
    const SurfOct& oc = plan.oct[kp.x];
    const int m = kp.y;
    float ctr_trace = 0.0f;
    if (active && lane < 27) {
        const int dz = lane / 9 - 1, dy = (lane % 9) / 3 - 1, dx = lane % 3 - 1;
        float tr;
        s_a[wave][lane] = surf_response(I, h, w, (kp.z + dy) * oc.step, (kp.w + dx) * oc.step, oc.size[m + dz], oc.inv[m + dz], oc.inv_xy[m + dz], &tr);
        if (lane == 13) ctr_trace = tr;
    }
    ctr_trace = __shfl(ctr_trace, 13);
    __syncthreads();
    float ox = 0.0f, oy = 0.0f, os = 0.0f;
    if (active) surf_refine(s_a[wave], ox, oy, os);  // (accepted by the detection kernel: same values, same arithmetic)
    const float metric = s_a[wave][13];
    const float px = ((float)kp.w + ox) * (float)oc.step, py = ((float)kp.z + oy) * (float)oc.step;
    const float sizef = (float)oc.size[m] + os * (float)(oc.size[m + 1] - oc.size[m]);
    const float s = (1.2f * sizef) / 9.0f;
    __syncthreads();
    // ---- orientation --------------------------------------------------------------------------------------------------
    float c = 1.0f, sn = 0.0f, angle = 0.0f;
    if (!upright) {
        if (active) {
            const int hs = max(1, round_half_up(2.0f * s));
            for (int k = lane; k < kOriN; k += 64) {
                const float X = px + (float)tb->ori_dj[k] * s, Y = py + (float)tb->ori_di[k] * s;
                int dx, dy;
                haar(I, h, w, round_half_up(Y), round_half_up(X), hs, dx, dy);
                const float g = tb->ori_g[k];
                s_x[wave][k] = g * (float)dx;
                s_y[wave][k] = g * (float)dy;
            }
        }
        __syncthreads();
        if (active) {
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
        __syncthreads();
    }
    // ---- descriptor ---------------------------------------------------------------------------------------------------
    if (active) {
        const int hs = max(1, round_half_up(s));
        for (int q = lane; q < 400; q += 64) {
            const int r = q / 20, cc = q % 20;
            const float fu = ((float)(cc - 10) + 0.5f) * s, fv = ((float)(r - 10) + 0.5f) * s;
            const float X = px + (c * fu - sn * fv), Y = py + (sn * fu + c * fv);
            int dx, dy;
            haar(I, h, w, round_half_up(Y), round_half_up(X), hs, dx, dy);
            const float fx = (float)dx, fy = (float)dy;
            const float tx = c * fx + sn * fy, ty = c * fy - sn * fx;
            const float g = tb->desc_g[q];
            s_x[wave][q] = g * tx;
            s_y[wave][q] = g * ty;
        }
    }
    __syncthreads();
    if (!active) return;
    // lane = output column: sub-region (lane >> 2) of the 4 x 4 grid, component (lane & 3) of (sum dx, sum dy, sum |dx|, sum |dy|)
    const int sr = lane >> 2, comp = lane & 3, sri = sr >> 2, srj = sr & 3;
    const float* src = (comp & 1) ? s_y[wave] : s_x[wave];
    float acc = 0.0f;
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b) {
            const float v = src[(sri * 5 + a) * 20 + srj * 5 + b];
            acc = acc + (comp >= 2 ? fabsf(v) : v);
        }
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
            aux[(size_t)kidx * 4 + 3] = ctr_trace > 0.0f ? 1.0f : (ctr_trace < 0.0f ? -1.0f : 0.0f);
        }
    }
}

// ---- strongest-N (DESIGN.md "Strongest-N for SIFT and SURF") ----------------------------------------------------------------
// The metric of every candidate: the centre response, s_a[wave][13] of surf_keypoint_kernel - the same device function on the same
// operands, so the same bits - as the selection's key (select_dev.h: one group), and the candidate's index as the sort's value.
__device__ __forceinline__ float surf_metric(const uint32_t* __restrict__ I, const SurfPlan& plan, const int4 kp) {
    const SurfOct& oc = plan.oct[kp.x];
    const int m = kp.y;
    float tr;
    return surf_response(I, plan.h, plan.w, kp.z * oc.step, kp.w * oc.step, oc.size[m], oc.inv[m], oc.inv_xy[m], &tr);
}
__global__ __launch_bounds__(256) void surf_metric_kernel(const uint32_t* __restrict__ I, SurfPlan plan, const int4* __restrict__ cand,
                                                          unsigned int n, unsigned long long* __restrict__ keys,
                                                          unsigned int* __restrict__ vals) {
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keys[i] = strength_key_f32(surf_metric(I, plan, cand[i]));
    vals[i] = i;
}

// Uniform-N (DESIGN.md "Uniform-N selection"): the same key under the candidate's segment = the cell of its detection sample
// (i * step, j * step), the unrefined one that surf_emit_kernel lists, in the rows x cols grid over the image.
__global__ __launch_bounds__(256) void surf_uniform_key_kernel(const uint32_t* __restrict__ I, SurfPlan plan, const int4* __restrict__ cand,
                                                               unsigned int n, int rows, int cols, unsigned long long* __restrict__ keys,
                                                               unsigned int* __restrict__ vals) {
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 kp = cand[i];
    const int step = plan.oct[kp.x].step;
    keys[i] = (unsigned long long)uniform_cell(kp.z * step, kp.w * step, plan.h, plan.w, rows, cols) << kSegmentShift |
              strength_key_f32(surf_metric(I, plan, kp));
    vals[i] = i;
}

// the checks of aps_surf_extract, which come before any device work
void check_args(const uint8_t* img, int height, int width, int channels, int img_layout, const aps_surf_params* params, int desc_layout,
                int64_t cap, const int64_t* count) {
    APS_REQUIRE(img && params && count, APS_E_ARG, "NULL argument");
    APS_REQUIRE(height > 0 && width > 0, APS_E_DIM, "empty image");
    APS_REQUIRE(channels == 1 || channels == 3, APS_E_DIM, "channels must be 1 or 3");
    APS_REQUIRE(img_layout == APS_IMG_U8_HWC || img_layout == APS_IMG_U8_MATLAB, APS_E_TYPE, "unknown image layout");
    APS_REQUIRE(desc_layout == APS_ROWMAJOR || desc_layout == APS_COLMAJOR, APS_E_TYPE, "unknown descriptor layout");
    APS_REQUIRE(params->n_octaves >= 1 && params->n_octaves <= kMaxOct, APS_E_ARG, "NumOctaves must be in 1..%d", kMaxOct);
    APS_REQUIRE(params->n_scale_levels >= 3 && params->n_scale_levels <= kMaxLev, APS_E_ARG, "NumScaleLevels must be in 3..%d", kMaxLev);
    APS_REQUIRE(params->metric_threshold >= 0, APS_E_ARG, "MetricThreshold must be >= 0");
    APS_REQUIRE(cap >= 0 && cap < (int64_t)1 << 31, APS_E_ARG, "capacity out of range");
    // the integral image holds exact 32-bit sums: the whole image at full brightness has to fit
    APS_REQUIRE(integral_fits(height, width), APS_E_ARG,
                "SURF: %d x %d pixels exceed the 32-bit integral image (height * width * 255 must stay below 2^32)", height, width);
}

// What both entries hold once the candidates are known: the integral image, the candidate bitmap (bit order = canonical order) and
// the exclusive scan of its popcounts; prefix[n_words] is the number of candidates.
struct SurfFront {
    SurfPlan plan;
    long long n_words = 0;
    In<uint8_t> dimg;
    Ws<uint32_t> T, I;
    Ws<unsigned long long> bitmap;
    Ws<unsigned int> prefix;
    const unsigned int* d_total() const { return prefix.get() + n_words; }
};

// plan, integral image, detection and scan on the calling thread's stream; no read-back.  false: smaller than the first octave's support.
bool surf_front(const uint8_t* img, int H, int W, int channels, int img_layout, const aps_surf_params* params, SurfFront& F) {
    const int nlv = params->n_scale_levels;
    // plan: octaves whose largest filter fits
    SurfPlan& plan = F.plan;
    std::memset(&plan, 0, sizeof plan);
    plan.nlv = nlv;
    plan.h = H;
    plan.w = W;
    long long n_words = 0;
    for (int o = 1; o <= params->n_octaves; ++o) {
        const long long top = 3ll * ((1ll << o) * nlv + 1);
        if (top > std::min(H, W)) break;
        SurfOct& oc = plan.oct[plan.n_oct++];
        oc.step = 1 << (o - 1);
        oc.gh = (H - 1) / oc.step + 1;
        oc.gw = (W - 1) / oc.step + 1;
        oc.wpr = (int)cdiv(oc.gw, 64);
        for (int l = 0; l < nlv; ++l) {
            oc.size[l] = 3 * ((1 << o) * (l + 1) + 1);
            const double lobe = (double)(oc.size[l] / 3);
            oc.inv[l] = (float)(1.0 / ((2.0 * lobe - 1.0) * lobe));
            oc.inv_xy[l] = (float)(1.0 / (lobe * lobe));
        }
        oc.word0 = n_words;
        n_words += (long long)(nlv - 2) * oc.gh * oc.wpr;
    }
    F.n_words = n_words;
    if (plan.n_oct == 0) return false;
    F.dimg.bind(img, (size_t)H * W * channels);
    F.T.alloc((size_t)H * W);
    F.I.alloc((size_t)(H + 1) * (W + 1));
    {
        Prof prof("surf_integral");
        integral_image(F.dimg, H, W, channels, img_layout, F.T, F.I, nullptr);
    }
    F.bitmap.alloc((size_t)n_words + 1);  // (+1: a zero word, whose prefix is the total)
    F.prefix.alloc((size_t)n_words + 1);
    APS_HIP(hipMemsetAsync(F.bitmap.get() + n_words, 0, sizeof(unsigned long long), stream()));
    {
        Prof prof("surf_detect");
        for (int o = 0; o < plan.n_oct; ++o) {
            const SurfOct& oc = plan.oct[o];
            surf_detect_kernel<<<dim3(oc.wpr, cdiv(oc.gh, kTH)), 256, 0, stream()>>>(F.I, H, W, oc, nlv, (float)params->metric_threshold, F.bitmap);
        }
        check_launch("surf_detect_kernel");
    }
    exclusive_scan(popcounts(F.bitmap.get()), F.prefix.get(), 0u, (size_t)n_words + 1);
    return true;
}

// aps_surf_extract_strongest and, with grid_rows > 0, aps_surf_extract_uniform behind their argument checks.  Two read-backs: the
// candidate count, which sizes the grids and the sort below, then the final count.
void surf_strongest_chain(const uint8_t* img, int H, int W, int channels, int img_layout, const aps_surf_params* params, long long N,
                          int grid_rows, int grid_cols, float* desc, int desc_layout, int64_t ldd, double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    ctx();
    *count = 0;
    SurfFront F;
    if (!surf_front(img, H, W, channels, img_layout, params, F)) return;
    const unsigned int M = read_back(F.d_total());  // the first read-back: the candidates
    const unsigned int K = (unsigned int)std::min<long long>(M, N);
    *count = K;
    if (params->max_features > 0 && M > (unsigned int)params->max_features) {
        *count = M;
        fail(APS_E_CAP, "SURF found %u features, more than params.max_features = %d", M, params->max_features);
    }
    if ((int64_t)K > cap) fail(APS_E_CAP, "feature capacity %lld < %u features", (long long)cap, K);
    if (K == 0) return;
    APS_REQUIRE(desc && loc, APS_E_ARG, "NULL output with features present");
    if (desc_layout == APS_ROWMAJOR)
        APS_REQUIRE(ldd >= 64, APS_E_DIM, "ldd < 64");
    else
        APS_REQUIRE(ldd >= cap, APS_E_DIM, "ldd < cap");
    APS_REQUIRE(ldl >= cap, APS_E_DIM, "ldl < cap");
    Ws<int4> cand(M), sel;
    surf_emit_kernel<<<cdiv((size_t)F.n_words, 256), 256, 0, stream()>>>(F.bitmap, F.prefix, F.n_words, F.plan, cand, M);
    check_launch("surf_emit_kernel");
    // the kept keypoints, in canonical order
    Ws<unsigned long long> keys, words;
    Ws<unsigned int> vals, prefix;
    const int4* kps = cand;
    const unsigned int* d_total = F.d_total();
    if (K < M) {
        Prof prof("surf_select");
        keys.alloc(M);
        vals.alloc(M);
        unsigned int n_words = 0;
        if (grid_rows > 0) {  // uniform-N: the candidates that come first in their cell, the cells' shares by water-filling K
            surf_uniform_key_kernel<<<cdiv(M, 256), 256, 0, stream()>>>(F.I, F.plan, cand, M, grid_rows, grid_cols, keys, vals);
            check_launch("surf_uniform_key_kernel");
            UniformBudget budget = {};
            budget.q[0] = K;
            select_uniform(keys, nullptr, vals, M, 1u, (unsigned int)(grid_rows * grid_cols), budget, words, prefix, n_words);
        } else {
            surf_metric_kernel<<<cdiv(M, 256), 256, 0, stream()>>>(F.I, F.plan, cand, M, keys, vals);
            check_launch("surf_metric_kernel");
            select_by_key(keys, vals, M, single_group_cut(M, K), words, prefix, n_words, 32u);
        }
        sel.alloc(K);
        select_compact_kernel<int4><<<cdiv(n_words, 256), 256, 0, stream()>>>(words, prefix, n_words, cand, M, sel, K);
        check_launch("select_compact_kernel");
        kps = sel;
        d_total = prefix.get() + n_words;
    }
    const size_t dwidth = desc_layout == APS_ROWMAJOR && ldd >= 128 ? 128 : 64;
    Out<float> odesc(desc, desc_layout == APS_ROWMAJOR ? (size_t)(K - 1) * ldd + dwidth : (size_t)63 * ldd + K);
    Out<double> oloc(loc, (size_t)ldl + K);
    Out<float> oaux(aux, (size_t)K * 4);
    Ws<SurfTables> d_tb(1);
    APS_HIP(hipMemcpyAsync(d_tb, &host_tables(), sizeof(SurfTables), hipMemcpyHostToDevice, stream()));
    {
        Prof prof("surf_keypoint");
        surf_keypoint_kernel<<<cdiv(K, 4), 256, 0, stream()>>>(F.I, F.plan, d_tb, kps, d_total, K, params->upright ? 1 : 0, odesc, desc_layout,
                                                              (long long)ldd, oloc, (long long)ldl, oaux.present() ? oaux.get() : nullptr);
    }
    check_launch("surf_keypoint_kernel");
    const unsigned int n = read_back(d_total);  // the second read-back: the count the device kept is the count the host worked out
    APS_REQUIRE(n == K, APS_E_INTERNAL, "strongest-N kept %u rows on the device, %u on the host", n, K);
    if (desc_layout == APS_ROWMAJOR)
        odesc.commit_2d(dwidth, K, (size_t)ldd);
    else
        odesc.commit_2d(K, 64, (size_t)ldd);
    oloc.commit_2d(K, 2, (size_t)ldl);
    oaux.commit((size_t)K * 4);
}

}  // namespace
}  // namespace aps

using namespace aps;

extern "C" {

int aps_surf_extract(const uint8_t* img, int height, int width, int channels, int img_layout,
                     const aps_surf_params* params, float* desc, int desc_layout, int64_t ldd,
                     double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        check_args(img, height, width, channels, img_layout, params, desc_layout, cap, count);
        ctx();
        *count = 0;
        const int H = height, W = width;
        SurfFront F;
        if (!surf_front(img, H, W, channels, img_layout, params, F)) return;  // smaller than the first octave's support: no features, no error
        const SurfPlan& plan = F.plan;
        const long long n_words = F.n_words;
        const Ws<uint32_t>& I = F.I;
        const Ws<unsigned long long>& bitmap = F.bitmap;
        const Ws<unsigned int>& prefix = F.prefix;
        const unsigned int* d_total = prefix.get() + n_words;
        const bool write = cap > 0 && desc && loc;
        const unsigned int kcap = write ? (unsigned int)cap : 0u;
        Out<float> odesc, oaux;
        Out<double> oloc;
        const size_t dwidth = desc_layout == APS_ROWMAJOR && ldd >= 128 ? 128 : 64;
        if (write) {
            if (desc_layout == APS_ROWMAJOR)
                APS_REQUIRE(ldd >= 64, APS_E_DIM, "ldd < 64");
            else
                APS_REQUIRE(ldd >= cap, APS_E_DIM, "ldd < cap");
            APS_REQUIRE(ldl >= cap, APS_E_DIM, "ldl < cap");
            odesc.bind(desc, desc_layout == APS_ROWMAJOR ? (size_t)(cap - 1) * ldd + dwidth : (size_t)63 * ldd + cap);
            oloc.bind(loc, (size_t)ldl + cap);
            oaux.bind(aux, (size_t)cap * 4);
            Ws<int4> kps((size_t)kcap);
            Ws<SurfTables> d_tb(1);
            APS_HIP(hipMemcpyAsync(d_tb, &host_tables(), sizeof(SurfTables), hipMemcpyHostToDevice, stream()));
            surf_emit_kernel<<<cdiv((size_t)n_words, 256), 256, 0, stream()>>>(bitmap, prefix, n_words, plan, kps, kcap);
            check_launch("surf_emit_kernel");
            {
                Prof prof("surf_keypoint");
                surf_keypoint_kernel<<<cdiv(kcap, 4), 256, 0, stream()>>>(I, plan, d_tb, kps, d_total, kcap, params->upright ? 1 : 0, odesc,
                                                                         desc_layout, (long long)ldd, oloc, (long long)ldl,
                                                                         oaux.present() ? oaux.get() : nullptr);
            }
            check_launch("surf_keypoint_kernel");
        }
        const unsigned int n = read_back(d_total);  // the one read-back of the chain
        *count = n;
        if (params->max_features > 0 && n > (unsigned int)params->max_features)
            fail(APS_E_CAP, "SURF found %u features, more than params.max_features = %d", n, params->max_features);
        if ((int64_t)n > cap) fail(APS_E_CAP, "feature capacity %lld < %u features", (long long)cap, n);
        if (n == 0) return;
        APS_REQUIRE(desc && loc, APS_E_ARG, "NULL output with features present");
        if (desc_layout == APS_ROWMAJOR)
            odesc.commit_2d(dwidth, n, (size_t)ldd);
        else
            odesc.commit_2d(n, 64, (size_t)ldd);
        oloc.commit_2d(n, 2, (size_t)ldl);
        oaux.commit((size_t)n * 4);
    });
}

int aps_surf_extract_strongest(const uint8_t* img, int height, int width, int channels, int img_layout,
                               const aps_surf_strongest_params* params, float* desc, int desc_layout, int64_t ldd,
                               double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(params, APS_E_ARG, "NULL argument");
        APS_REQUIRE(params->n_strongest >= 1, APS_E_ARG, "n_strongest (NumStrongest) must be at least 1");
        check_args(img, height, width, channels, img_layout, &params->surf, desc_layout, cap, count);
        surf_strongest_chain(img, height, width, channels, img_layout, &params->surf, params->n_strongest, 0, 0, desc, desc_layout, ldd, loc,
                             ldl, aux, cap, count);
    });
}

int aps_surf_extract_uniform(const uint8_t* img, int height, int width, int channels, int img_layout,
                             const aps_surf_uniform_params* params, float* desc, int desc_layout, int64_t ldd,
                             double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        APS_REQUIRE(params, APS_E_ARG, "NULL argument");
        check_uniform(params->strongest.n_strongest, params->grid_rows, params->grid_cols);
        check_args(img, height, width, channels, img_layout, &params->strongest.surf, desc_layout, cap, count);
        surf_strongest_chain(img, height, width, channels, img_layout, &params->strongest.surf, params->strongest.n_strongest,
                             params->grid_rows, params->grid_cols, desc, desc_layout, ldd, loc, ldl, aux, cap, count);
    });
}

}  // extern "C"
