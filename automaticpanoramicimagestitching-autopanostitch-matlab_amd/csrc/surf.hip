// surf.hip — SURF detector + 64-D descriptor on the gfx950.
// Stands behind PP/featureMatching/getFeaturePoints.m:54-55,71-74 (rgb2gray -> detectSURFFeatures(gray, 'NumOctaves', 8) ->
// extractFeatures).  The toolbox functions are closed code; the algorithm is SURF of Bay, Ess, Tuytelaars, Van Gool (2008)
// restated in DESIGN.md "SURF contract", which fixes every operation and summation order below so that a NumPy restatement
// (tests/surf_mirror.py) reproduces the outputs bit for bit.  The design rule that makes this possible: integers wherever
// the algorithm allows (gray plane, integral image, every box and Haar sum), short f32 chains with a written order
// elsewhere, Gaussian weights and window directions from host tables (f64 -> f32), and no device transcendental in any
// stored value or discrete decision (atan2f only feeds aux's angle_deg).
//
// A call works on a group of 1 .. 16 views of one shape (aps_surf_extract_batch; the single-view entries are groups of one): every
// stage below is one launch for the group, with the view as the last grid dimension or decoded from the packed word's offset.
// The integral images lie one after the other, the candidate bitmap is packed [view][octave][level][row][word].
// Chain of one call (no host read-back until the final counts; every grid is a capacity grid):
//   integral_image        gray plane and the exact 32-bit integral image (integral_dev.h: row scan, column scan, column carry)
//   surf_detect_kernel   per octave: all levels of a 64 x 8 tile (+1 halo) into LDS, threshold, strict 3x3x3 maximum and the
//                         refinement's verdict; one ballot = one 64-bit word of the candidate bitmap, whose bit order IS the
//                         canonical feature order (octave, level, row, col) within the view
//   exclusive scan of all views' words' popcounts (rocprim), surf_emit_kernel (ordered compaction, no atomics)
//   group_rows_kernel     (group_dev.h) every view's count, first keypoint and rows to write: all views' or, if one does not fit, none
//   surf_keypoint_kernel  one wave per keypoint: the 27 responses again, refinement, orientation, descriptor, outputs
// aps_surf_extract_strongest and aps_surf_extract_batch_strongest (DESIGN.md "Strongest-N for SIFT and SURF") share the chain up to
// the scan, read the views' candidate counts back, and go on with grids of the candidates' size:
//   surf_emit_kernel      the candidate list, the views' one after the other
//   surf_metric_kernel    the centre response of every candidate = its metric, as the sort key under the view = the selection's group
//   select_by_key         (select_dev.h) stable radix sort, flags, ballot words, scan; select_compact_kernel (canonical order again)
//   surf_keypoint_kernel  on the kept keypoints only
// aps_surf_extract_uniform and aps_surf_extract_batch_uniform (DESIGN.md "Uniform-N selection") are that chain with
// surf_uniform_key_kernel and select_uniform in the place of surf_metric_kernel and select_by_key.
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
    long long n_words;      // bitmap words of one view
    size_t integ_pitch;     // elements of one view's (h + 1) x (w + 1) integral image
    SurfOct oct[kMaxOct];
};
static_assert(kGroupViews == APS_SURF_MAX_VIEWS && kGroupViews <= kSelectGroups, "a view is a group of the selection (select_dev.h)");

// a keypoint of the group as the lists hold it: (octave | view << 16, level, row, col) of its detection sample
__device__ __forceinline__ int kp_octave(const int4 kp) { return kp.x & 0xffff; }
__device__ __forceinline__ int kp_view(const int4 kp) { return kp.x >> 16; }

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

__global__ __launch_bounds__(256) void surf_detect_kernel(const uint32_t* __restrict__ I, size_t integ_pitch, int h, int w, SurfOct oc, int nlv,
                                                          float thr, unsigned long long* __restrict__ bitmap, long long n_words) {
    __shared__ float R[kMaxLev][kTH + 2][kTW + 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    I += blockIdx.z * integ_pitch;  // (the view)
    bitmap += blockIdx.z * n_words;
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

// Ordered compaction: bit k of word q (of n_words, all views') becomes keypoint prefix[q] + (set bits below k) as
// (octave | view << 16, level, row, col); the view and the octave are decoded from the word's offset.
__global__ __launch_bounds__(256) void surf_emit_kernel(const unsigned long long* __restrict__ bitmap, const unsigned int* __restrict__ prefix,
                                                        long long n_words, SurfPlan plan, int4* __restrict__ kps, unsigned int kcap) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_words) return;
    unsigned long long bits = bitmap[q];
    if (!bits) return;
    unsigned int pos = prefix[q];
    const int view = (int)(q / plan.n_words);
    const long long qv = q - view * plan.n_words;
    int o = 0;
    while (o + 1 < plan.n_oct && qv >= plan.oct[o + 1].word0) ++o;
    const SurfOct& oc = plan.oct[o];
    const long long rel = qv - oc.word0;
    const int jw = (int)(rel % oc.wpr), row = (int)(rel / oc.wpr), i = row % oc.gh, m = 1 + row / oc.gh;
    while (bits) {
        const int k = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        if (pos < kcap) kps[pos] = make_int4(o | view << 16, m, i, jw * 64 + k);
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

// One wave per keypoint; blockIdx.y is the view, whose record says where its keypoints start and how many rows it writes.  Every
// wave of the capacity grid passes every barrier; the ones beyond the view's rows do no work.
__global__ __launch_bounds__(256) void surf_keypoint_kernel(const uint32_t* __restrict__ I, SurfPlan plan, const SurfTables* __restrict__ tb,
                                                            const int4* __restrict__ kps, const ViewRows<float>* __restrict__ views,
                                                            int upright, int desc_layout, long long ldd, long long ldl) {
    __shared__ float s_a[4][32];
    __shared__ float s_x[4][400], s_y[4][400];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ViewRows<float> V = views[blockIdx.y];
    const unsigned int kidx = blockIdx.x * 4 + wave;  // the row of the view
    const bool active = kidx < V.rows;
    float* __restrict__ desc = V.desc;
    double* __restrict__ loc = V.loc;
    float* __restrict__ aux = V.aux;
    I += blockIdx.y * plan.integ_pitch;
    const int h = plan.h, w = plan.w;
    int4 kp = make_int4(0, 1, 0, 0);
    if (active) kp = kps[V.kp0 + kidx];
    const SurfOct& oc = plan.oct[kp_octave(kp)];
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
// operands, so the same bits - as the selection's key (select_dev.h: the view is the group), and the candidate's index as the sort's value.
__device__ __forceinline__ float surf_metric(const uint32_t* __restrict__ I, const SurfPlan& plan, const int4 kp) {
    const SurfOct& oc = plan.oct[kp_octave(kp)];
    const int m = kp.y;
    float tr;
    return surf_response(I + kp_view(kp) * plan.integ_pitch, plan.h, plan.w, kp.z * oc.step, kp.w * oc.step, oc.size[m], oc.inv[m], oc.inv_xy[m], &tr);
}
__global__ __launch_bounds__(256) void surf_metric_kernel(const uint32_t* __restrict__ I, SurfPlan plan, const int4* __restrict__ cand,
                                                          unsigned int n, unsigned long long* __restrict__ keys,
                                                          unsigned int* __restrict__ vals) {
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 kp = cand[i];
    keys[i] = (unsigned long long)kp_view(kp) << 60 | strength_key_f32(surf_metric(I, plan, kp));
    vals[i] = i;
}

// Uniform-N (DESIGN.md "Uniform-N selection"): the same key under the candidate's segment = view * cells + the cell of its detection
// sample (i * step, j * step), the unrefined one that surf_emit_kernel lists, in the rows x cols grid over the image.
__global__ __launch_bounds__(256) void surf_uniform_key_kernel(const uint32_t* __restrict__ I, SurfPlan plan, const int4* __restrict__ cand,
                                                               unsigned int n, int rows, int cols, unsigned long long* __restrict__ keys,
                                                               unsigned int* __restrict__ vals) {
    const unsigned int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 kp = cand[i];
    const int step = plan.oct[kp_octave(kp)].step;
    const unsigned int cell = (unsigned int)uniform_cell(kp.z * step, kp.w * step, plan.h, plan.w, rows, cols);
    keys[i] = (unsigned long long)(kp_view(kp) * rows * cols + cell) << kSegmentShift |
              strength_key_f32(surf_metric(I, plan, kp));
    vals[i] = i;
}

// the checks of the SURF entries, which come before any device work
void check_args(const aps_surf_view* views, int nv, int height, int width, int channels, int img_layout, const aps_surf_params* params,
                int desc_layout) {
    APS_REQUIRE(views && params, APS_E_ARG, "NULL argument");
    APS_REQUIRE(nv >= 1 && nv <= kGroupViews, APS_E_ARG, "n_views must be in 1..%d", kGroupViews);
    for (int v = 0; v < nv; ++v) APS_REQUIRE(views[v].img, APS_E_ARG, "NULL argument");
    APS_REQUIRE(height > 0 && width > 0, APS_E_DIM, "empty image");
    APS_REQUIRE(channels == 1 || channels == 3, APS_E_DIM, "channels must be 1 or 3");
    APS_REQUIRE(img_layout == APS_IMG_U8_HWC || img_layout == APS_IMG_U8_MATLAB, APS_E_TYPE, "unknown image layout");
    APS_REQUIRE(desc_layout == APS_ROWMAJOR || desc_layout == APS_COLMAJOR, APS_E_TYPE, "unknown descriptor layout");
    APS_REQUIRE(params->n_octaves >= 1 && params->n_octaves <= kMaxOct, APS_E_ARG, "NumOctaves must be in 1..%d", kMaxOct);
    APS_REQUIRE(params->n_scale_levels >= 3 && params->n_scale_levels <= kMaxLev, APS_E_ARG, "NumScaleLevels must be in 3..%d", kMaxLev);
    APS_REQUIRE(params->metric_threshold >= 0, APS_E_ARG, "MetricThreshold must be >= 0");
    for (int v = 0; v < nv; ++v) APS_REQUIRE(views[v].cap >= 0 && views[v].cap < (int64_t)1 << 31, APS_E_ARG, "capacity out of range");
    // the integral image holds exact 32-bit sums: the whole image at full brightness has to fit
    APS_REQUIRE(integral_fits(height, width), APS_E_ARG,
                "SURF: %d x %d pixels exceed the 32-bit integral image (height * width * 255 must stay below 2^32)", height, width);
}

// What every entry holds once the candidates are known: the views' integral images, the candidate bitmap (bit order = the views one
// after the other, each in canonical order) and the exclusive scan of its popcounts; prefix[v * plan.n_words] is the first candidate
// of view v, prefix[n_words] the number of all.
struct SurfFront {
    SurfPlan plan;
    long long n_words = 0;  // of all views
    std::vector<In<uint8_t>> dimg;
    Ws<uint32_t> T, I;
    Ws<unsigned long long> bitmap;
    Ws<unsigned int> prefix;
};

// plan, integral images, detection and scan of the group on the calling thread's stream; no read-back.  false: smaller than the first
// octave's support.
bool surf_front(const aps_surf_view* views, int nv, int H, int W, int channels, int img_layout, const aps_surf_params* params, SurfFront& F) {
    const int nlv = params->n_scale_levels;
    // plan: octaves whose largest filter fits
    SurfPlan& plan = F.plan;
    std::memset(&plan, 0, sizeof plan);
    plan.nlv = nlv;
    plan.h = H;
    plan.w = W;
    plan.integ_pitch = (size_t)(H + 1) * (W + 1);
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
    plan.n_words = n_words;
    F.n_words = n_words * nv;
    if (plan.n_oct == 0) return false;
    ViewImgs imgs;
    std::memset(&imgs, 0, sizeof imgs);
    F.dimg = std::vector<In<uint8_t>>(nv);
    for (int v = 0; v < nv; ++v) {
        F.dimg[v].bind(views[v].img, (size_t)H * W * channels);
        imgs.p[v] = F.dimg[v];
    }
    const size_t t_pitch = (size_t)H * W;
    F.T.alloc(nv * t_pitch);
    F.I.alloc(nv * plan.integ_pitch);
    {
        Prof prof("surf_integral");
        integral_image(imgs, nv, H, W, channels, img_layout, F.T, t_pitch, F.I, plan.integ_pitch, nullptr, 0);
    }
    F.bitmap.alloc((size_t)F.n_words + 1);  // (+1: a zero word, whose prefix is the total)
    F.prefix.alloc((size_t)F.n_words + 1);
    APS_HIP(hipMemsetAsync(F.bitmap.get() + F.n_words, 0, sizeof(unsigned long long), stream()));
    {
        Prof prof("surf_detect");
        for (int o = 0; o < plan.n_oct; ++o) {
            const SurfOct& oc = plan.oct[o];
            surf_detect_kernel<<<dim3(oc.wpr, cdiv(oc.gh, kTH), nv), 256, 0, stream()>>>(F.I, plan.integ_pitch, H, W, oc, nlv,
                                                                                       (float)params->metric_threshold, F.bitmap, n_words);
        }
        check_launch("surf_detect_kernel");
    }
    exclusive_scan(popcounts(F.bitmap.get()), F.prefix.get(), 0u, (size_t)F.n_words + 1);
    return true;
}

// the rows of the views in `kps` (view v's at its record's kp0) -> every view's desc, loc and aux: one launch, the view in the grid
void surf_describe(const SurfFront& F, const int4* kps, GroupOut<float, aps_surf_view>& out, unsigned int most, int upright) {
    Ws<SurfTables> d_tb(1);
    APS_HIP(hipMemcpyAsync(d_tb, &host_tables(), sizeof(SurfTables), hipMemcpyHostToDevice, stream()));
    {
        Prof prof("surf_keypoint");
        surf_keypoint_kernel<<<dim3(cdiv(most, 4), out.nv), 256, 0, stream()>>>(F.I, F.plan, d_tb, kps, out.d_rows, upright, out.desc_layout,
                                                                               (long long)out.ldd, (long long)out.ldl);
    }
    check_launch("surf_keypoint_kernel");
}

inline size_t surf_row_width(int desc_layout, int64_t ldd) { return desc_layout == APS_ROWMAJOR && ldd >= 128 ? 128 : 64; }

// aps_surf_extract and aps_surf_extract_batch behind their argument checks, on a group of nv views.  One read-back: the views' counts.
void surf_chain(aps_surf_view* views, int nv, int H, int W, int channels, int img_layout, const aps_surf_params* params, int desc_layout,
                int64_t ldd, int64_t ldl) {
    ctx();
    for (int v = 0; v < nv; ++v) views[v].count = 0;
    unsigned int room[kGroupViews], n[kGroupViews];
    check_views(views, nv, 64, desc_layout, ldd, ldl, room);
    SurfFront F;
    if (!surf_front(views, nv, H, W, channels, img_layout, params, F)) return;  // smaller than the first octave's support: no features, no error
    GroupOut<float, aps_surf_view> out(views, nv, room, 64, surf_row_width(desc_layout, ldd), desc_layout, ldd, ldl, nullptr, nullptr);
    ViewLimits lim = {};
    size_t kcap = 0;
    for (int v = 0; v < nv; ++v) kcap += lim.cap[v] = room[v];
    lim.max_features = params->max_features;
    Ws<unsigned int> d_n(nv);
    group_rows_kernel<float><<<1, 64, 0, stream()>>>(F.prefix, F.plan.n_words, nv, lim, out.d_rows, d_n);
    check_launch("group_rows_kernel");
    if (kcap) {  // (views that fit have at most kcap keypoints between them; when one does not fit, no row is written)
        Ws<int4> kps(kcap);
        surf_emit_kernel<<<cdiv((size_t)F.n_words, 256), 256, 0, stream()>>>(F.bitmap, F.prefix, F.n_words, F.plan, kps,
                                                                             (unsigned int)std::min<size_t>(kcap, 0xffffffffu));
        check_launch("surf_emit_kernel");
        surf_describe(F, kps, out, *std::max_element(room, room + nv), params->upright ? 1 : 0);
    }
    read_back(d_n.get(), n, nv);  // the one read-back of the chain
    settle_counts(views, nv, n, n, params->max_features, "SURF");
    out.commit(n);
}

// The selection entries behind their argument checks, on a group of nv views: of every view its N strongest candidates, or with
// grid_rows > 0 N spread over the cells of its grid.  Two read-backs: the views' candidate counts, which size the grids and the sort
// below, then the counts the device kept.
void surf_select_chain(aps_surf_view* views, int nv, int H, int W, int channels, int img_layout, const aps_surf_params* params, long long N,
                       int grid_rows, int grid_cols, int desc_layout, int64_t ldd, int64_t ldl) {
    ctx();
    for (int v = 0; v < nv; ++v) views[v].count = 0;
    unsigned int room[kGroupViews], M[kGroupViews], K[kGroupViews], row0[kGroupViews], kept[kGroupViews];
    check_views(views, nv, 64, desc_layout, ldd, ldl, room);
    SurfFront F;
    if (!surf_front(views, nv, H, W, channels, img_layout, params, F)) return;
    Ws<unsigned int> d_n(nv);
    view_counts_kernel<<<1, 64, 0, stream()>>>(F.prefix, F.plan.n_words, nv, d_n);
    check_launch("view_counts_kernel");
    read_back(d_n.get(), M, nv);  // the first read-back: the candidates
    ViewOffsets off = {};
    unsigned int Kt = 0, most = 0;
    bool cut = false;
    for (int v = 0; v < kGroupViews; ++v) {
        if (v < nv) {
            K[v] = (unsigned int)std::min<long long>(M[v], N);
            row0[v] = Kt;
            Kt += K[v];
            most = std::max(most, K[v]);
            cut = cut || K[v] < M[v];
        }
        off.off[v + 1] = off.off[v] + (v < nv ? M[v] : 0u);
    }
    settle_counts(views, nv, K, M, params->max_features, "SURF");
    if (Kt == 0) return;
    const unsigned int Mt = off.off[nv];
    Ws<int4> cand(Mt), sel;
    surf_emit_kernel<<<cdiv((size_t)F.n_words, 256), 256, 0, stream()>>>(F.bitmap, F.prefix, F.n_words, F.plan, cand, Mt);
    check_launch("surf_emit_kernel");
    // the kept keypoints, the views one after the other, each in canonical order
    const int4* kps = cand;
    if (cut) {  // (a view that keeps all its candidates goes through the selection with them as its budget)
        Prof prof("surf_select");
        Ws<unsigned long long> keys(Mt), words;
        Ws<unsigned int> vals(Mt), prefix;
        unsigned int n_words = 0;
        if (grid_rows > 0) {  // uniform-N: the candidates that come first in their cell, the cells' shares by water-filling K
            surf_uniform_key_kernel<<<cdiv(Mt, 256), 256, 0, stream()>>>(F.I, F.plan, cand, Mt, grid_rows, grid_cols, keys, vals);
            check_launch("surf_uniform_key_kernel");
            UniformBudget budget = {};
            for (int v = 0; v < nv; ++v) budget.q[v] = K[v];
            select_uniform(keys, nullptr, vals, Mt, (unsigned int)nv, (unsigned int)(grid_rows * grid_cols), budget, words, prefix, n_words);
        } else {
            surf_metric_kernel<<<cdiv(Mt, 256), 256, 0, stream()>>>(F.I, F.plan, cand, Mt, keys, vals);
            check_launch("surf_metric_kernel");
            StrongestCut c;
            for (int g = 0; g < kSelectGroups; ++g) {
                c.start[g] = g < nv ? off.off[g] : Mt;
                c.keep[g] = g < nv ? K[g] : 0u;
            }
            select_by_key(keys, vals, Mt, c, words, prefix, n_words, nv > 1 ? 64u : 32u);
        }
        sel.alloc(Kt);
        select_compact_kernel<int4><<<cdiv(n_words, 256), 256, 0, stream()>>>(words, prefix, n_words, cand, Mt, sel, Kt);
        check_launch("select_compact_kernel");
        view_kept_kernel<<<1, 64, 0, stream()>>>(words, prefix, off, nv, d_n);
        check_launch("view_kept_kernel");
        kps = sel;
    }
    GroupOut<float, aps_surf_view> out(views, nv, K, 64, surf_row_width(desc_layout, ldd), desc_layout, ldd, ldl, row0, K);
    surf_describe(F, kps, out, most, params->upright ? 1 : 0);
    read_back(d_n.get(), kept, nv);  // the second read-back: the counts the device kept are the counts the host worked out
    for (int v = 0; v < nv; ++v) APS_REQUIRE(kept[v] == K[v], APS_E_INTERNAL, "strongest-N kept %u rows on the device, %u on the host", kept[v], K[v]);
    out.commit(K);
}

// the single-view entries: a group of one, *count from the view whether the chain returns or fails
template <class Chain>
void surf_single(const uint8_t* img, float* desc, double* loc, float* aux, int64_t cap, int64_t* count, Chain&& chain) {
    APS_REQUIRE(count, APS_E_ARG, "NULL argument");
    aps_surf_view view = {img, desc, loc, aux, cap, *count};
    try {
        chain(&view);
    } catch (...) {
        *count = view.count;
        throw;
    }
    *count = view.count;
}

void surf_plain(aps_surf_view* views, int nv, int height, int width, int channels, int img_layout, const aps_surf_params* params,
                int desc_layout, int64_t ldd, int64_t ldl) {
    check_args(views, nv, height, width, channels, img_layout, params, desc_layout);
    surf_chain(views, nv, height, width, channels, img_layout, params, desc_layout, ldd, ldl);
}

void surf_strongest(aps_surf_view* views, int nv, int height, int width, int channels, int img_layout, const aps_surf_strongest_params* params,
                    int desc_layout, int64_t ldd, int64_t ldl) {
    APS_REQUIRE(params, APS_E_ARG, "NULL argument");
    APS_REQUIRE(params->n_strongest >= 1, APS_E_ARG, "n_strongest (NumStrongest) must be at least 1");
    check_args(views, nv, height, width, channels, img_layout, &params->surf, desc_layout);
    surf_select_chain(views, nv, height, width, channels, img_layout, &params->surf, params->n_strongest, 0, 0, desc_layout, ldd, ldl);
}

void surf_uniform(aps_surf_view* views, int nv, int height, int width, int channels, int img_layout, const aps_surf_uniform_params* params,
                  int desc_layout, int64_t ldd, int64_t ldl) {
    APS_REQUIRE(params, APS_E_ARG, "NULL argument");
    check_uniform(params->strongest.n_strongest, params->grid_rows, params->grid_cols);
    check_args(views, nv, height, width, channels, img_layout, &params->strongest.surf, desc_layout);
    surf_select_chain(views, nv, height, width, channels, img_layout, &params->strongest.surf, params->strongest.n_strongest, params->grid_rows,
                      params->grid_cols, desc_layout, ldd, ldl);
}

}  // namespace

// aps_internal.h: the selection over one group of int4 candidates, with this translation unit's copies of select_dev.h's kernels
void select_int4_group(const unsigned long long* keys, const unsigned int* vals, const int4* cand, unsigned int n, unsigned int keep,
                       unsigned int cells, int4* sel, unsigned int* d_kept) {
    Ws<unsigned long long> words;
    Ws<unsigned int> prefix;
    unsigned int n_words = 0;
    if (cells > 0) {
        UniformBudget budget = {};
        budget.q[0] = keep;
        select_uniform(keys, nullptr, vals, n, 1u, cells, budget, words, prefix, n_words);
    } else {
        select_by_key(keys, vals, n, single_group_cut(n, keep), words, prefix, n_words, 32u);
    }
    select_compact_kernel<int4><<<cdiv(n_words, 256), 256, 0, stream()>>>(words, prefix, n_words, cand, n, sel, keep);
    check_launch("select_compact_kernel");
    ViewOffsets off = {};
    for (int v = 1; v <= kGroupViews; ++v) off.off[v] = n;
    view_kept_kernel<<<1, 64, 0, stream()>>>(words, prefix, off, 1, d_kept);
    check_launch("view_kept_kernel");
}

}  // namespace aps

using namespace aps;

extern "C" {

int aps_surf_extract(const uint8_t* img, int height, int width, int channels, int img_layout,
                     const aps_surf_params* params, float* desc, int desc_layout, int64_t ldd,
                     double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        surf_single(img, desc, loc, aux, cap, count,
                    [&](aps_surf_view* view) { surf_plain(view, 1, height, width, channels, img_layout, params, desc_layout, ldd, ldl); });
    });
}

int aps_surf_extract_strongest(const uint8_t* img, int height, int width, int channels, int img_layout,
                               const aps_surf_strongest_params* params, float* desc, int desc_layout, int64_t ldd,
                               double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        surf_single(img, desc, loc, aux, cap, count,
                    [&](aps_surf_view* view) { surf_strongest(view, 1, height, width, channels, img_layout, params, desc_layout, ldd, ldl); });
    });
}

int aps_surf_extract_uniform(const uint8_t* img, int height, int width, int channels, int img_layout,
                             const aps_surf_uniform_params* params, float* desc, int desc_layout, int64_t ldd,
                             double* loc, int64_t ldl, float* aux, int64_t cap, int64_t* count) {
    return guarded([&] {
        surf_single(img, desc, loc, aux, cap, count,
                    [&](aps_surf_view* view) { surf_uniform(view, 1, height, width, channels, img_layout, params, desc_layout, ldd, ldl); });
    });
}

int aps_surf_extract_batch(aps_surf_view* views, int n_views, int height, int width, int channels, int img_layout,
                           const aps_surf_params* params, int desc_layout, int64_t ldd, int64_t ldl) {
    return guarded([&] { surf_plain(views, n_views, height, width, channels, img_layout, params, desc_layout, ldd, ldl); });
}

int aps_surf_extract_batch_strongest(aps_surf_view* views, int n_views, int height, int width, int channels, int img_layout,
                                     const aps_surf_strongest_params* params, int desc_layout, int64_t ldd, int64_t ldl) {
    return guarded([&] { surf_strongest(views, n_views, height, width, channels, img_layout, params, desc_layout, ldd, ldl); });
}

int aps_surf_extract_batch_uniform(aps_surf_view* views, int n_views, int height, int width, int channels, int img_layout,
                                   const aps_surf_uniform_params* params, int desc_layout, int64_t ldd, int64_t ldl) {
    return guarded([&] { surf_uniform(views, n_views, height, width, channels, img_layout, params, desc_layout, ldd, ldl); });
}

}  // extern "C"

