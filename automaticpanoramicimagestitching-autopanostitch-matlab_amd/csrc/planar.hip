// planar.hip — the planar-scan compositor on gfx950: uint8 images + homographies in, uint8 panorama out, every
// canvas-sized array resident on the device.
//
// Restates PP/renderPanorama/renderPanorama.m:519-699 (pureNonRotationalPanoramas: warp every image and its tent
// weight map to the common canvas, 'none' / 'linear' / 'multiband', paint the void, uint8),
// PP/imageProcessing/imageWarp.m:125-168 (bilinear, valid only where all four taps are inside) and the accumulation
// of PP/gainCompensation/gainCompensationH.m:45-52,78-149.
//
// HBM layout
//   source images : the caller's uint8 h x w x c rows, read as they are (1 byte per channel and tap).
//   layers        : float4 (r, g, b, weight) per canvas pixel and image, out_h x out_w, written and read inside the
//                   image's footprint only (struct Rect, render_dev.h); outside it a layer is exactly zero by
//                   construction and is never touched.
// The arithmetic per pixel is the one of image_warp_h_kernel<float, APS_WARP_BILINEAR> (render.hip) applied to
// (float)u8 / 255.0f and to the tent map, so the composite equals the host-orchestrated chain of
// renderPanorama.pureNonRotationalPanoramas bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <vector>

#include "render_dev.h"

namespace aps {

constexpr int kPlanarMaxImages = 64;  // the inside-mask of the weight normalisation is one 64-bit word

struct PlanarJob {
    const uint8_t* src;  // h x w x c, row-major interleaved
    const float* tx;     // tent table, w entries
    const float* ty;     // tent table, h entries
    float4* layer;       // out_h x out_w
    double A[9];         // adjugate of H / H(3,3)
    double det;
    Rect r;              // footprint, clipped to the canvas
    int h, w, c;
    float g[3];
    int pad[2];
};
static_assert(sizeof(PlanarJob) == 160, "aps_planar_composite_bytes counts 160 bytes per image for this table");

// renderPanorama.warpWeights' 1-D factor: t(1:ceil(n/2)) = linspace(0,1,.), t(floor(n/2)+1:n) = linspace(1,0,.), the
// second assignment winning where they overlap; linspace in f64 as start + i * (delta / div) with the last element
// set to the stop value, then cast to f32.
static void planar_tent(int n, float* t) {
    const int a = (n + 1) / 2, b0 = n / 2, nb = n - n / 2;
    for (int k = 0; k < a; ++k) {
        double v = 1.0;
        if (a > 1) {
            const double step = 1.0 / (double)(a - 1);
            v = (double)k * step + 0.0;
            if (k == a - 1) v = 1.0;
        }
        t[k] = (float)v;
    }
    for (int q = 0; q < nb; ++q) {
        double v = 0.0;
        if (nb > 1) {
            const double step = -1.0 / (double)(nb - 1);
            v = (double)q * step + 1.0;
            if (q == nb - 1) v = 0.0;
        }
        t[b0 + q] = (float)v;
    }
}

// Footprint of one image on the canvas: the half-open rectangle outside which planar_layer_kernel accepts no pixel.
//
// The kernel accepts canvas pixel (x, y) when its computed source position lies in S = [1, w) x [1, h).  Take the
// source rectangle grown by half a pixel, G = [0.5, w + 0.5] x [0.5, h + 0.5].  When the denominator
// d(p) = H(3,:) * [p; 1] has one sign on the four corners of G it has that sign on all of G (d is affine, G convex),
// the forward map is continuous there and maps G onto the convex quadrilateral of the mapped corners, so
// H(G) lies in their bounding box.  An accepted pixel's EXACT pre-image lies in G as long as the kernel's f64 error
// in the source position stays below half a pixel; that error is a few ulps times the ratio of the largest term to
// the denominator, which the test |d| > 1e-6 * (|H31 x| + |H32 y| + |H33|) on the corners bounds by ~1e6: far below
// 0.5 for any coordinate a canvas can have.  The box itself is computed in f64 (error << 1 px) and grown by one
// canvas pixel on every side.  When the sign test or the magnitude test fails (the horizon crosses or grazes the
// image) the quadrilateral is not the pre-image and the footprint is the whole canvas.
static Rect planar_footprint(const double* H, int h, int w, int out_h, int out_w, double x0, double y0, double sx, double sy,
                             bool* whole) {
    const Rect all{0, 0, out_w, out_h};
    if (whole) *whole = true;
    const double cx[4] = {0.5, (double)w + 0.5, (double)w + 0.5, 0.5}, cy[4] = {0.5, 0.5, (double)h + 0.5, (double)h + 0.5};
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    int sign = 0;
    for (int i = 0; i < 4; ++i) {
        const double d = (H[2] * cx[i] + H[5] * cy[i]) + H[8];
        const double scale = (std::fabs(H[2] * cx[i]) + std::fabs(H[5] * cy[i])) + std::fabs(H[8]);
        if (!std::isfinite(d) || !(std::fabs(d) > 1e-6 * scale)) return all;
        const int s = d > 0 ? 1 : -1;
        if (sign && s != sign) return all;
        sign = s;
        const double X = ((H[0] * cx[i] + H[3] * cy[i]) + H[6]) / d, Y = ((H[1] * cx[i] + H[4] * cy[i]) + H[7]) / d;
        if (!std::isfinite(X) || !std::isfinite(Y)) return all;
        xmin = std::min(xmin, X), xmax = std::max(xmax, X), ymin = std::min(ymin, Y), ymax = std::max(ymax, Y);
    }
    const double fx0 = std::floor((xmin - x0) / sx) - 1.0, fx1 = std::ceil((xmax - x0) / sx) + 2.0;
    const double fy0 = std::floor((ymin - y0) / sy) - 1.0, fy1 = std::ceil((ymax - y0) / sy) + 2.0;
    if (whole) *whole = false;
    Rect r;
    r.x0 = (int)std::min(std::max(fx0, 0.0), (double)out_w);
    r.x1 = (int)std::min(std::max(fx1, 0.0), (double)out_w);
    r.y0 = (int)std::min(std::max(fy0, 0.0), (double)out_h);
    r.y1 = (int)std::min(std::max(fy1, 0.0), (double)out_h);
    if (r.x1 <= r.x0 || r.y1 <= r.y0) r = Rect{0, 0, 0, 0};
    return r;
}

// The device memory one composite requests (the formula of aps_planar_composite_bytes, include/aps.h).
static int64_t planar_bytes(int n, const int* ih, const int* iw, const int* ic, int out_h, int out_w, int blending, int levels) {
    const int64_t P = (int64_t)out_h * out_w;
    int64_t b = 0;
    for (int k = 0; k < n; ++k) b += (int64_t)ih[k] * iw[k] * ic[k] + 4 * ((int64_t)ih[k] + iw[k]);
    b += (int64_t)n * (int64_t)sizeof(PlanarJob) + 16 * (int64_t)n * P + P + 3 * P;
    if (blending == APS_BLEND_MULTIBAND) {
        const int maxl = (int)std::floor(std::log2((double)std::min(out_h, out_w)));
        const int L = std::max(1, std::min(levels, maxl));
        int64_t down = 0, inner = 0;  // pixels of levels 1..L-1, of levels 1..L-2
        int hl = out_h, wl = out_w;
        for (int l = 1; l < L; ++l) {
            hl = std::max(1, hl / 2);
            wl = std::max(1, wl / 2);
            down += (int64_t)hl * wl;
            if (l < L - 1) inner += (int64_t)hl * wl;
        }
        b += 16 * P;                                           // F
        b += 16 * (int64_t)n * down;                           // the layers' Gaussian levels 1..L-1
        if (L > 1) b += 16 * (int64_t)std::min(n, kMaxK) * P;  // blurred level of one batch of layers
        b += 16 * (P + down) + 16 * inner;                     // numerator pyramid, collapse buffers
    }
    return b;
}

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// One image per blockIdx.z (jobs[k0 + z]), 64 x 4 canvas pixels of its footprint per workgroup.  Inverse map, validity
// and the four-tap sums as image_warp_h_kernel<float, APS_WARP_BILINEAR>: f64, ((w11*p11 + w12*p12) + w21*p21) + w22*p22
// (no contraction: this library is compiled with -ffp-contract=off), rounded to f32; the map is evaluated once for
// colour and weight.
__global__ __launch_bounds__(256) void planar_layer_kernel(const PlanarJob* __restrict__ jobs, int k0, int W, double x0, double y0,
                                                           double sx, double sy) {
    const PlanarJob& j = jobs[k0 + blockIdx.z];
    const int x = j.r.x0 + blockIdx.x * 64 + (threadIdx.x & 63), y = j.r.y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= j.r.x1 || y >= j.r.y1) return;
    const double X = x0 + (double)x * sx, Y = y0 + (double)y * sy;
    const double s0 = ((j.A[0] * X + j.A[3] * Y) + j.A[6]) / j.det;
    const double s1 = ((j.A[1] * X + j.A[4] * Y) + j.A[7]) / j.det;
    const double s2 = ((j.A[2] * X + j.A[5] * Y) + j.A[8]) / j.det;
    double wv = fabs(s2) > 1e-12 ? fabs(s2) : 1e-12;
    wv = s2 < 0 ? -wv : (s2 > 0 ? wv : 0.0);
    const double srcx = s0 / wv, srcy = s1 / wv;
    const double fx1 = floor(srcx), fy1 = floor(srcy);
    const bool valid = fx1 >= 1 && fx1 + 1 <= j.w && fy1 >= 1 && fy1 + 1 <= j.h;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) {
        const int x1 = (int)fx1, y1 = (int)fy1;
        const double wx = srcx - fx1, wy = srcy - fy1;
        const double w11 = (1 - wx) * (1 - wy), w12 = (1 - wx) * wy, w21 = wx * (1 - wy), w22 = wx * wy;
        const int C = j.c;
        const uint8_t* __restrict__ r0 = j.src + ((size_t)(y1 - 1) * j.w + (x1 - 1)) * C;
        const uint8_t* __restrict__ r1 = r0 + (size_t)j.w * C;
        float col[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < C) {
                const double p11 = (double)((float)r0[c] / 255.0f), p21 = (double)((float)r0[C + c] / 255.0f);
                const double p12 = (double)((float)r1[c] / 255.0f), p22 = (double)((float)r1[C + c] / 255.0f);
                col[c] = (float)(((w11 * p11 + w12 * p12) + w21 * p21) + w22 * p22);
            } else {
                col[c] = col[0];
            }
        }
        const float ta = j.ty[y1 - 1], tb = j.ty[y1], tl = j.tx[x1 - 1], tr = j.tx[x1];
        const double t11 = (double)(ta * tl), t12 = (double)(tb * tl), t21 = (double)(ta * tr), t22 = (double)(tb * tr);
        float wgt = (float)(((w11 * t11 + w12 * t12) + w21 * t21) + w22 * t22);
        wgt = wgt < 0.f ? 0.f : (wgt > 1.f ? 1.f : wgt);
        o = make_float4(col[0] * j.g[0], col[1] * j.g[1], col[2] * j.g[2], wgt);
    }
    j.layer[(size_t)y * W + x] = o;
}

// multiBandBlending.m:72-85 over the footprints (w = max(0,w) / sum where sum > 1e-8: the arithmetic of
// norm_weights_kernel, mbb_norm); coverage = any raw weight > 0, taken before the division can flush one to zero.
__global__ __launch_bounds__(256) void planar_norm_kernel(const PlanarJob* __restrict__ jobs, int K, int W, size_t n,
                                                          uint8_t* __restrict__ cov) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
    unsigned long long inside = 0ull;
    float s = 0.f;
    bool any = false;
    for (int k = 0; k < K; ++k) {
        if (!in_rect(jobs[k].r, x, y)) continue;
        inside |= 1ull << k;
        const float wv = jobs[k].layer[p].w;
        s = s + (wv > 0.f ? wv : 0.f);
        any |= wv > 0.f;
    }
    for (int k = 0; k < K; ++k) {
        if (!((inside >> k) & 1)) continue;
        const float w0 = jobs[k].layer[p].w;
        const float wv = w0 > 0.f ? w0 : 0.f;
        jobs[k].layer[p].w = s > 1e-8f ? wv / s : 0.f;
    }
    cov[p] = any ? 1 : 0;
}

// uint8(round(255 * f)) as the host tail forms it: the product in f64, MATLAB round (half away from zero), clamp.
// (paint_kernel of the tiled renderer rounds 255.0f * v in f32, which can land on the other side of a half.)
__device__ __forceinline__ uint8_t planar_u8(float f) {
    const double v = 255.0 * (double)f;
    double r = floor(fabs(v) + 0.5);
    r = v < 0 ? -r : r;
    r = r > 0.0 ? r : 0.0;
    r = r < 255.0 ? r : 255.0;
    return (uint8_t)r;
}

__device__ __forceinline__ void planar_store(uint8_t* __restrict__ pano, uint8_t* __restrict__ covered, size_t p, bool cov,
                                             int white, float r, float g, float b) {
    const uint8_t v = white ? 255 : 0;
    pano[3 * p] = cov ? planar_u8(r) : v;
    pano[3 * p + 1] = cov ? planar_u8(g) : v;
    pano[3 * p + 2] = cov ? planar_u8(b) : v;
    if (covered) covered[p] = cov ? 1 : 0;
}

// MODE APS_BLEND_LINEAR: linear_blend_kernel's sums in image order (a layer outside its footprint adds exact zeros) and its
// division.  MODE APS_BLEND_NONE: the colour of the FIRST layer of maximal weight (numpy argmax / MATLAB max).  Void
// pixels (no weight > 0) take the canvas colour; then uint8.
template <int MODE>
__global__ __launch_bounds__(256) void planar_fuse_kernel(const PlanarJob* __restrict__ jobs, int K, int W, size_t n, int white,
                                                          uint8_t* __restrict__ pano, uint8_t* __restrict__ covered) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
    float acc[3] = {0.f, 0.f, 0.f}, den = 0.f, best = 0.f;
    bool any = false;
    for (int k = 0; k < K; ++k) {
        if (!in_rect(jobs[k].r, x, y)) continue;
        const float4 g = jobs[k].layer[p];
        any |= g.w > 0.f;
        if (MODE == APS_BLEND_LINEAR) {
            acc[0] = acc[0] + g.x * g.w;
            acc[1] = acc[1] + g.y * g.w;
            acc[2] = acc[2] + g.z * g.w;
            den = den + g.w;
        } else if (g.w > best) {
            best = g.w;
            acc[0] = g.x;
            acc[1] = g.y;
            acc[2] = g.z;
        }
    }
    if (MODE == APS_BLEND_LINEAR) {
        const float tiny = 1.1920928955078125e-07f;
        const float d = den > tiny ? den : tiny;
        acc[0] = acc[0] / d;
        acc[1] = acc[1] / d;
        acc[2] = acc[2] / d;
    }
    planar_store(pano, covered, p, any, white, acc[0], acc[1], acc[2]);
}

// the multiband result: max(0, min(1, F)) as unpack_clamp_kernel(clamp01 = 1), void painted, uint8
__global__ __launch_bounds__(256) void planar_finish_kernel(const float4* __restrict__ F, const uint8_t* __restrict__ cov, size_t n,
                                                            int white, uint8_t* __restrict__ pano, uint8_t* __restrict__ covered) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float4 f = F[p];
    float v[3] = {f.x, f.y, f.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = v[c];
        t = t > 0.f ? t : 0.f;  // max(0,F): NaN -> 0
        t = t < 1.f ? t : 1.f;
        v[c] = t;
    }
    planar_store(pano, covered, p, cov[p] != 0, white, v[0], v[1], v[2]);
}

// gainCompensationH.m:45-52,78-149 on the resident layers: gain_stats_warped_kernel with float4 layers and footprints (a
// pair whose footprints do not intersect is never valid together).  One thread per sampled canvas point.
__global__ __launch_bounds__(256) void planar_gain_stats_kernel(const PlanarJob* __restrict__ jobs, int n_img, int W, int ds, int ws,
                                                                int hs, double* __restrict__ Nij, double* __restrict__ sCi,
                                                                double* __restrict__ sCj) {
    __shared__ GainPairTable s_tab;
    s_tab.init();
    const int ix = blockIdx.x * 16 + (threadIdx.x & 15), iy = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (ix < ws && iy < hs) {
        const int x = ix * ds, y = iy * ds;
        auto sample = [&](int k, float* c3) {
            if (!in_rect(jobs[k].r, x, y)) return false;
            const float4 g = jobs[k].layer[(size_t)y * W + x];
            c3[0] = g.x;
            c3[1] = g.y;
            c3[2] = g.z;
            return g.w > 0.f && isfinite(g.x) && isfinite(g.y) && isfinite(g.z);
        };
        for (int i = 0; i < n_img; ++i) {
            float ci[3];
            if (!sample(i, ci)) continue;
            for (int j = i + 1; j < n_img; ++j) {
                float cj[3];
                if (sample(j, cj)) s_tab.add(n_img, i, j, ci, cj, Nij, sCi, sCj);
            }
        }
    }
    s_tab.flush(n_img, Nij, sCi, sCj);
}

// ------------------------------------------------------------------------------------------------
// host orchestration
// ------------------------------------------------------------------------------------------------
struct PlanarLayers {
    std::vector<std::unique_ptr<In<uint8_t>>> imgs;
    Ws<float> tents;
    std::vector<float> host_tents;  // (pageable sources of asynchronous copies live until the call's last synchronise)
    std::vector<Ws<float4>> store;
    std::vector<float4*> layers;
    std::vector<Rect> rects;
    Ws<PlanarJob> jobs;
    std::vector<PlanarJob> host_jobs;
};

static void planar_check_args(const uint8_t* const* images, const int* ih, const int* iw, const int* ic, int n, const double* H,
                              int out_h, int out_w, double sx, double sy) {
    APS_REQUIRE(images && ih && iw && ic && H, APS_E_ARG, "NULL argument");
    APS_REQUIRE(n >= 1, APS_E_ARG, "need at least one image (%d)", n);
    APS_REQUIRE(n <= kPlanarMaxImages, APS_E_DIM, "more than %d images in one planar composite (%d)", kPlanarMaxImages, n);
    APS_REQUIRE(out_h > 0 && out_w > 0 && (int64_t)out_h * out_w < ((int64_t)1 << 31), APS_E_DIM, "bad canvas size %d x %d", out_h,
                out_w);
    APS_REQUIRE(sx > 0 && sy > 0 && std::isfinite(sx) && std::isfinite(sy), APS_E_ARG, "pixel extents must be positive");
    for (int k = 0; k < n; ++k) {
        APS_REQUIRE(images[k], APS_E_ARG, "NULL image %d", k);
        APS_REQUIRE(ih[k] > 0 && iw[k] > 0 && (ic[k] == 1 || ic[k] == 3), APS_E_DIM, "image %d: bad size %d x %d x %d", k, ih[k],
                    iw[k], ic[k]);
        HWarp hw;
        make_hwarp(H + 9 * k, hw);
        // |det| against Hadamard's bound on it (rows and columns of H / H(3,3)): zero up to rounding = no inverse map
        const double* h = H + 9 * k;
        const double s = h[8] != 0 ? h[8] : 1.0;
        double rows = 1.0, cols = 1.0;
        bool fin = true;
        for (int a = 0; a < 3; ++a) {
            double r2 = 0, c2 = 0;
            for (int b = 0; b < 3; ++b) {
                fin = fin && std::isfinite(h[a + 3 * b]);
                r2 += (h[a + 3 * b] / s) * (h[a + 3 * b] / s);
                c2 += (h[b + 3 * a] / s) * (h[b + 3 * a] / s);
            }
            rows *= std::sqrt(r2);
            cols *= std::sqrt(c2);
        }
        APS_REQUIRE(fin && std::isfinite(hw.det) && std::fabs(hw.det) > 1e-14 * std::min(rows, cols), APS_E_ARG,
                    "homography %d is singular or not finite (det %g)", k, hw.det);
    }
}

// Refuses before the first launch when the request cannot fit (renderPanorama.m:245-266: "skip this panorama").
static void planar_precheck(int64_t need) {
    size_t free_b = 0, total_b = 0;
    APS_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t have = free_b + ws_idle_bytes();
    APS_REQUIRE((uint64_t)need <= (uint64_t)have, APS_E_OOM,
                "planar composite needs %lld bytes of device memory, %zu are free: this panorama cannot fit", (long long)need, have);
}

static void planar_build_layers(const uint8_t* const* images, const int* ih, const int* iw, const int* ic, int n, const double* H,
                                int out_h, int out_w, double x0, double y0, double sx, double sy, const float* gains,
                                PlanarLayers& L) {
    const size_t P = (size_t)out_h * out_w;
    const bool no_cull = std::getenv("APS_PLANAR_NO_CULL") != nullptr;
    size_t nt = 0;
    for (int k = 0; k < n; ++k) nt += (size_t)ih[k] + iw[k];
    std::vector<float>& tents = L.host_tents;
    tents.resize(nt);
    L.tents.alloc(nt);
    L.store.resize(n);
    L.layers.resize(n);
    L.rects.resize(n);
    L.host_jobs.resize(n);
    size_t off = 0;
    for (int k = 0; k < n; ++k) {
        PlanarJob& j = L.host_jobs[k];
        L.imgs.emplace_back(new In<uint8_t>(images[k], (size_t)ih[k] * iw[k] * ic[k]));
        j.src = L.imgs.back()->get();
        planar_tent(iw[k], tents.data() + off);
        j.tx = L.tents.get() + off;
        off += iw[k];
        planar_tent(ih[k], tents.data() + off);
        j.ty = L.tents.get() + off;
        off += ih[k];
        L.store[k].alloc(P);
        j.layer = L.layers[k] = L.store[k];
        HWarp hw;
        make_hwarp(H + 9 * k, hw);
        for (int e = 0; e < 9; ++e) j.A[e] = hw.A[e];
        j.det = hw.det;
        j.r = L.rects[k] = no_cull ? Rect{0, 0, out_w, out_h} : planar_footprint(H + 9 * k, ih[k], iw[k], out_h, out_w, x0, y0, sx, sy, nullptr);
        j.h = ih[k], j.w = iw[k], j.c = ic[k];
        for (int c = 0; c < 3; ++c) j.g[c] = gains ? gains[3 * k + c] : 1.0f;
        j.pad[0] = j.pad[1] = 0;
    }
    L.jobs.alloc(n);
    APS_HIP(hipMemcpyAsync(L.tents, tents.data(), nt * sizeof(float), hipMemcpyHostToDevice, stream()));
    APS_HIP(hipMemcpyAsync(L.jobs, L.host_jobs.data(), n * sizeof(PlanarJob), hipMemcpyHostToDevice, stream()));
    Prof prof("planar_layers");
    for (int k0 = 0; k0 < n; k0 += kMaxK) {
        const int kc = std::min(kMaxK, n - k0);
        int mw = 0, mh = 0;
        for (int k = k0; k < k0 + kc; ++k) {
            mw = std::max(mw, L.rects[k].x1 - L.rects[k].x0);
            mh = std::max(mh, L.rects[k].y1 - L.rects[k].y0);
        }
        if (mw <= 0 || mh <= 0) continue;
        planar_layer_kernel<<<dim3(cdiv(mw, 64), cdiv(mh, 4), kc), 256, 0, stream()>>>(L.jobs.get(), k0, out_w, x0, y0, sx, sy);
        check_launch("planar_layer_kernel");
    }
}

}  // namespace aps

using namespace aps;

extern "C" {

int64_t aps_planar_composite_bytes(int n_img, const int* img_h, const int* img_w, const int* img_c, int out_h, int out_w,
                                   int blending, int levels) {
    int64_t bytes = 0;
    const int st = guarded([&] {
        APS_REQUIRE(img_h && img_w && img_c, APS_E_ARG, "NULL argument");
        APS_REQUIRE(n_img >= 1, APS_E_ARG, "need at least one image (%d)", n_img);
        APS_REQUIRE(n_img <= kPlanarMaxImages, APS_E_DIM, "more than %d images in one planar composite (%d)", kPlanarMaxImages, n_img);
        APS_REQUIRE(out_h > 0 && out_w > 0 && (int64_t)out_h * out_w < ((int64_t)1 << 31), APS_E_DIM, "bad canvas size %d x %d", out_h,
                    out_w);
        APS_REQUIRE(blending == APS_BLEND_NONE || blending == APS_BLEND_LINEAR || blending == APS_BLEND_MULTIBAND, APS_E_ARG,
                    "unknown blending mode %d", blending);
        APS_REQUIRE(blending != APS_BLEND_MULTIBAND || levels >= 1, APS_E_ARG, "levels must be a positive integer");
        for (int k = 0; k < n_img; ++k)
            APS_REQUIRE(img_h[k] > 0 && img_w[k] > 0 && (img_c[k] == 1 || img_c[k] == 3), APS_E_DIM, "image %d: bad size %d x %d x %d", k,
                        img_h[k], img_w[k], img_c[k]);
        bytes = planar_bytes(n_img, img_h, img_w, img_c, out_h, out_w, blending, levels);
    });
    return st == APS_OK ? bytes : (int64_t)st;
}

int aps_planar_tent(int n, float* t) {
    return guarded([&] {
        APS_REQUIRE(t, APS_E_ARG, "NULL argument");
        APS_REQUIRE(n >= 1, APS_E_DIM, "bad length %d", n);
        planar_tent(n, t);
    });
}

int aps_planar_footprints(int n_img, const int* img_h, const int* img_w, const double* H, int out_h, int out_w, double x0, double y0,
                          double sx, double sy, int* rects, int* whole) {
    return guarded([&] {
        APS_REQUIRE(img_h && img_w && H && rects, APS_E_ARG, "NULL argument");
        APS_REQUIRE(n_img >= 1 && out_h > 0 && out_w > 0, APS_E_DIM, "bad dimensions");
        APS_REQUIRE(sx > 0 && sy > 0, APS_E_ARG, "pixel extents must be positive");
        for (int k = 0; k < n_img; ++k) {
            APS_REQUIRE(img_h[k] > 0 && img_w[k] > 0, APS_E_DIM, "image %d: bad size", k);
            bool w = false;
            const Rect r = planar_footprint(H + 9 * k, img_h[k], img_w[k], out_h, out_w, x0, y0, sx, sy, &w);
            rects[4 * k] = r.x0, rects[4 * k + 1] = r.y0, rects[4 * k + 2] = r.x1, rects[4 * k + 3] = r.y1;
            if (whole) whole[k] = w ? 1 : 0;
        }
    });
}

int aps_planar_composite(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                         const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int blending, int levels,
                         float sigma, int white_canvas, const float* gains, uint8_t* pano, uint8_t* covered) {
    return guarded([&] {
        planar_check_args(images, img_h, img_w, img_c, n_img, H, out_h, out_w, sx, sy);
        APS_REQUIRE(pano, APS_E_ARG, "NULL argument");
        APS_REQUIRE(blending == APS_BLEND_NONE || blending == APS_BLEND_LINEAR || blending == APS_BLEND_MULTIBAND, APS_E_ARG,
                    "unknown blending mode %d", blending);
        if (blending == APS_BLEND_MULTIBAND) {
            APS_REQUIRE(levels >= 1, APS_E_ARG, "levels must be a positive integer");
            APS_REQUIRE(sigma > 0, APS_E_ARG, "sigma must be positive");
            const Taps tp = make_taps(sigma);
            APS_REQUIRE(tp.r >= 1 && tp.r <= 4, APS_E_ARG, "pyrSigma %g needs a %d-tap filter; 3..9 taps are built", (double)sigma,
                        2 * tp.r + 1);
        }
        ctx();
        planar_precheck(planar_bytes(n_img, img_h, img_w, img_c, out_h, out_w, blending, levels));
        const size_t P = (size_t)out_h * out_w;
        Out<uint8_t> oP(pano, 3 * P), oC(covered, P);
        PlanarLayers L;
        planar_build_layers(images, img_h, img_w, img_c, n_img, H, out_h, out_w, x0, y0, sx, sy, gains, L);
        uint8_t* cov_out = oC.present() ? oC.get() : nullptr;
        const int white = white_canvas ? 1 : 0;
        if (blending == APS_BLEND_MULTIBAND) {
            Ws<uint8_t> cov(P);
            Ws<float4> F(P);
            planar_norm_kernel<<<cdiv(P, 256), 256, 0, stream()>>>(L.jobs.get(), n_img, out_w, P, cov);
            check_launch("planar_norm_kernel");
            multiband_device(L.layers, L.rects.data(), out_h, out_w, levels, sigma, F);
            planar_finish_kernel<<<cdiv(P, 256), 256, 0, stream()>>>(F, cov, P, white, oP.get(), cov_out);
            check_launch("planar_finish_kernel");
        } else {
            if (blending == APS_BLEND_LINEAR)
                planar_fuse_kernel<APS_BLEND_LINEAR><<<cdiv(P, 256), 256, 0, stream()>>>(L.jobs.get(), n_img, out_w, P, white, oP.get(), cov_out);
            else
                planar_fuse_kernel<APS_BLEND_NONE><<<cdiv(P, 256), 256, 0, stream()>>>(L.jobs.get(), n_img, out_w, P, white, oP.get(), cov_out);
            check_launch("planar_fuse_kernel");
        }
        oP.commit();
        oC.commit();
        APS_HIP(hipStreamSynchronize(stream()));  // the staged inputs and the workspace must outlive the launches
    });
}

int aps_planar_gain_stats(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                          const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int downsample,
                          double* n_ij, double* sum_ci, double* sum_cj) {
    return guarded([&] {
        planar_check_args(images, img_h, img_w, img_c, n_img, H, out_h, out_w, sx, sy);
        APS_REQUIRE(n_ij && sum_ci && sum_cj, APS_E_ARG, "NULL argument");
        APS_REQUIRE(downsample >= 1, APS_E_ARG, "overlapDownsample must be >= 1");
        ctx();
        planar_precheck(planar_bytes(n_img, img_h, img_w, img_c, out_h, out_w, APS_BLEND_NONE, 1));
        PlanarLayers L;
        planar_build_layers(images, img_h, img_w, img_c, n_img, H, out_h, out_w, x0, y0, sx, sy, nullptr, L);
        const size_t nn = (size_t)n_img * n_img;
        Out<double> oN(n_ij, nn), oI(sum_ci, 3 * nn), oJ(sum_cj, 3 * nn);
        APS_HIP(hipMemsetAsync(oN.get(), 0, nn * sizeof(double), stream()));
        APS_HIP(hipMemsetAsync(oI.get(), 0, 3 * nn * sizeof(double), stream()));
        APS_HIP(hipMemsetAsync(oJ.get(), 0, 3 * nn * sizeof(double), stream()));
        const int ws = (out_w - 1) / downsample + 1, hs = (out_h - 1) / downsample + 1;  // numel(1:ds:end)
        {
            Prof prof("planar_gain_stats");
            planar_gain_stats_kernel<<<dim3(cdiv(ws, 16), cdiv(hs, 16)), 256, 0, stream()>>>(L.jobs.get(), n_img, out_w, downsample, ws, hs,
                                                                                          oN.get(), oI.get(), oJ.get());
        }
        check_launch("planar_gain_stats_kernel");
        oN.commit();
        oI.commit();
        oJ.commit();
        APS_HIP(hipStreamSynchronize(stream()));
    });
}

}  // extern "C"
