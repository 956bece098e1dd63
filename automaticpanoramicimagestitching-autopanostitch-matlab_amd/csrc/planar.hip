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
    float4* layer;       // out_h x out_w; the compact compositor: the footprint's pixels, pitch r.x1 - r.x0
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
// planar_layer_pixel: one canvas pixel of one image, shared by the dense and the compact layer kernel (one image per
// blockIdx.z (jobs[k0 + z]), 64 x 4 canvas pixels of its footprint per workgroup).  Inverse map, validity
// and the four-tap sums as image_warp_h_kernel<float, APS_WARP_BILINEAR>: f64, ((w11*p11 + w12*p12) + w21*p21) + w22*p22
// (no contraction: this library is compiled with -ffp-contract=off), rounded to f32; the map is evaluated once for
// colour and weight.
__device__ __forceinline__ float4 planar_layer_pixel(const PlanarJob& j, int x, int y, double x0, double y0, double sx, double sy) {
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
    return o;
}

__global__ __launch_bounds__(256) void planar_layer_kernel(const PlanarJob* __restrict__ jobs, int k0, int W, double x0, double y0,
                                                           double sx, double sy) {
    const PlanarJob& j = jobs[k0 + blockIdx.z];
    const int x = j.r.x0 + blockIdx.x * 64 + (threadIdx.x & 63), y = j.r.y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= j.r.x1 || y >= j.r.y1) return;
    j.layer[(size_t)y * W + x] = planar_layer_pixel(j, x, y, x0, y0, sx, sy);
}

// The same layer stored inside its footprint only: row pitch = the footprint's width (the footprint-compact compositor below).
__global__ __launch_bounds__(256) void planar_layer_compact_kernel(const PlanarJob* __restrict__ jobs, int k0, double x0, double y0,
                                                                   double sx, double sy) {
    const PlanarJob& j = jobs[k0 + blockIdx.z];
    const int x = j.r.x0 + blockIdx.x * 64 + (threadIdx.x & 63), y = j.r.y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= j.r.x1 || y >= j.r.y1) return;
    j.layer[(size_t)(y - j.r.y0) * (j.r.x1 - j.r.x0) + (x - j.r.x0)] = planar_layer_pixel(j, x, y, x0, y0, sx, sy);
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
                              int out_h, int out_w, double sx, double sy, int max_images = kPlanarMaxImages,
                              bool need_images = true) {
    APS_REQUIRE((images || !need_images) && ih && iw && ic && H, APS_E_ARG, "NULL argument");
    APS_REQUIRE(n >= 1, APS_E_ARG, "need at least one image (%d)", n);
    APS_REQUIRE(n <= max_images, APS_E_DIM, "more than %d images in one planar composite (%d)", max_images, n);
    APS_REQUIRE(out_h > 0 && out_w > 0 && (int64_t)out_h * out_w < ((int64_t)1 << 31), APS_E_DIM, "bad canvas size %d x %d", out_h,
                out_w);
    APS_REQUIRE(sx > 0 && sy > 0 && std::isfinite(sx) && std::isfinite(sy), APS_E_ARG, "pixel extents must be positive");
    for (int k = 0; k < n; ++k) {
        APS_REQUIRE(!need_images || images[k], APS_E_ARG, "NULL image %d", k);
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
                                PlanarLayers& L, bool compact = false) {
    // compact: the caller has filled L.layers and L.rects (footprint-sized layers of one arena)
    const size_t P = (size_t)out_h * out_w;
    const bool no_cull = std::getenv("APS_PLANAR_NO_CULL") != nullptr;
    size_t nt = 0;
    for (int k = 0; k < n; ++k) nt += (size_t)ih[k] + iw[k];
    std::vector<float>& tents = L.host_tents;
    tents.resize(nt);
    L.tents.alloc(nt);
    if (!compact) {
        L.store.resize(n);
        L.layers.resize(n);
        L.rects.resize(n);
    }
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
        if (!compact) {
            L.store[k].alloc(P);
            L.layers[k] = L.store[k];
        }
        j.layer = L.layers[k];
        HWarp hw;
        make_hwarp(H + 9 * k, hw);
        for (int e = 0; e < 9; ++e) j.A[e] = hw.A[e];
        j.det = hw.det;
        j.r = L.rects[k] = compact ? L.rects[k] : no_cull ? Rect{0, 0, out_w, out_h} : planar_footprint(H + 9 * k, ih[k], iw[k], out_h, out_w, x0, y0, sx, sy, nullptr);
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
        if (compact)
            planar_layer_compact_kernel<<<dim3(cdiv(mw, 64), cdiv(mh, 4), kc), 256, 0, stream()>>>(L.jobs.get(), k0, x0, y0, sx, sy);
        else
            planar_layer_kernel<<<dim3(cdiv(mw, 64), cdiv(mh, 4), kc), 256, 0, stream()>>>(L.jobs.get(), k0, out_w, x0, y0, sx, sy);
        check_launch("planar_layer_kernel");
    }
}

// ------------------------------------------------------------------------------------------------
// the footprint-compact compositor (aps_planar_composite_compact, aps_planar_gain_stats_compact)
// ------------------------------------------------------------------------------------------------
// Same pixels, same arithmetic and same order of every sum as the dense compositor above; what changes is where a layer
// lives and who looks at it.
//   layers   : every image at every pyramid level is stored inside its footprint only (CLayer: base pointer, footprint,
//              row pitch = the footprint's width), all of them carved out of one arena.  No buffer multiplies the image
//              count by the canvas.
//   lists    : per level, the canvas is cut into 64 x 64 blocks; the host builds, from the footprints alone, the list of
//              images (ascending) whose footprint meets each block and uploads all lists once.  The per-pixel kernels walk the
//              list of their block (a workgroup lies inside one block, so list bounds and entries are wave-uniform loads)
//              instead of all n jobs, and one pass per level accumulates every contributor.
constexpr int kListBlock = 64, kListShift = 6;

struct CLayer {
    float4* p;  // the footprint's pixels, row-major, pitch r.x1 - r.x0
    Rect r;     // footprint at this level, clipped to the level
    int pad[2];
};
static_assert(sizeof(CLayer) == 32, "aps_planar_composite_compact_bytes counts 32 bytes per image and level table entry");

__device__ __forceinline__ size_t c_index(const CLayer& c, int x, int y) {
    return (size_t)(y - c.r.y0) * (size_t)(c.r.x1 - c.r.x0) + (size_t)(x - c.r.x0);
}
__device__ __forceinline__ float4 ld_compact(const CLayer& c, int x, int y) {
    return in_rect(c.r, x, y) ? c.p[c_index(c, x, y)] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Everything the host derives from the shapes and homographies alone: level sizes, the footprints multiband_device derives
// (G_l; blurred G_l = grown by the filter radius; G_(l+1) = map_rect through the resize), arena offsets, contributor lists.
struct CompactPlan {
    int L = 1;
    std::vector<int> lh, lw;
    std::vector<std::vector<Rect>> gr, br;          // [level][image]
    std::vector<std::vector<int64_t>> goff, boff;  // pixel offsets into the layer arena / the blur scratch
    int64_t layer_px = 0, blur_px = 0;
    std::vector<int> bw, bh;                        // blocks per row / column of a level
    std::vector<int64_t> list_off;                  // start of a level's (start[blocks + 1], idx[entries]) in `lists`
    std::vector<int> lists;
    int64_t list_ints = 0;
};

static int compact_levels(int out_h, int out_w, int blending, int levels) {
    if (blending != APS_BLEND_MULTIBAND) return 1;
    const int maxl = (int)std::floor(std::log2((double)std::min(out_h, out_w)));
    return std::max(1, std::min(levels, maxl));
}

// radius: the Gaussian's (make_taps(sigma).r); fill_lists = false only counts them (the byte formula needs no entries)
static void compact_plan(int n, const int* ih, const int* iw, const double* H, int out_h, int out_w, double x0, double y0, double sx,
                         double sy, int L, int radius, bool fill_lists, CompactPlan& pl) {
    const bool no_cull = std::getenv("APS_PLANAR_NO_CULL") != nullptr;
    pl.L = L;
    pl.lh.assign(L, out_h);
    pl.lw.assign(L, out_w);
    for (int l = 1; l < L; ++l) {
        pl.lh[l] = std::max(1, pl.lh[l - 1] / 2);
        pl.lw[l] = std::max(1, pl.lw[l - 1] / 2);
    }
    pl.gr.assign(L, std::vector<Rect>(n));
    pl.br.assign(L, std::vector<Rect>(n));
    pl.goff.assign(L, std::vector<int64_t>(n, 0));
    pl.boff.assign(L, std::vector<int64_t>(n, 0));
    for (int k = 0; k < n; ++k)
        pl.gr[0][k] = no_cull ? Rect{0, 0, out_w, out_h}
                              : clip_rect(planar_footprint(H + 9 * k, ih[k], iw[k], out_h, out_w, x0, y0, sx, sy, nullptr), out_w, out_h);
    auto area = [](const Rect& r) { return (int64_t)(r.x1 - r.x0) * (int64_t)(r.y1 - r.y0); };
    pl.layer_px = pl.blur_px = 0;
    for (int l = 0; l < L; ++l) {
        int64_t blur = 0;
        for (int k = 0; k < n; ++k) {
            const Rect g = pl.gr[l][k];
            const bool empty = g.x1 <= g.x0;
            pl.br[l][k] = empty ? g : clip_rect(Rect{g.x0 - radius, g.y0 - radius, g.x1 + radius, g.y1 + radius}, pl.lw[l], pl.lh[l]);
            if (l + 1 < L) {
                pl.gr[l + 1][k] = empty ? g : map_rect(pl.br[l][k], pl.lh[l], pl.lw[l], pl.lh[l + 1], pl.lw[l + 1]);
                pl.boff[l][k] = blur;
                blur += area(pl.br[l][k]);
            }
            pl.goff[l][k] = pl.layer_px;
            pl.layer_px += area(g);
        }
        pl.blur_px = std::max(pl.blur_px, blur);
    }
    // contributor lists: count per block, prefix sums, then fill with the images in ascending order
    pl.bw.resize(L);
    pl.bh.resize(L);
    pl.list_off.resize(L);
    pl.list_ints = 0;
    std::vector<std::vector<int>> count(L);
    for (int l = 0; l < L; ++l) {
        pl.bw[l] = (pl.lw[l] + kListBlock - 1) >> kListShift;
        pl.bh[l] = (pl.lh[l] + kListBlock - 1) >> kListShift;
        const size_t nb = (size_t)pl.bw[l] * pl.bh[l];
        if (fill_lists) count[l].assign(nb + 1, 0);
        int64_t entries = 0;
        for (int k = 0; k < n; ++k) {
            const Rect g = pl.gr[l][k];
            if (g.x1 <= g.x0) continue;
            const int bx0 = g.x0 >> kListShift, bx1 = (g.x1 - 1) >> kListShift, by0 = g.y0 >> kListShift, by1 = (g.y1 - 1) >> kListShift;
            entries += (int64_t)(bx1 - bx0 + 1) * (by1 - by0 + 1);
            if (fill_lists)
                for (int by = by0; by <= by1; ++by)
                    for (int bx = bx0; bx <= bx1; ++bx) ++count[l][(size_t)by * pl.bw[l] + bx + 1];
        }
        pl.list_off[l] = pl.list_ints;
        pl.list_ints += (int64_t)nb + 1 + entries;
    }
    APS_REQUIRE(pl.list_ints < ((int64_t)1 << 31) && (int64_t)n * (2 * L - 1) < ((int64_t)1 << 31), APS_E_DIM,
                "planar composite: %d images on this canvas exceed the int32 range of the contributor lists", n);
    if (!fill_lists) return;
    pl.lists.assign((size_t)pl.list_ints, 0);
    for (int l = 0; l < L; ++l) {
        const size_t nb = (size_t)pl.bw[l] * pl.bh[l];
        int* start = pl.lists.data() + pl.list_off[l];
        int* idx = start + nb + 1;
        for (size_t b = 0; b < nb; ++b) start[b + 1] = start[b] + count[l][b + 1];
        std::vector<int>& fill = count[l];  // reused: entries written so far per block
        std::fill(fill.begin(), fill.end(), 0);
        for (int k = 0; k < n; ++k) {
            const Rect g = pl.gr[l][k];
            if (g.x1 <= g.x0) continue;
            const int bx0 = g.x0 >> kListShift, bx1 = (g.x1 - 1) >> kListShift, by0 = g.y0 >> kListShift, by1 = (g.y1 - 1) >> kListShift;
            for (int by = by0; by <= by1; ++by)
                for (int bx = bx0; bx <= bx1; ++bx) {
                    const size_t b = (size_t)by * pl.bw[l] + bx;
                    idx[start[b] + fill[b]++] = k;
                }
        }
    }
}

// The device memory one compact composite requests (the formula of aps_planar_composite_compact_bytes, include/aps.h).
static int64_t compact_bytes(const CompactPlan& pl, int n, const int* ih, const int* iw, const int* ic, int out_h, int out_w, int blending) {
    const int64_t P = (int64_t)out_h * out_w;
    int64_t b = 0;
    for (int k = 0; k < n; ++k) b += (int64_t)ih[k] * iw[k] * ic[k] + 4 * ((int64_t)ih[k] + iw[k]);
    b += (int64_t)n * (int64_t)sizeof(PlanarJob) + (int64_t)sizeof(CLayer) * n * (2 * pl.L - 1);
    b += 16 * pl.layer_px + 16 * pl.blur_px + 4 * pl.list_ints + P + 3 * P;
    if (blending == APS_BLEND_MULTIBAND) {
        int64_t down = 0, inner = 0;
        for (int l = 1; l < pl.L; ++l) {
            down += (int64_t)pl.lh[l] * pl.lw[l];
            if (l < pl.L - 1) inner += (int64_t)pl.lh[l] * pl.lw[l];
        }
        b += 16 * P + 16 * (P + down) + 16 * inner;  // F, numerator pyramid, collapse buffers
    }
    return b;
}

// ---- kernels -------------------------------------------------------------------------------------
// A workgroup of 64 x 4 (or 32 x 4) pixels lies inside one 64 x 64 block: blockIdx.x * width and blockIdx.y * 4 never
// straddle a multiple of 64.
struct BlockList {
    const int* __restrict__ idx;
    int n;
};
__device__ __forceinline__ BlockList block_list(const int* __restrict__ lists, int bw, int nblocks, int x, int y) {
    const int b = (y >> kListShift) * bw + (x >> kListShift);
    const int s = lists[b];
    return BlockList{lists + nblocks + 1 + s, lists[b + 1] - s};
}

// planar_norm_kernel over the block's contributors
__global__ __launch_bounds__(256) void compact_norm_kernel(const CLayer* __restrict__ G, const int* __restrict__ lists, int bw,
                                                           int nblocks, int W, int Hh, uint8_t* __restrict__ cov) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= Hh) return;
    const BlockList bl = block_list(lists, bw, nblocks, x, y);
    float s = 0.f;
    bool any = false;
    for (int i = 0; i < bl.n; ++i) {
        const CLayer& c = G[bl.idx[i]];
        if (!in_rect(c.r, x, y)) continue;
        const float wv = c.p[c_index(c, x, y)].w;
        s = s + (wv > 0.f ? wv : 0.f);
        any |= wv > 0.f;
    }
    for (int i = 0; i < bl.n; ++i) {
        const CLayer& c = G[bl.idx[i]];
        if (!in_rect(c.r, x, y)) continue;
        float4* q = c.p + c_index(c, x, y);
        const float w0 = q->w;
        const float wv = w0 > 0.f ? w0 : 0.f;
        q->w = s > 1e-8f ? wv / s : 0.f;
    }
    cov[(size_t)y * W + x] = any ? 1 : 0;
}

// planar_fuse_kernel over the block's contributors
template <int MODE>
__global__ __launch_bounds__(256) void compact_fuse_kernel(const CLayer* __restrict__ G, const int* __restrict__ lists, int bw,
                                                           int nblocks, int W, int Hh, int white, uint8_t* __restrict__ pano,
                                                           uint8_t* __restrict__ covered) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= Hh) return;
    const BlockList bl = block_list(lists, bw, nblocks, x, y);
    float acc[3] = {0.f, 0.f, 0.f}, den = 0.f, best = 0.f;
    bool any = false;
    for (int i = 0; i < bl.n; ++i) {
        const CLayer& c = G[bl.idx[i]];
        if (!in_rect(c.r, x, y)) continue;
        const float4 g = c.p[c_index(c, x, y)];
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
    planar_store(pano, covered, (size_t)y * W + x, any, white, acc[0], acc[1], acc[2]);
}

// mb_blur_kernel (render.hip) on compact layers: column pass then row pass through one LDS tile, replicate padding at the
// level's border, the same fmaf chains; one image per blockIdx.z, input inside G's footprint, output inside B's.
constexpr int kCBW = 32, kCBH = 16;
template <int R>
__global__ __launch_bounds__(256) void compact_blur_kernel(const CLayer* __restrict__ G, const CLayer* __restrict__ B, int k0, int h,
                                                           int w, Taps tp) {
    const CLayer in = G[k0 + blockIdx.z], out = B[k0 + blockIdx.z];
    constexpr int IW = kCBW + 2 * R, IH = kCBH + 2 * R;
    const int x0 = out.r.x0 + blockIdx.x * kCBW, y0 = out.r.y0 + blockIdx.y * kCBH, tid = threadIdx.x;
    if (x0 >= out.r.x1 || y0 >= out.r.y1) return;  // the grid is sized for the largest output rect of the launch
    __shared__ float4 s_in[IH * IW];
    __shared__ float4 s_v[kCBH * IW];
    for (int e = tid; e < IH * IW; e += 256) {
        const int ly = e / IW, lx = e - ly * IW;
        const int gy = min(max(y0 + ly - R, 0), h - 1), gx = min(max(x0 + lx - R, 0), w - 1);
        s_in[e] = ld_compact(in, gx, gy);
    }
    __syncthreads();
    for (int e = tid; e < kCBH * IW; e += 256) {
        const int ly = e / IW, lx = e - ly * IW;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t <= 2 * R; ++t) a = fma4(tp.k[t], s_in[(ly + t) * IW + lx], a);
        s_v[e] = a;
    }
    __syncthreads();
    for (int e = tid; e < kCBH * kCBW; e += 256) {
        const int ly = e / kCBW, lx = e - ly * kCBW;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= out.r.x1 || gy >= out.r.y1) continue;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t <= 2 * R; ++t) a = fma4(tp.k[t], s_v[ly * IW + lx + t], a);
        out.p[c_index(out, gx, gy)] = a;
    }
}

// resize_at (render.hip) with the load left to the caller: ld(x, y) returns the input pixel (zero outside a footprint).
// Both passes of imresize for one output pixel, the smaller scale factor first, the same fmaf chains and zero-tap skips.
template <bool ROWS_FIRST, class Ld>
__device__ __forceinline__ float4 resize_with(const Ld& ld, int h, int w, int Pr, int lr, const float* wr, int Pc, int lc,
                                              const float* wc) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ROWS_FIRST) {
        for (int tc = 0; tc < Pc; ++tc) {
            if (wc[tc] == 0.f) continue;
            const int xx = min(max(lc + tc, 1), w) - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int tr = 0; tr < Pr; ++tr)
                if (wr[tr] != 0.f) v = fma4(wr[tr], ld(xx, min(max(lr + tr, 1), h) - 1), v);
            a = fma4(wc[tc], v, a);
        }
    } else {
        for (int tr = 0; tr < Pr; ++tr) {
            if (wr[tr] == 0.f) continue;
            const int yy = min(max(lr + tr, 1), h) - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int tc = 0; tc < Pc; ++tc)
                if (wc[tc] != 0.f) v = fma4(wc[tc], ld(min(max(lc + tc, 1), w) - 1, yy), v);
            a = fma4(wr[tr], v, a);
        }
    }
    return a;
}

// mb_resize_kernel on compact layers: blurred level (B, h x w) -> next Gaussian level (D, oh x ow), one image per blockIdx.z
template <bool ROWS_FIRST>
__global__ __launch_bounds__(128) void compact_resize_kernel(const CLayer* __restrict__ B, const CLayer* __restrict__ D, int k0, int h,
                                                             int w, int oh, int ow) {
    const CLayer in = B[k0 + blockIdx.z], out = D[k0 + blockIdx.z];
    const int x = out.r.x0 + blockIdx.x * 32 + (threadIdx.x & 31), y = out.r.y0 + blockIdx.y * 4 + (threadIdx.x >> 5);
    if (x >= out.r.x1 || y >= out.r.y1) return;
    int lr, lc;
    float wr[12], wc[12];
    const int Pr = resize_taps(h, oh, y, lr, wr);
    const int Pc = resize_taps(w, ow, x, lc, wc);
    out.p[c_index(out, x, y)] =
        resize_with<ROWS_FIRST>([&](int xx, int yy) { return ld_compact(in, xx, yy); }, h, w, Pr, lr, wr, Pc, lc, wc);
}

// mb_lap_all_kernel over the block's contributors: Num_l = sum_k (G_k - imresize(D_k, size_l)) .* w_k in ascending image order
// from +0, every contributor in this one pass; has_d == 0: the coarsest level, Num_L = sum_k G_k .* w_k.
template <bool ROWS_FIRST>
__global__ __launch_bounds__(128) void compact_lap_kernel(const CLayer* __restrict__ G, const CLayer* __restrict__ D,
                                                          const int* __restrict__ lists, int bw, int nblocks, int has_d, int h, int w,
                                                          int dh, int dw, float4* __restrict__ num) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 4 + (threadIdx.x >> 5);
    if (x >= w || y >= h) return;
    const BlockList bl = block_list(lists, bw, nblocks, x, y);
    float acc[3] = {0.f, 0.f, 0.f};
    int lr = 0, lc = 0, Pr = 0, Pc = 0;
    float wr[12], wc[12];
    bool have_taps = false;
    for (int i = 0; i < bl.n; ++i) {
        const int k = bl.idx[i];
        const CLayer& c = G[k];
        if (!in_rect(c.r, x, y)) continue;
        const float4 g = c.p[c_index(c, x, y)];
        if (!has_d) {
            acc[0] = acc[0] + g.x * g.w;
            acc[1] = acc[1] + g.y * g.w;
            acc[2] = acc[2] + g.z * g.w;
            continue;
        }
        if (!have_taps) {
            Pr = resize_taps(dh, h, y, lr, wr);
            Pc = resize_taps(dw, w, x, lc, wc);
            have_taps = true;
        }
        const CLayer& d = D[k];
        const float4 u = resize_with<ROWS_FIRST>([&](int xx, int yy) { return ld_compact(d, xx, yy); }, dh, dw, Pr, lr, wr, Pc, lc, wc);
        acc[0] = acc[0] + (g.x - u.x) * g.w;
        acc[1] = acc[1] + (g.y - u.y) * g.w;
        acc[2] = acc[2] + (g.z - u.z) * g.w;
    }
    num[(size_t)y * w + x] = make_float4(acc[0], acc[1], acc[2], 0.f);
}

// mb_collapse_kernel: F_l = imresize(F_(l+1), size_l) + Num_l (canvas-sized buffers, no layers involved)
template <bool ROWS_FIRST>
__global__ __launch_bounds__(128) void compact_collapse_kernel(const float4* __restrict__ Fc, int ch, int cw,
                                                               const float4* __restrict__ num, int h, int w, float4* __restrict__ out) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 4 + (threadIdx.x >> 5);
    if (x >= w || y >= h) return;
    int lr, lc;
    float wr[12], wc[12];
    const int Pr = resize_taps(ch, h, y, lr, wr);
    const int Pc = resize_taps(cw, w, x, lc, wc);
    const float4 u = resize_with<ROWS_FIRST>([&](int xx, int yy) { return Fc[(size_t)yy * cw + xx]; }, ch, cw, Pr, lr, wr, Pc, lc, wc);
    const float4 n = num[(size_t)y * w + x];
    out[(size_t)y * w + x] = make_float4(u.x + n.x, u.y + n.y, u.z + n.z, 0.f);
}

// planar_gain_stats_kernel over the block's contributors: the pairs of a sampled point are pairs of its block's list
__global__ __launch_bounds__(256) void compact_gain_stats_kernel(const CLayer* __restrict__ G, const int* __restrict__ lists, int bw,
                                                                 int nblocks, int n_img, int ds, int ws, int hs,
                                                                 double* __restrict__ Nij, double* __restrict__ sCi,
                                                                 double* __restrict__ sCj) {
    __shared__ GainPairTable s_tab;
    s_tab.init();
    const int ix = blockIdx.x * 16 + (threadIdx.x & 15), iy = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (ix < ws && iy < hs) {
        const int x = ix * ds, y = iy * ds;
        const BlockList bl = block_list(lists, bw, nblocks, x, y);
        auto sample = [&](int k, float* c3) {
            const CLayer& c = G[k];
            if (!in_rect(c.r, x, y)) return false;
            const float4 g = c.p[c_index(c, x, y)];
            c3[0] = g.x;
            c3[1] = g.y;
            c3[2] = g.z;
            return g.w > 0.f && isfinite(g.x) && isfinite(g.y) && isfinite(g.z);
        };
        for (int a = 0; a < bl.n; ++a) {
            float ci[3];
            const int i = bl.idx[a];
            if (!sample(i, ci)) continue;
            for (int b = a + 1; b < bl.n; ++b) {
                float cj[3];
                const int j = bl.idx[b];
                if (sample(j, cj)) s_tab.add(n_img, i, j, ci, cj, Nij, sCi, sCj);
            }
        }
    }
    s_tab.flush(n_img, Nij, sCi, sCj);
}

// ---- host orchestration --------------------------------------------------------------------------
struct CompactDevice {
    PlanarLayers L;
    Ws<float4> arena, blur;
    Ws<CLayer> tab;  // G tables of levels 0..L-1, then B tables of levels 0..L-2, n entries each
    std::vector<CLayer> host_tab;
    Ws<int> lists;
    const CLayer* G(int l, int n) const { return tab.get() + (size_t)l * n; }
    const CLayer* B(int l, int n, int L_) const { return tab.get() + (size_t)(L_ + l) * n; }
};

// Allocates the arena, uploads tables and lists, warps every image into its footprint (level 0).
static void compact_setup(const CompactPlan& pl, const uint8_t* const* images, const int* ih, const int* iw, const int* ic, int n,
                          const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, const float* gains,
                          CompactDevice& D) {
    const int L = pl.L;
    D.arena.alloc((size_t)pl.layer_px);
    if (pl.blur_px) D.blur.alloc((size_t)pl.blur_px);
    D.host_tab.resize((size_t)n * (2 * L - 1));
    for (int l = 0; l < L; ++l)
        for (int k = 0; k < n; ++k) {
            D.host_tab[(size_t)l * n + k] = CLayer{D.arena.get() + pl.goff[l][k], pl.gr[l][k], {0, 0}};
            if (l + 1 < L) D.host_tab[(size_t)(L + l) * n + k] = CLayer{D.blur.get() + pl.boff[l][k], pl.br[l][k], {0, 0}};
        }
    D.tab.alloc(D.host_tab.size());
    D.lists.alloc(pl.lists.size());
    APS_HIP(hipMemcpyAsync(D.tab, D.host_tab.data(), D.host_tab.size() * sizeof(CLayer), hipMemcpyHostToDevice, stream()));
    APS_HIP(hipMemcpyAsync(D.lists, pl.lists.data(), pl.lists.size() * sizeof(int), hipMemcpyHostToDevice, stream()));
    D.L.layers.resize(n);
    D.L.rects.resize(n);
    for (int k = 0; k < n; ++k) {
        D.L.layers[k] = D.arena.get() + pl.goff[0][k];
        D.L.rects[k] = pl.gr[0][k];
    }
    planar_build_layers(images, ih, iw, ic, n, H, out_h, out_w, x0, y0, sx, sy, gains, D.L, true);
}

// multiband_device on compact layers with normalised weights: per level, blur and downsample every layer inside its
// footprints (16 images per launch), then ONE Laplacian pass over the level for all contributors; then the collapse.
static void compact_multiband(const CompactPlan& pl, const CompactDevice& D, int n, float sigma, float4* F) {
    Prof prof("multiband_compact");
    const int L = pl.L;
    const Taps tp = make_taps(sigma);
    std::vector<Ws<float4>> num(L);
    for (int l = 0; l < L; ++l) num[l].alloc((size_t)pl.lh[l] * pl.lw[l]);
    auto span = [](const Rect* r, int count, int& mw, int& mh) {
        mw = mh = 0;
        for (int k = 0; k < count; ++k) {
            mw = std::max(mw, r[k].x1 - r[k].x0);
            mh = std::max(mh, r[k].y1 - r[k].y0);
        }
    };
    for (int l = 0; l < L; ++l) {
        const int hl = pl.lh[l], wl = pl.lw[l];
        const bool last = l == L - 1;
        const int nh = last ? 0 : pl.lh[l + 1], nw = last ? 0 : pl.lw[l + 1];
        const CLayer* G = D.G(l, n);
        if (!last) {
            const CLayer *B = D.B(l, n, L), *Dn = D.G(l + 1, n);
            const bool rf = rows_first(hl, wl, nh, nw);
            for (int k0 = 0; k0 < n; k0 += kMaxK) {
                const int kc = std::min(kMaxK, n - k0);
                int mw, mh;
                span(pl.br[l].data() + k0, kc, mw, mh);
                if (mw > 0 && mh > 0) {
                    const dim3 bg(cdiv(mw, kCBW), cdiv(mh, kCBH), kc);
                    switch (tp.r) {
                        case 1: compact_blur_kernel<1><<<bg, 256, 0, stream()>>>(G, B, k0, hl, wl, tp); break;
                        case 2: compact_blur_kernel<2><<<bg, 256, 0, stream()>>>(G, B, k0, hl, wl, tp); break;
                        case 3: compact_blur_kernel<3><<<bg, 256, 0, stream()>>>(G, B, k0, hl, wl, tp); break;
                        default: compact_blur_kernel<4><<<bg, 256, 0, stream()>>>(G, B, k0, hl, wl, tp); break;
                    }
                }
                span(pl.gr[l + 1].data() + k0, kc, mw, mh);
                if (mw > 0 && mh > 0) {
                    const dim3 rg(cdiv(mw, 32), cdiv(mh, 4), kc);
                    if (rf)
                        compact_resize_kernel<true><<<rg, 128, 0, stream()>>>(B, Dn, k0, hl, wl, nh, nw);
                    else
                        compact_resize_kernel<false><<<rg, 128, 0, stream()>>>(B, Dn, k0, hl, wl, nh, nw);
                }
            }
            check_launch("compact pyramid level");
        }
        float4* dst = (last && L == 1) ? F : num[l].get();
        const int* lists = D.lists.get() + pl.list_off[l];
        const int nblocks = pl.bw[l] * pl.bh[l];
        const dim3 lg(cdiv(wl, 32), cdiv(hl, 4));
        if (last || rows_first(nh, nw, hl, wl))
            compact_lap_kernel<true><<<lg, 128, 0, stream()>>>(G, last ? G : D.G(l + 1, n), lists, pl.bw[l], nblocks, last ? 0 : 1, hl, wl, nh, nw, dst);
        else
            compact_lap_kernel<false><<<lg, 128, 0, stream()>>>(G, D.G(l + 1, n), lists, pl.bw[l], nblocks, 1, hl, wl, nh, nw, dst);
        check_launch("compact_lap_kernel");
    }
    std::vector<Ws<float4>> fl(std::max(L - 1, 0));
    const float4* cur = L > 1 ? num[L - 1].get() : nullptr;
    for (int l = L - 2; l >= 0; --l) {
        float4* dst = F;
        if (l > 0) {
            fl[l].alloc((size_t)pl.lh[l] * pl.lw[l]);
            dst = fl[l];
        }
        const dim3 cg(cdiv(pl.lw[l], 32), cdiv(pl.lh[l], 4));
        if (rows_first(pl.lh[l + 1], pl.lw[l + 1], pl.lh[l], pl.lw[l]))
            compact_collapse_kernel<true><<<cg, 128, 0, stream()>>>(cur, pl.lh[l + 1], pl.lw[l + 1], num[l], pl.lh[l], pl.lw[l], dst);
        else
            compact_collapse_kernel<false><<<cg, 128, 0, stream()>>>(cur, pl.lh[l + 1], pl.lw[l + 1], num[l], pl.lh[l], pl.lw[l], dst);
        check_launch("compact_collapse_kernel");
        cur = dst;
    }
}

constexpr int kCompactMaxImages = 0x7fffffff;  // what remains is the int32 range of tables and lists (compact_plan)
constexpr int kCompactRadius = 4;  // the byte formula charges every footprint as for the widest filter built (9 taps)
constexpr int kCompactGainMaxImages = 65535;  // GainPairTable keys a pair as i * n + j + 1 in 32 bits

static void compact_check_blending(int blending, int levels, float sigma, bool need_sigma) {
    APS_REQUIRE(blending == APS_BLEND_NONE || blending == APS_BLEND_LINEAR || blending == APS_BLEND_MULTIBAND, APS_E_ARG,
                "unknown blending mode %d", blending);
    if (blending == APS_BLEND_MULTIBAND) {
        APS_REQUIRE(levels >= 1, APS_E_ARG, "levels must be a positive integer");
        if (!need_sigma) return;
        APS_REQUIRE(sigma > 0, APS_E_ARG, "sigma must be positive");
        const Taps tp = make_taps(sigma);
        APS_REQUIRE(tp.r >= 1 && tp.r <= 4, APS_E_ARG, "pyrSigma %g needs a %d-tap filter; 3..9 taps are built", (double)sigma,
                    2 * tp.r + 1);
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

int64_t aps_planar_composite_compact_bytes(int n_img, const int* img_h, const int* img_w, const int* img_c, const double* H, int out_h,
                                           int out_w, double x0, double y0, double sx, double sy, int blending, int levels) {
    int64_t bytes = 0;
    const int st = guarded([&] {
        planar_check_args(nullptr, img_h, img_w, img_c, n_img, H, out_h, out_w, sx, sy, kCompactMaxImages, false);
        compact_check_blending(blending, levels, 0.f, false);
        CompactPlan pl;
        compact_plan(n_img, img_h, img_w, H, out_h, out_w, x0, y0, sx, sy, compact_levels(out_h, out_w, blending, levels), kCompactRadius,
                     false, pl);
        bytes = compact_bytes(pl, n_img, img_h, img_w, img_c, out_h, out_w, blending);
    });
    return st == APS_OK ? bytes : (int64_t)st;
}

int aps_planar_composite_compact(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                                 const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int blending,
                                 int levels, float sigma, int white_canvas, const float* gains, uint8_t* pano, uint8_t* covered) {
    return guarded([&] {
        planar_check_args(images, img_h, img_w, img_c, n_img, H, out_h, out_w, sx, sy, kCompactMaxImages);
        APS_REQUIRE(pano, APS_E_ARG, "NULL argument");
        compact_check_blending(blending, levels, sigma, true);
        ctx();
        const int L = compact_levels(out_h, out_w, blending, levels);
        CompactPlan pl;
        compact_plan(n_img, img_h, img_w, H, out_h, out_w, x0, y0, sx, sy, L, kCompactRadius, false, pl);
        planar_precheck(compact_bytes(pl, n_img, img_h, img_w, img_c, out_h, out_w, blending));
        compact_plan(n_img, img_h, img_w, H, out_h, out_w, x0, y0, sx, sy, L, blending == APS_BLEND_MULTIBAND ? make_taps(sigma).r : 0, true,
                     pl);
        const size_t P = (size_t)out_h * out_w;
        Out<uint8_t> oP(pano, 3 * P), oC(covered, P);
        CompactDevice D;
        compact_setup(pl, images, img_h, img_w, img_c, n_img, H, out_h, out_w, x0, y0, sx, sy, gains, D);
        uint8_t* cov_out = oC.present() ? oC.get() : nullptr;
        const int white = white_canvas ? 1 : 0, nblocks = pl.bw[0] * pl.bh[0];
        const int* lists0 = D.lists.get() + pl.list_off[0];
        const dim3 pg(cdiv(out_w, 64), cdiv(out_h, 4));
        if (blending == APS_BLEND_MULTIBAND) {
            Ws<uint8_t> cov(P);
            Ws<float4> F(P);
            compact_norm_kernel<<<pg, 256, 0, stream()>>>(D.G(0, n_img), lists0, pl.bw[0], nblocks, out_w, out_h, cov);
            check_launch("compact_norm_kernel");
            compact_multiband(pl, D, n_img, sigma, F);
            planar_finish_kernel<<<cdiv(P, 256), 256, 0, stream()>>>(F, cov, P, white, oP.get(), cov_out);
            check_launch("planar_finish_kernel");
        } else {
            if (blending == APS_BLEND_LINEAR)
                compact_fuse_kernel<APS_BLEND_LINEAR><<<pg, 256, 0, stream()>>>(D.G(0, n_img), lists0, pl.bw[0], nblocks, out_w, out_h, white, oP.get(), cov_out);
            else
                compact_fuse_kernel<APS_BLEND_NONE><<<pg, 256, 0, stream()>>>(D.G(0, n_img), lists0, pl.bw[0], nblocks, out_w, out_h, white, oP.get(), cov_out);
            check_launch("compact_fuse_kernel");
        }
        oP.commit();
        oC.commit();
        APS_HIP(hipStreamSynchronize(stream()));  // the staged inputs, tables and the workspace must outlive the launches
    });
}

int aps_planar_gain_stats_compact(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                                  const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int downsample,
                                  double* n_ij, double* sum_ci, double* sum_cj) {
    return guarded([&] {
        planar_check_args(images, img_h, img_w, img_c, n_img, H, out_h, out_w, sx, sy, kCompactGainMaxImages);
        APS_REQUIRE(n_ij && sum_ci && sum_cj, APS_E_ARG, "NULL argument");
        APS_REQUIRE(downsample >= 1, APS_E_ARG, "overlapDownsample must be >= 1");
        ctx();
        CompactPlan pl;
        compact_plan(n_img, img_h, img_w, H, out_h, out_w, x0, y0, sx, sy, 1, 0, true, pl);
        const size_t nn = (size_t)n_img * n_img;
        planar_precheck(compact_bytes(pl, n_img, img_h, img_w, img_c, out_h, out_w, APS_BLEND_NONE) + (int64_t)(7 * nn * sizeof(double)));
        CompactDevice D;
        compact_setup(pl, images, img_h, img_w, img_c, n_img, H, out_h, out_w, x0, y0, sx, sy, nullptr, D);
        Out<double> oN(n_ij, nn), oI(sum_ci, 3 * nn), oJ(sum_cj, 3 * nn);
        APS_HIP(hipMemsetAsync(oN.get(), 0, nn * sizeof(double), stream()));
        APS_HIP(hipMemsetAsync(oI.get(), 0, 3 * nn * sizeof(double), stream()));
        APS_HIP(hipMemsetAsync(oJ.get(), 0, 3 * nn * sizeof(double), stream()));
        const int ws = (out_w - 1) / downsample + 1, hs = (out_h - 1) / downsample + 1;  // numel(1:ds:end)
        {
            Prof prof("planar_gain_stats_compact");
            compact_gain_stats_kernel<<<dim3(cdiv(ws, 16), cdiv(hs, 16)), 256, 0, stream()>>>(
                D.G(0, n_img), D.lists.get() + pl.list_off[0], pl.bw[0], pl.bw[0] * pl.bh[0], n_img, downsample, ws, hs, oN.get(), oI.get(),
                oJ.get());
        }
        check_launch("compact_gain_stats_kernel");
        oN.commit();
        oI.commit();
        oJ.commit();
        APS_HIP(hipStreamSynchronize(stream()));
    });
}

}  // extern "C"
