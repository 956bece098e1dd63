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
//
// Two compositors, one arithmetic.  The dense one (aps_planar_composite) keeps canvas-sized layers and walks images
// 0..K-1 at every pixel; the compact one (aps_planar_composite_compact) keeps footprint-sized layers and walks the
// contributor list of the pixel's 64 x 64 block.  They return the same bytes because every per-pixel computation has ONE
// source: the warp (planar_layer_pixel), normalisation, fusion and gain statistics (kernel templates over a layer set:
// DenseSet / CompactSet say who contributes to a pixel and where its value lives), and the pyramid (resize_with, blur_tile,
// lap_accumulate, multiband_collapse, pyramid_levels, pyramid_footprints in render_dev.h / render.hip).  The compositors
// differ in storage and contributor walk only; so do the two halves of the host side (DenseCompositor / CompactCompositor
// under planar_composite_impl and planar_gain_stats_impl).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <vector>

#include "render_dev.h"

namespace aps {

// The dense compositor's documented limit (include/aps.h; refusing the 65th image is tested behaviour): every pixel walks all
// K layers and memory is K canvases, so beyond it the compact compositor is the one to call.  No kernel depends on the number.
constexpr int kPlanarMaxImages = 64;

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

struct PlanarArgs {  // the leading arguments of the entry points (the byte formulas know no images, the dense one no H and no view)
    const uint8_t* const* images;
    const int *ih, *iw, *ic;
    int n;
    const double* H;
    int out_h, out_w;
    double x0, y0, sx, sy;
};

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

// Every image's footprint; APS_PLANAR_NO_CULL (a test switch) makes each one the whole canvas.
static std::vector<Rect> planar_footprints(const PlanarArgs& a) {
    const bool no_cull = std::getenv("APS_PLANAR_NO_CULL") != nullptr;
    std::vector<Rect> r(a.n);
    for (int k = 0; k < a.n; ++k)
        r[k] = no_cull ? Rect{0, 0, a.out_w, a.out_h}
                       : planar_footprint(a.H + 9 * k, a.ih[k], a.iw[k], a.out_h, a.out_w, a.x0, a.y0, a.sx, a.sy, nullptr);
    return r;
}

// What both byte formulas charge before the layers: sources, tents, the job table, coverage and the uint8 panorama.
static int64_t planar_io_bytes(const PlanarArgs& a) {
    const int64_t P = (int64_t)a.out_h * a.out_w;
    int64_t b = 0;
    for (int k = 0; k < a.n; ++k) b += (int64_t)a.ih[k] * a.iw[k] * a.ic[k] + 4 * ((int64_t)a.ih[k] + a.iw[k]);
    return b + (int64_t)a.n * (int64_t)sizeof(PlanarJob) + P + 3 * P;
}

// The device memory one composite requests (the formula of aps_planar_composite_bytes, include/aps.h).
static int64_t planar_bytes(const PlanarArgs& a, int blending, int levels) {
    const int64_t P = (int64_t)a.out_h * a.out_w, n = a.n;
    int64_t b = planar_io_bytes(a) + 16 * n * P;
    if (blending == APS_BLEND_MULTIBAND) {
        std::vector<int> lh, lw;
        pyramid_levels(a.out_h, a.out_w, levels, lh, lw);
        const int L = (int)lh.size();
        b += 16 * n * pyramid_px(lh, lw, 1, L);              // the layers' Gaussian levels 1..L-1
        if (L > 1) b += 16 * std::min<int64_t>(n, kMaxK) * P;  // blurred level of one batch of layers
        b += pyramid_result_bytes(lh, lw);
    }
    return b;
}

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// planar_layer_pixel: one canvas pixel of one image (planar_layer_kernel: one image per
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

// where a pixel lives in a layer stored inside its footprint r only: row-major, pitch = the footprint's width
__device__ __forceinline__ size_t c_index(const Rect& r, int x, int y) {
    return (size_t)(y - r.y0) * (size_t)(r.x1 - r.x0) + (size_t)(x - r.x0);
}

// COMPACT: the layer is stored inside its footprint only (row pitch = the footprint's width; W is not used); else at canvas pitch W.
template <bool COMPACT>
__global__ __launch_bounds__(256) void planar_layer_kernel(const PlanarJob* __restrict__ jobs, int k0, int W, double x0, double y0,
                                                           double sx, double sy) {
    const PlanarJob& j = jobs[k0 + blockIdx.z];
    const int x = j.r.x0 + blockIdx.x * 64 + (threadIdx.x & 63), y = j.r.y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= j.r.x1 || y >= j.r.y1) return;
    j.layer[COMPACT ? c_index(j.r, x, y) : (size_t)y * W + x] = planar_layer_pixel(j, x, y, x0, y0, sx, sy);
}

// ---- layer sets: who contributes to a canvas pixel, and where its value lives ----------------------------------------------------
// A set maps the launch's threads to pixels (thread_pixel) and offers, at a pixel, n candidates in ascending image order:
// image(i), its footprint rect(i) (a candidate counts only where in_rect holds) and the address pixel(i) of its value.
constexpr int kListBlock = 64, kListShift = 6;

struct CLayer {
    float4* p;  // the footprint's pixels, row-major, pitch r.x1 - r.x0
    Rect r;     // footprint at this level, clipped to the level
    int pad[2];
};
static_assert(sizeof(CLayer) == 32, "aps_planar_composite_compact_bytes counts 32 bytes per image and level table entry");

__device__ __forceinline__ float4 ld_compact(const CLayer& c, int x, int y) {
    return in_rect(c.r, x, y) ? c.p[c_index(c.r, x, y)] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Canvas-sized layers, all K images at every pixel; a 1-D grid over the npix = H * W pixels.
struct DenseSet {
    const PlanarJob* __restrict__ jobs;
    int K, W;
    size_t npix;
    struct At {
        const PlanarJob* __restrict__ jobs;
        size_t p;
        int n;
        __device__ __forceinline__ int image(int i) const { return i; }
        __device__ __forceinline__ const Rect& rect(int i) const { return jobs[i].r; }
        __device__ __forceinline__ float4* pixel(int i) const { return jobs[i].layer + p; }
    };
    __device__ __forceinline__ bool thread_pixel(int& x, int& y) const {
        const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
        y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
        return p < npix;
    }
    __device__ __forceinline__ At at(int x, int y) const { return At{jobs, (size_t)y * W + x, K}; }
};

// Footprint-sized layers (one level's table G) and the ascending contributor list of the pixel's 64 x 64 block; 64 x 4 pixels
// per workgroup, which therefore lies inside one block (blockIdx.x * 64 and blockIdx.y * 4 never straddle a multiple of 64):
// list bounds and entries are wave-uniform loads.  lists = start[nblocks + 1], then the entries.
struct CompactSet {
    const CLayer* __restrict__ G;
    const int* __restrict__ lists;
    int bw, nblocks, W, H;
    struct At {
        const CLayer* __restrict__ G;
        const int* __restrict__ idx;
        int n, x, y;
        __device__ __forceinline__ int image(int i) const { return idx[i]; }
        __device__ __forceinline__ const Rect& rect(int i) const { return G[idx[i]].r; }
        __device__ __forceinline__ float4* pixel(int i) const {
            const CLayer& c = G[idx[i]];
            return c.p + c_index(c.r, x, y);
        }
    };
    __device__ __forceinline__ bool thread_pixel(int& x, int& y) const {
        x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
        return x < W && y < H;
    }
    __device__ __forceinline__ At at(int x, int y) const {
        const int b = (y >> kListShift) * bw + (x >> kListShift);
        const int s = lists[b];
        return At{G, lists + nblocks + 1 + s, lists[b + 1] - s, x, y};
    }
};

// multiBandBlending.m:72-85 over the footprints (w = max(0,w) / sum where sum > 1e-8: the arithmetic of
// norm_weights_kernel, mbb_norm); coverage = any raw weight > 0, taken before the division can flush one to zero.
template <class Set>
__global__ __launch_bounds__(256) void planar_norm_kernel(Set set, uint8_t* __restrict__ cov) {
    int x, y;
    if (!set.thread_pixel(x, y)) return;
    const auto at = set.at(x, y);
    float s = 0.f;
    bool any = false;
    for (int i = 0; i < at.n; ++i) {
        if (!in_rect(at.rect(i), x, y)) continue;
        const float wv = at.pixel(i)->w;
        s = s + (wv > 0.f ? wv : 0.f);
        any |= wv > 0.f;
    }
    for (int i = 0; i < at.n; ++i) {
        if (!in_rect(at.rect(i), x, y)) continue;
        float4* q = at.pixel(i);
        const float w0 = q->w;
        const float wv = w0 > 0.f ? w0 : 0.f;
        q->w = s > 1e-8f ? wv / s : 0.f;
    }
    cov[(size_t)y * set.W + x] = any ? 1 : 0;
}

// APS_BLEND_MULTIBAND_MAXWEIGHT: the max-weight partition in planar_norm_kernel's place ("Max-weight multiband
// contract"): weight 1 for the first layer of maximal raw weight (> 0; `w > best` as planar_fuse_kernel<APS_BLEND_NONE>, so a
// NaN never owns), 0 for the others; coverage as planar_norm_kernel.
template <class Set>
__global__ __launch_bounds__(256) void planar_maxweight_kernel(Set set, uint8_t* __restrict__ cov) {
    int x, y;
    if (!set.thread_pixel(x, y)) return;
    const auto at = set.at(x, y);
    float best = 0.f;
    int owner = -1;
    for (int i = 0; i < at.n; ++i) {
        if (!in_rect(at.rect(i), x, y)) continue;
        const float wv = at.pixel(i)->w;
        if (wv > best) {
            best = wv;
            owner = i;
        }
    }
    for (int i = 0; i < at.n; ++i) {
        if (!in_rect(at.rect(i), x, y)) continue;
        at.pixel(i)->w = i == owner ? 1.0f : 0.0f;
    }
    cov[(size_t)y * set.W + x] = owner >= 0 ? 1 : 0;
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
template <int MODE, class Set>
__global__ __launch_bounds__(256) void planar_fuse_kernel(Set set, int white, uint8_t* __restrict__ pano, uint8_t* __restrict__ covered) {
    int x, y;
    if (!set.thread_pixel(x, y)) return;
    const auto at = set.at(x, y);
    float acc[3] = {0.f, 0.f, 0.f}, den = 0.f, best = 0.f;
    bool any = false;
    for (int i = 0; i < at.n; ++i) {
        if (!in_rect(at.rect(i), x, y)) continue;
        const float4 g = *at.pixel(i);
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
    planar_store(pano, covered, (size_t)y * set.W + x, any, white, acc[0], acc[1], acc[2]);
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
// pair whose footprints do not intersect is never valid together; the pairs of a point are pairs of its candidates).  One
// thread per sampled canvas point.
template <class Set>
__global__ __launch_bounds__(256) void planar_gain_stats_kernel(Set set, int n_img, int ds, int ws, int hs, double* __restrict__ Nij,
                                                                double* __restrict__ sCi, double* __restrict__ sCj) {
    __shared__ GainPairTable s_tab;
    s_tab.init();
    const int ix = blockIdx.x * 16 + (threadIdx.x & 15), iy = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (ix < ws && iy < hs) {
        const int x = ix * ds, y = iy * ds;
        const auto at = set.at(x, y);
        auto sample = [&](int i, float* c3) {
            if (!in_rect(at.rect(i), x, y)) return false;
            const float4 g = *at.pixel(i);
            c3[0] = g.x;
            c3[1] = g.y;
            c3[2] = g.z;
            return g.w > 0.f && isfinite(g.x) && isfinite(g.y) && isfinite(g.z);
        };
        for (int a = 0; a < at.n; ++a) {
            float ci[3];
            if (!sample(a, ci)) continue;
            for (int b = a + 1; b < at.n; ++b) {
                float cj[3];
                if (sample(b, cj)) s_tab.add(n_img, at.image(a), at.image(b), ci, cj, Nij, sCi, sCj);
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

// Shapes, canvas and homographies.  need_view = false: the dense byte formula, which knows sizes only.
static void planar_check_shapes(const PlanarArgs& a, int max_images, bool need_images = true, bool need_view = true) {
    APS_REQUIRE((a.images || !need_images) && a.ih && a.iw && a.ic && (a.H || !need_view), APS_E_ARG, "NULL argument");
    APS_REQUIRE(a.n >= 1, APS_E_ARG, "need at least one image (%d)", a.n);
    APS_REQUIRE(a.n <= max_images, APS_E_DIM, "more than %d images in one planar composite (%d)", max_images, a.n);
    APS_REQUIRE(a.out_h > 0 && a.out_w > 0 && (int64_t)a.out_h * a.out_w < ((int64_t)1 << 31), APS_E_DIM, "bad canvas size %d x %d",
                a.out_h, a.out_w);
    APS_REQUIRE(!need_view || (a.sx > 0 && a.sy > 0 && std::isfinite(a.sx) && std::isfinite(a.sy)), APS_E_ARG,
                "pixel extents must be positive");
    for (int k = 0; k < a.n; ++k) {
        APS_REQUIRE(!need_images || a.images[k], APS_E_ARG, "NULL image %d", k);
        APS_REQUIRE(a.ih[k] > 0 && a.iw[k] > 0 && (a.ic[k] == 1 || a.ic[k] == 3), APS_E_DIM, "image %d: bad size %d x %d x %d", k,
                    a.ih[k], a.iw[k], a.ic[k]);
        if (!need_view) continue;
        HWarp hw;
        make_hwarp(a.H + 9 * k, hw);
        // |det| against Hadamard's bound on it (rows and columns of H / H(3,3)): zero up to rounding = no inverse map
        const double* h = a.H + 9 * k;
        const double s = h[8] != 0 ? h[8] : 1.0;
        double rows = 1.0, cols = 1.0;
        bool fin = true;
        for (int i = 0; i < 3; ++i) {
            double r2 = 0, c2 = 0;
            for (int b = 0; b < 3; ++b) {
                fin = fin && std::isfinite(h[i + 3 * b]);
                r2 += (h[i + 3 * b] / s) * (h[i + 3 * b] / s);
                c2 += (h[b + 3 * i] / s) * (h[b + 3 * i] / s);
            }
            rows *= std::sqrt(r2);
            cols *= std::sqrt(c2);
        }
        APS_REQUIRE(fin && std::isfinite(hw.det) && std::fabs(hw.det) > 1e-14 * std::min(rows, cols), APS_E_ARG,
                    "homography %d is singular or not finite (det %g)", k, hw.det);
    }
}

// need_sigma = false: the byte formulas, which know no sigma.  Returns the mode the plans and byte formulas see:
// APS_BLEND_MULTIBAND_MAXWEIGHT differs from APS_BLEND_MULTIBAND in one kernel of planar_composite_impl only.
static int planar_check_blending(int blending, int levels, float sigma, bool need_sigma) {
    APS_REQUIRE(blending == APS_BLEND_NONE || blending == APS_BLEND_LINEAR || blending == APS_BLEND_MULTIBAND ||
                    blending == APS_BLEND_MULTIBAND_MAXWEIGHT,
                APS_E_ARG, "unknown blending mode %d", blending);
    if (blending == APS_BLEND_MULTIBAND_MAXWEIGHT) blending = APS_BLEND_MULTIBAND;
    if (blending == APS_BLEND_MULTIBAND) {
        APS_REQUIRE(levels >= 1, APS_E_ARG, "levels must be a positive integer");
        if (!need_sigma) return blending;
        APS_REQUIRE(sigma > 0, APS_E_ARG, "sigma must be positive");
        const Taps tp = make_taps(sigma);
        APS_REQUIRE(tp.r >= 1 && tp.r <= 4, APS_E_ARG, "pyrSigma %g needs a %d-tap filter; 3..9 taps are built", (double)sigma,
                    2 * tp.r + 1);
    }
    return blending;
}

// Refuses before the first launch when the request cannot fit (renderPanorama.m:245-266: "skip this panorama").
static void planar_precheck(int64_t need) {
    size_t free_b = 0, total_b = 0;
    APS_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t have = free_b + ws_idle_bytes();
    APS_REQUIRE((uint64_t)need <= (uint64_t)have, APS_E_OOM,
                "planar composite needs %lld bytes of device memory, %zu are free: this panorama cannot fit", (long long)need, have);
}

// Stages sources and tents, fills the job table and warps every image into its layer.  The caller has filled L.layers and
// L.rects: canvas-sized layers (compact = false) or the footprint-sized ones of the arena.
static void planar_build_layers(const PlanarArgs& a, const float* gains, bool compact, PlanarLayers& L) {
    const int n = a.n;
    size_t nt = 0;
    for (int k = 0; k < n; ++k) nt += (size_t)a.ih[k] + a.iw[k];
    std::vector<float>& tents = L.host_tents;
    tents.resize(nt);
    L.tents.alloc(nt);
    L.host_jobs.resize(n);
    size_t off = 0;
    for (int k = 0; k < n; ++k) {
        PlanarJob& j = L.host_jobs[k];
        L.imgs.emplace_back(new In<uint8_t>(a.images[k], (size_t)a.ih[k] * a.iw[k] * a.ic[k]));
        j.src = L.imgs.back()->get();
        planar_tent(a.iw[k], tents.data() + off);
        j.tx = L.tents.get() + off;
        off += a.iw[k];
        planar_tent(a.ih[k], tents.data() + off);
        j.ty = L.tents.get() + off;
        off += a.ih[k];
        j.layer = L.layers[k];
        HWarp hw;
        make_hwarp(a.H + 9 * k, hw);
        for (int e = 0; e < 9; ++e) j.A[e] = hw.A[e];
        j.det = hw.det;
        j.r = L.rects[k];
        j.h = a.ih[k], j.w = a.iw[k], j.c = a.ic[k];
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
        const dim3 grid(cdiv(mw, 64), cdiv(mh, 4), kc);
        if (compact)
            planar_layer_kernel<true><<<grid, 256, 0, stream()>>>(L.jobs.get(), k0, a.out_w, a.x0, a.y0, a.sx, a.sy);
        else
            planar_layer_kernel<false><<<grid, 256, 0, stream()>>>(L.jobs.get(), k0, a.out_w, a.x0, a.y0, a.sx, a.sy);
        check_launch("planar_layer_kernel");
    }
}

// The dense compositor's half of planar_composite_impl / planar_gain_stats_impl: one canvas-sized layer per image.
struct DenseCompositor {
    static constexpr int kMaxImages = kPlanarMaxImages, kGainMaxImages = kPlanarMaxImages;
    static constexpr const char *kNorm = "planar_norm_kernel", *kFuse = "planar_fuse_kernel", *kGain = "planar_gain_stats_kernel",
                                *kGainProf = "planar_gain_stats";
    const PlanarArgs& a;
    PlanarLayers L;
    size_t P() const { return (size_t)a.out_h * a.out_w; }
    // the statistics' outputs were never part of this formula
    void plan(int blending, int levels, float, int64_t) { planar_precheck(planar_bytes(a, blending, levels)); }
    void build(const float* gains) {
        L.rects = planar_footprints(a);
        L.store.resize(a.n);
        L.layers.resize(a.n);
        for (int k = 0; k < a.n; ++k) {
            L.store[k].alloc(P());
            L.layers[k] = L.store[k];
        }
        planar_build_layers(a, gains, false, L);
    }
    DenseSet set() const { return DenseSet{L.jobs.get(), a.n, a.out_w, P()}; }
    dim3 grid() const { return dim3(cdiv(P(), 256)); }
    void multiband(int levels, float sigma, float4* F) { multiband_device(L.layers, L.rects.data(), a.out_h, a.out_w, levels, sigma, F); }
};

// ------------------------------------------------------------------------------------------------
// the footprint-compact compositor (aps_planar_composite_compact, aps_planar_gain_stats_compact)
// ------------------------------------------------------------------------------------------------
// Same pixels, same arithmetic and same order of every sum as the dense compositor: the same bodies.  What changes is where a
// layer lives and who looks at it.
//   layers   : every image at every pyramid level is stored inside its footprint only (CLayer: base pointer, footprint,
//              row pitch = the footprint's width), all of them carved out of one arena.  No buffer multiplies the image
//              count by the canvas.
//   lists    : per level, the canvas is cut into 64 x 64 blocks; the host builds, from the footprints alone, the list of
//              images (ascending) whose footprint meets each block and uploads all lists once.  The per-pixel kernels walk the
//              list of their block (CompactSet) instead of all n jobs, and one pass per level accumulates every contributor.

// Everything the host derives from the shapes and homographies alone: level sizes and footprints (pyramid_levels,
// pyramid_footprints: the ones multiband_device derives), arena offsets, contributor lists.
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

// levels: as asked for (1 unless multiband); radius: the Gaussian's (make_taps(sigma).r); fill_lists = false only counts them
// (the byte formula needs no entries)
static void compact_plan(const PlanarArgs& a, int levels, int radius, bool fill_lists, CompactPlan& pl) {
    const int n = a.n;
    pyramid_levels(a.out_h, a.out_w, levels, pl.lh, pl.lw);
    const int L = pl.L = (int)pl.lh.size();
    pyramid_footprints(planar_footprints(a), radius, pl.lh, pl.lw, pl.gr, pl.br);
    pl.goff.assign(L, std::vector<int64_t>(n, 0));
    pl.boff.assign(L, std::vector<int64_t>(n, 0));
    auto area = [](const Rect& r) { return (int64_t)(r.x1 - r.x0) * (int64_t)(r.y1 - r.y0); };
    pl.layer_px = pl.blur_px = 0;
    for (int l = 0; l < L; ++l) {
        int64_t blur = 0;
        for (int k = 0; k < n; ++k) {
            if (l + 1 < L) {
                pl.boff[l][k] = blur;
                blur += area(pl.br[l][k]);
            }
            pl.goff[l][k] = pl.layer_px;
            pl.layer_px += area(pl.gr[l][k]);
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
static int64_t compact_bytes(const CompactPlan& pl, const PlanarArgs& a, int blending) {
    int64_t b = planar_io_bytes(a) + (int64_t)sizeof(CLayer) * a.n * (2 * pl.L - 1);
    b += 16 * pl.layer_px + 16 * pl.blur_px + 4 * pl.list_ints;
    if (blending == APS_BLEND_MULTIBAND) b += pyramid_result_bytes(pl.lh, pl.lw);
    return b;
}

// ---- pyramid kernels on compact layers: the bodies of render_dev.h with footprint-pitch loads and stores ---------------------------
// imgaussfilt: one image per blockIdx.z, input inside G's footprint, output inside B's
template <int R>
__global__ __launch_bounds__(256) void compact_blur_kernel(const CLayer* __restrict__ G, const CLayer* __restrict__ B, int k0, int h,
                                                           int w, Taps tp) {
    const CLayer in = G[k0 + blockIdx.z], out = B[k0 + blockIdx.z];
    blur_tile<R>([&](int x, int y) { return ld_compact(in, x, y); }, [&](int x, int y, float4 v) { out.p[c_index(out.r, x, y)] = v; },
                 out.r, h, w, tp);
}

// imresize: blurred level (B, h x w) -> next Gaussian level (D, oh x ow), one image per blockIdx.z
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
    out.p[c_index(out.r, x, y)] =
        resize_with<ROWS_FIRST>([&](int xx, int yy) { return ld_compact(in, xx, yy); }, h, w, Pr, lr, wr, Pc, lc, wc);
}

// The Laplacian numerator of one level over the block's contributors, every contributor in this one pass, from +0
// (lap_accumulate); 32 x 4 pixels per workgroup, inside one list block.
struct CompactWalk : CompactSet::At {
    const CLayer* __restrict__ D;  // the next level's table
    __device__ __forceinline__ float4 d(int i, int xx, int yy) const { return ld_compact(D[idx[i]], xx, yy); }
};
template <bool ROWS_FIRST>
__global__ __launch_bounds__(128) void compact_lap_kernel(CompactSet set, const CLayer* __restrict__ D, int has_d, int dh, int dw,
                                                          float4* __restrict__ num) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 4 + (threadIdx.x >> 5), h = set.H, w = set.W;
    if (x >= w || y >= h) return;
    float acc[3] = {0.f, 0.f, 0.f};
    lap_accumulate<ROWS_FIRST>(CompactWalk{set.at(x, y), D}, has_d, x, y, h, w, dh, dw, acc);
    num[(size_t)y * w + x] = make_float4(acc[0], acc[1], acc[2], 0.f);
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
    CompactSet set(const CompactPlan& pl, int l, int n) const {
        return CompactSet{G(l, n), lists.get() + pl.list_off[l], pl.bw[l], pl.bw[l] * pl.bh[l], pl.lw[l], pl.lh[l]};
    }
};

// Allocates the arena, uploads tables and lists, warps every image into its footprint (level 0).
static void compact_setup(const CompactPlan& pl, const PlanarArgs& a, const float* gains, CompactDevice& D) {
    const int L = pl.L, n = a.n;
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
    for (int k = 0; k < n; ++k) D.L.layers[k] = D.arena.get() + pl.goff[0][k];
    D.L.rects = pl.gr[0];
    planar_build_layers(a, gains, true, D.L);
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
                    const dim3 bg(cdiv(mw, kBlurW), cdiv(mh, kBlurH), kc);
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
        const dim3 lg(cdiv(wl, 32), cdiv(hl, 4));
        if (last || rows_first(nh, nw, hl, wl))
            compact_lap_kernel<true><<<lg, 128, 0, stream()>>>(D.set(pl, l, n), last ? G : D.G(l + 1, n), last ? 0 : 1, nh, nw, dst);
        else
            compact_lap_kernel<false><<<lg, 128, 0, stream()>>>(D.set(pl, l, n), D.G(l + 1, n), 1, nh, nw, dst);
        check_launch("compact_lap_kernel");
    }
    multiband_collapse(num, pl.lh, pl.lw, F);
}

constexpr int kCompactMaxImages = 0x7fffffff;  // what remains is the int32 range of tables and lists (compact_plan)
constexpr int kCompactRadius = 4;  // the byte formula charges every footprint as for the widest filter built (9 taps)
constexpr int kCompactGainMaxImages = 65535;  // GainPairTable keys a pair as i * n + j + 1 in 32 bits

// The compact compositor's half of planar_composite_impl / planar_gain_stats_impl.
struct CompactCompositor {
    static constexpr int kMaxImages = kCompactMaxImages, kGainMaxImages = kCompactGainMaxImages;
    static constexpr const char *kNorm = "compact_norm_kernel", *kFuse = "compact_fuse_kernel", *kGain = "compact_gain_stats_kernel",
                                *kGainProf = "planar_gain_stats_compact";
    const PlanarArgs& a;
    CompactPlan pl;
    CompactDevice D;
    // counts with the formula's radius, refuses what cannot fit, then plans with the call's own radius and fills the lists
    void plan(int blending, int levels, float sigma, int64_t stats_bytes) {
        const bool mb = blending == APS_BLEND_MULTIBAND;
        compact_plan(a, mb ? levels : 1, kCompactRadius, false, pl);
        planar_precheck(compact_bytes(pl, a, blending) + stats_bytes);
        compact_plan(a, mb ? levels : 1, mb ? make_taps(sigma).r : 0, true, pl);
    }
    void build(const float* gains) { compact_setup(pl, a, gains, D); }
    CompactSet set() const { return D.set(pl, 0, a.n); }
    dim3 grid() const { return dim3(cdiv(a.out_w, 64), cdiv(a.out_h, 4)); }
    void multiband(int, float sigma, float4* F) { compact_multiband(pl, D, a.n, sigma, F); }
};

// ------------------------------------------------------------------------------------------------
// the entry points' bodies, for either compositor
// ------------------------------------------------------------------------------------------------
template <class Compositor>
static void planar_composite_impl(const PlanarArgs& a, int blending, int levels, float sigma, int white_canvas, const float* gains,
                                  uint8_t* pano, uint8_t* covered) {
    planar_check_shapes(a, Compositor::kMaxImages);
    APS_REQUIRE(pano, APS_E_ARG, "NULL argument");
    const bool maxweight = blending == APS_BLEND_MULTIBAND_MAXWEIGHT;
    blending = planar_check_blending(blending, levels, sigma, true);
    ctx();
    Compositor c{a};
    c.plan(blending, levels, sigma, 0);
    const size_t P = (size_t)a.out_h * a.out_w;
    Out<uint8_t> oP(pano, 3 * P), oC(covered, P);
    c.build(gains);
    uint8_t* cov_out = oC.present() ? oC.get() : nullptr;
    const int white = white_canvas ? 1 : 0;
    const auto set = c.set();
    const dim3 grid = c.grid();
    if (blending == APS_BLEND_MULTIBAND) {
        Ws<uint8_t> cov(P);
        Ws<float4> F(P);
        if (maxweight)
            planar_maxweight_kernel<<<grid, 256, 0, stream()>>>(set, cov.get());
        else
            planar_norm_kernel<<<grid, 256, 0, stream()>>>(set, cov.get());
        check_launch(Compositor::kNorm);
        c.multiband(levels, sigma, F);
        planar_finish_kernel<<<cdiv(P, 256), 256, 0, stream()>>>(F, cov, P, white, oP.get(), cov_out);
        check_launch("planar_finish_kernel");
    } else {
        if (blending == APS_BLEND_LINEAR)
            planar_fuse_kernel<APS_BLEND_LINEAR><<<grid, 256, 0, stream()>>>(set, white, oP.get(), cov_out);
        else
            planar_fuse_kernel<APS_BLEND_NONE><<<grid, 256, 0, stream()>>>(set, white, oP.get(), cov_out);
        check_launch(Compositor::kFuse);
    }
    oP.commit();
    oC.commit();
    APS_HIP(hipStreamSynchronize(stream()));  // the staged inputs, tables and the workspace must outlive the launches
}

template <class Compositor>
static void planar_gain_stats_impl(const PlanarArgs& a, int downsample, double* n_ij, double* sum_ci, double* sum_cj) {
    planar_check_shapes(a, Compositor::kGainMaxImages);
    APS_REQUIRE(n_ij && sum_ci && sum_cj, APS_E_ARG, "NULL argument");
    APS_REQUIRE(downsample >= 1, APS_E_ARG, "overlapDownsample must be >= 1");
    ctx();
    const size_t nn = (size_t)a.n * a.n;
    Compositor c{a};
    c.plan(APS_BLEND_NONE, 1, 0.f, (int64_t)(7 * nn * sizeof(double)));
    c.build(nullptr);
    Out<double> oN(n_ij, nn), oI(sum_ci, 3 * nn), oJ(sum_cj, 3 * nn);
    APS_HIP(hipMemsetAsync(oN.get(), 0, nn * sizeof(double), stream()));
    APS_HIP(hipMemsetAsync(oI.get(), 0, 3 * nn * sizeof(double), stream()));
    APS_HIP(hipMemsetAsync(oJ.get(), 0, 3 * nn * sizeof(double), stream()));
    const int ws = (a.out_w - 1) / downsample + 1, hs = (a.out_h - 1) / downsample + 1;  // numel(1:ds:end)
    {
        Prof prof(Compositor::kGainProf);
        planar_gain_stats_kernel<<<dim3(cdiv(ws, 16), cdiv(hs, 16)), 256, 0, stream()>>>(c.set(), a.n, downsample, ws, hs, oN.get(),
                                                                                      oI.get(), oJ.get());
    }
    check_launch(Compositor::kGain);
    oN.commit();
    oI.commit();
    oJ.commit();
    APS_HIP(hipStreamSynchronize(stream()));
}

}  // namespace aps

using namespace aps;

extern "C" {

int64_t aps_planar_composite_bytes(int n_img, const int* img_h, const int* img_w, const int* img_c, int out_h, int out_w,
                                   int blending, int levels) {
    int64_t bytes = 0;
    const int st = guarded([&] {
        const PlanarArgs a{nullptr, img_h, img_w, img_c, n_img, nullptr, out_h, out_w, 0, 0, 1, 1};
        planar_check_shapes(a, kPlanarMaxImages, false, false);
        blending = planar_check_blending(blending, levels, 0.f, false);
        bytes = planar_bytes(a, blending, levels);
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
        planar_composite_impl<DenseCompositor>(PlanarArgs{images, img_h, img_w, img_c, n_img, H, out_h, out_w, x0, y0, sx, sy}, blending,
                                               levels, sigma, white_canvas, gains, pano, covered);
    });
}

int aps_planar_gain_stats(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                          const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int downsample,
                          double* n_ij, double* sum_ci, double* sum_cj) {
    return guarded([&] {
        planar_gain_stats_impl<DenseCompositor>(PlanarArgs{images, img_h, img_w, img_c, n_img, H, out_h, out_w, x0, y0, sx, sy}, downsample,
                                                n_ij, sum_ci, sum_cj);
    });
}

int64_t aps_planar_composite_compact_bytes(int n_img, const int* img_h, const int* img_w, const int* img_c, const double* H, int out_h,
                                           int out_w, double x0, double y0, double sx, double sy, int blending, int levels) {
    int64_t bytes = 0;
    const int st = guarded([&] {
        const PlanarArgs a{nullptr, img_h, img_w, img_c, n_img, H, out_h, out_w, x0, y0, sx, sy};
        planar_check_shapes(a, kCompactMaxImages, false);
        blending = planar_check_blending(blending, levels, 0.f, false);
        CompactPlan pl;
        compact_plan(a, blending == APS_BLEND_MULTIBAND ? levels : 1, kCompactRadius, false, pl);
        bytes = compact_bytes(pl, a, blending);
    });
    return st == APS_OK ? bytes : (int64_t)st;
}

int aps_planar_composite_compact(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                                 const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int blending,
                                 int levels, float sigma, int white_canvas, const float* gains, uint8_t* pano, uint8_t* covered) {
    return guarded([&] {
        planar_composite_impl<CompactCompositor>(PlanarArgs{images, img_h, img_w, img_c, n_img, H, out_h, out_w, x0, y0, sx, sy}, blending,
                                                 levels, sigma, white_canvas, gains, pano, covered);
    });
}

int aps_planar_gain_stats_compact(const uint8_t* const* images, const int* img_h, const int* img_w, const int* img_c, int n_img,
                                  const double* H, int out_h, int out_w, double x0, double y0, double sx, double sy, int downsample,
                                  double* n_ij, double* sum_ci, double* sum_cj) {
    return guarded([&] {
        planar_gain_stats_impl<CompactCompositor>(PlanarArgs{images, img_h, img_w, img_c, n_img, H, out_h, out_w, x0, y0, sx, sy},
                                                  downsample, n_ij, sum_ci, sum_cj);
    });
}

}  // extern "C"
