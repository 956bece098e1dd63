// render_dev.h — device-side structures and sampling functions shared by render.hip (per-tile reference path,
// linear/none blending, diagnostics), render_batch.hip (the batched multiband path) and planar.hip (the planar compositors),
// and the one statement of the multiband pyramid's arithmetic (resize_with, blur_tile, lap_accumulate) and shape
// (pyramid_levels, next_footprint, pyramid_footprints), and of the cover pass's column shift (cover_xshift).  See render.hip's
// header comment for the reference lines restated here.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

#include "aps_internal.h"

namespace aps {

// ------------------------------------------------------------------------------------------------
// device-side descriptors
// ------------------------------------------------------------------------------------------------
struct DevImage {
    const uint32_t* rgba;  // h*w words
    const float* wx;       // tent LUT, w entries
    const float* wy;       // tent LUT, h entries
    int h, w;
    float R[9];  // column-major, single(cam.R)
    float fx, fy, cx, cy;
    float gain[3];
    float g255[3];  // gain / 255: byte -> [0,1] and the gain in one factor (the fast sampler of the batched path)
    float tx[2], ty[2];  // the tent weight as min(p * t[0], (n - 1 - p) * t[1], 1), p = 0-based position (warpWeights in closed form)
    float cmin;  // cos of the largest angle between the optical axis and a ray that hits the pixel rectangle (minus a margin)
};

struct DevCanvas {
    int mode, H, W;
    float f, o0, o1;
    float Rref[9];
};

// The ray generators of the projections that are not in the reference ("Projection contract"); canvas_ray, gain_ray
// (render.hip) and row_trig (render_batch.hip) all come here, so each operation order is stated once.
// Miller: the elevation at canvas height b.
__device__ __forceinline__ float miller_elevation(float b) { return 1.25f * atanf(sinhf(0.8f * b)); }
// Fisheye / Panini: the ray at (a, b) in the reference frame, not normalised.  A fisheye pixel further than pi from the axis
// looks at nothing: the zero vector, which stays zero through R_ref and the normalisation and which project() refuses.
// A real function, result in registers: inlined, its sinf / cosf raised the register count of rw_warp_staged_kernel for
// every mode (73 -> 78 VGPRs); called, the kernels of the other modes keep their registers (DESIGN.md has the table).
struct Ray3 {
    float v[3];
};
inline __device__ __noinline__ Ray3 wide_ray(int mode, float a, float b) {
    Ray3 ray;
    float* r = ray.v;
    if (mode == APS_PROJ_FISHEYE) {
        const float rad = sqrtf(a * a + b * b);
        const float s = rad > 1e-6f ? sinf(rad) / rad : 1.0f;
        const bool seen = !(rad > 3.14159265f);
        r[0] = seen ? s * a : 0.0f;
        r[1] = seen ? s * b : 0.0f;
        r[2] = seen ? cosf(rad) : 0.0f;
    } else {  // APS_PROJ_PANINI
        r[0] = a;
        r[1] = b;
        r[2] = 1.0f - 0.25f * a * a;
    }
    return ray;
}

// NEW = false: the four modes of the reference only, the code the kernels had before the other projections came (the hot
// warp kernels of render_batch.hip are instantiated per mode family, so that those modes run the instructions they ran).
template <bool NEW = true>
__device__ __forceinline__ void canvas_ray(const DevCanvas& cv, float xp, float yp, float d[3]) {
    float x, y, z;
    if (cv.mode == APS_PROJ_CYLINDRICAL) {
        const float th = cv.o0 + xp / cv.f, hl = cv.o1 + yp / cv.f;
        x = sinf(th);
        y = hl;
        z = cosf(th);
    } else if (cv.mode == APS_PROJ_SPHERICAL) {
        const float th = cv.o0 + xp / cv.f, ph = cv.o1 + yp / cv.f;
        const float cp = cosf(ph), sp = sinf(ph);
        x = cp * sinf(th);
        y = sp;
        z = cp * cosf(th);
    } else if (NEW && cv.mode == APS_PROJ_MILLER) {
        const float th = cv.o0 + xp / cv.f, ph = miller_elevation(cv.o1 + yp / cv.f);
        const float cp = cosf(ph), sp = sinf(ph);
        x = cp * sinf(th);
        y = sp;
        z = cp * cosf(th);
    } else {
        float rx, ry, rz;
        if (cv.mode == APS_PROJ_PLANAR) {
            rx = cv.o0 + xp / cv.f;
            ry = cv.o1 + yp / cv.f;
            rz = 1.0f;
        } else if (!NEW || cv.mode == APS_PROJ_STEREOGRAPHIC) {
            const float a = cv.o0 + xp / cv.f, b = cv.o1 + yp / cv.f;
            const float r2 = a * a + b * b, den = 1.0f + r2;
            rx = 2.0f * a / den;
            ry = 2.0f * b / den;
            rz = (1.0f - r2) / den;
        } else {
            const Ray3 r = wide_ray(cv.mode, cv.o0 + xp / cv.f, cv.o1 + yp / cv.f);
            rx = r.v[0];
            ry = r.v[1];
            rz = r.v[2];
        }
        x = (cv.Rref[0] * rx + cv.Rref[1] * ry) + cv.Rref[2] * rz;
        y = (cv.Rref[3] * rx + cv.Rref[4] * ry) + cv.Rref[5] * rz;
        z = (cv.Rref[6] * rx + cv.Rref[7] * ry) + cv.Rref[8] * rz;
    }
    float n = sqrtf((x * x + y * y) + z * z);
    if (!(n > 1e-8f)) n = 1e-8f;
    d[0] = x / n;
    d[1] = y / n;
    d[2] = z / n;
}

struct Sample {
    float s[3];
    float wang, wf;
    bool m;
};

// Geometry only: (u, v, Wang, inside&front).  Used by the coverage prepass and by the sampler.
__device__ __forceinline__ bool project(const DevImage& im, const float d[3], float angle_pow,
                                        float& u, float& v, float& wa) {
    float cam[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) cam[c] = fmaf(d[2], im.R[c + 6], fmaf(d[1], im.R[c + 3], d[0] * im.R[c]));
    const float epsz = 1e-6f;
    const bool front = cam[2] > epsz;
    const float cz = cam[2] > epsz ? cam[2] : epsz;
    u = im.fx * (cam[0] / cz) + im.cx;
    v = im.fy * (cam[1] / cz) + im.cy;
    wa = cam[2] > 0.0f ? cam[2] : 0.0f;
    if (angle_pow == 2.0f)
        wa = wa * wa;
    else if (angle_pow != 1.0f)
        wa = powf(wa, angle_pow);
    wa = front ? wa : 0.0f;
    if (!isfinite(u) || !isfinite(v)) {
        u = 1.0f;
        v = 1.0f;
    }
    const bool inside = (u >= 1.0f) && (u <= (float)im.w) && (v >= 1.0f) && (v <= (float)im.h);
    return inside && wa > 0.0f;
}

__device__ __forceinline__ Sample sample_one(const DevImage& im, const float d[3], float angle_pow) {
    Sample r;
    float u, v, wa;
    r.m = project(im, d, angle_pow, u, v, wa);
    if (r.m) {
        const int w = im.w, h = im.h;
        int x0 = (int)floorf(u), y0 = (int)floorf(v);
        x0 = max(1, min(x0, w - 1));
        y0 = max(1, min(y0, h - 1));
        const int x1 = min(x0 + 1, w), y1 = min(y0 + 1, h);
        const float s = u - (float)x0, t = v - (float)y0;
        const uint32_t p00 = im.rgba[(size_t)(y0 - 1) * w + (x0 - 1)];
        const uint32_t p10 = im.rgba[(size_t)(y0 - 1) * w + (x1 - 1)];
        const uint32_t p01 = im.rgba[(size_t)(y1 - 1) * w + (x0 - 1)];
        const uint32_t p11 = im.rgba[(size_t)(y1 - 1) * w + (x1 - 1)];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g = im.gain[c];
            const float v00 = ((float)((p00 >> (8 * c)) & 255u) / 255.0f) * g;
            const float v10 = ((float)((p10 >> (8 * c)) & 255u) / 255.0f) * g;
            const float v01 = ((float)((p01 >> (8 * c)) & 255u) / 255.0f) * g;
            const float v11 = ((float)((p11 >> (8 * c)) & 255u) / 255.0f) * g;
            const float top = (1.0f - s) * v00 + s * v10;
            const float bot = (1.0f - s) * v01 + s * v11;
            r.s[c] = top * (1.0f - t) + bot * t;
        }
        const float wy0 = im.wy[y0 - 1], wy1 = im.wy[y1 - 1], wx0 = im.wx[x0 - 1], wx1 = im.wx[x1 - 1];
        const float f00 = wy0 * wx0, f10 = wy0 * wx1, f01 = wy1 * wx0, f11 = wy1 * wx1;
        const float top = (1.0f - s) * f00 + s * f10;
        const float bot = (1.0f - s) * f01 + s * f11;
        r.wf = top * (1.0f - t) + bot * t;
        r.wang = wa;
    } else {
        r.s[0] = r.s[1] = r.s[2] = 0.0f;
        r.wf = 0.0f;
        r.wang = 0.0f;
    }
    return r;
}

// Footprint of a layer inside its tile, half-open [x0,x1) x [y0,y1).  A layer is EXACTLY zero (colour and
// weight) outside its rect, at every pyramid level (the rect grows by the filter radius per blur and is
// mapped through the resize taps per level), so kernels neither store nor load there: a load outside the
// rect is replaced by 0, which is the value the full-tile computation would have read.  Results are the
// same bits as processing full tiles; the traffic is that of the footprints.
struct Rect {
    int x0, y0, x1, y1;
};
constexpr int kMaxK = 16;  // layers per kernel-argument table
struct RectTab {
    Rect r[kMaxK];
};
__device__ __forceinline__ bool in_rect(const Rect& r, int x, int y) {
    return x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1;
}
__device__ __forceinline__ float4 ld_rect(const float4* __restrict__ p, int w, const Rect& r, int x, int y) {
    return in_rect(r, x, y) ? p[(size_t)y * w + x] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------------------------------------
// pyramid building blocks on float4 images
// ------------------------------------------------------------------------------------------------
struct Taps {
    float k[17];
    int r;
};

__device__ __forceinline__ float4 fma4(float w, const float4 v, float4 a) {
    a.x = fmaf(w, v.x, a.x);
    a.y = fmaf(w, v.y, a.y);
    a.z = fmaf(w, v.z, a.z);
    a.w = fmaf(w, v.w, a.w);
    return a;
}

// imresize contributions (triangle kernel) for output index x (0-based); all in f64 like MATLAB
__device__ __forceinline__ int resize_taps(int in_len, int out_len, int x, int& left, float wts[12]) {
    const double scale = (double)out_len / (double)in_len;
    const double kw = scale < 1.0 ? 2.0 / scale : 2.0;
    const double u = (double)(x + 1) / scale + 0.5 * (1.0 - 1.0 / scale);
    left = (int)floor(u - kw / 2.0);
    int P = (int)ceil(kw) + 2;
    if (P > 12) P = 12;  // scale >= 0.2 always holds for floor(/2) pyramids (scale in [1/3, 1/2] or >= 2)
    double wd[12], s = 0;
    for (int t = 0; t < P; ++t) {
        const double dx = u - (double)(left + t);
        double a = scale < 1.0 ? scale * dx : dx;
        a = fabs(a);
        double v = a < 1.0 ? 1.0 - a : 0.0;
        if (scale < 1.0) v = scale * v;
        wd[t] = v;
        s += v;
    }
    for (int t = 0; t < P; ++t) wts[t] = (float)(wd[t] / s);
    return P;
}

// imresize for one output pixel, both passes, with the load left to the caller: ld(x, y) returns the input pixel (zero outside a
// footprint, a patch in LDS, a plain image).  Per second-pass tap the first-pass result at that intermediate position is an fmaf
// chain over the first-pass taps; the intermediate value depends only on its own position, so this equals materialising the
// intermediate image.  ROWS_FIRST = the reference's rule (smaller scale factor first, ties -> rows).  Every resize of the
// multiband pyramids, dense or compact, down or up, is this one function.
template <bool ROWS_FIRST, class Ld>
__device__ __forceinline__ float4 resize_with(const Ld& ld, int h, int w, int Pr, int lr, const float* wr, int Pc, int lc,
                                              const float* wc) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ROWS_FIRST) {  // pass 1 resizes rows (at full width), pass 2 resizes columns
        for (int tc = 0; tc < Pc; ++tc) {
            if (wc[tc] == 0.f) continue;  // a zero tap adds 0 * v: nothing (finite data)
            const int xx = min(max(lc + tc, 1), w) - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int tr = 0; tr < Pr; ++tr)
                if (wr[tr] != 0.f) v = fma4(wr[tr], ld(xx, min(max(lr + tr, 1), h) - 1), v);
            a = fma4(wc[tc], v, a);
        }
    } else {
        for (int tr = 0; tr < Pr; ++tr) {
            if (wr[tr] == 0.f) continue;  // a zero tap adds 0 * v: nothing (finite data)
            const int yy = min(max(lr + tr, 1), h) - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int tc = 0; tc < Pc; ++tc)
                if (wc[tc] != 0.f) v = fma4(wc[tc], ld(min(max(lc + tc, 1), w) - 1, yy), v);
            a = fma4(wr[tr], v, a);
        }
    }
    return a;
}

// imgaussfilt of one kBlurW x kBlurH output tile of the rectangle `orc` (tile blockIdx.x, blockIdx.y; 256 threads): haloed tile into
// LDS with replicate padding at the h x w level's border, column (vertical) pass, then row pass.  ld(x, y) returns an input
// pixel, st(x, y, v) stores an output pixel: where a layer lives is the caller's business.
constexpr int kBlurW = 32, kBlurH = 16;
template <int R, class Ld, class St>
__device__ __forceinline__ void blur_tile(const Ld& ld, const St& st, const Rect& orc, int h, int w, const Taps& tp) {
    constexpr int IW = kBlurW + 2 * R, IH = kBlurH + 2 * R;
    const int x0 = orc.x0 + blockIdx.x * kBlurW, y0 = orc.y0 + blockIdx.y * kBlurH, tid = threadIdx.x;
    if (x0 >= orc.x1 || y0 >= orc.y1) return;  // the grid is sized for the largest output rect of the launch
    __shared__ float4 s_in[IH * IW];
    __shared__ float4 s_v[kBlurH * IW];
    for (int e = tid; e < IH * IW; e += 256) {
        const int ly = e / IW, lx = e - ly * IW;
        const int gy = min(max(y0 + ly - R, 0), h - 1), gx = min(max(x0 + lx - R, 0), w - 1);
        s_in[e] = ld(gx, gy);
    }
    __syncthreads();
    for (int e = tid; e < kBlurH * IW; e += 256) {  // vertical pass for every column of the haloed tile
        const int ly = e / IW, lx = e - ly * IW;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t <= 2 * R; ++t) a = fma4(tp.k[t], s_in[(ly + t) * IW + lx], a);
        s_v[e] = a;
    }
    __syncthreads();
    for (int e = tid; e < kBlurH * kBlurW; e += 256) {  // horizontal pass
        const int ly = e / kBlurW, lx = e - ly * kBlurW;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= orc.x1 || gy >= orc.y1) continue;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t <= 2 * R; ++t) a = fma4(tp.k[t], s_v[ly * IW + lx + t], a);
        st(gx, gy, a);
    }
}

// Level l of multiBandBlending.m:136-144 at pixel (x, y) of the h x w level, for the contributors of `walk` in ascending order:
//   acc += (G_k - imresize(D_k, size_l)) .* w_k,   D_k = the dh x dw next level,
// or, with has_d == 0, the coarsest level (:159): acc += G_k .* w_k.  acc carries in whatever the caller accumulated before.
// The walk offers n candidates; candidate i has the footprint rect(i), its value at (x, y) behind pixel(i) and the next level's
// loader d(i, xx, yy).  A layer whose footprint does not contain the pixel contributes (0 - u) * 0: skipped; the resize taps
// are computed when the first contributor needs them.
template <bool ROWS_FIRST, class Walk>
__device__ __forceinline__ void lap_accumulate(const Walk& walk, int has_d, int x, int y, int h, int w, int dh, int dw, float acc[3]) {
    if (!has_d) {
        for (int i = 0; i < walk.n; ++i) {
            if (!in_rect(walk.rect(i), x, y)) continue;
            const float4 g = *walk.pixel(i);
            acc[0] = acc[0] + g.x * g.w;
            acc[1] = acc[1] + g.y * g.w;
            acc[2] = acc[2] + g.z * g.w;
        }
        return;
    }
    int lr = 0, lc = 0, Pr = 0, Pc = 0;
    float wr[12], wc[12];
    bool have_taps = false;
    for (int i = 0; i < walk.n; ++i) {
        if (!in_rect(walk.rect(i), x, y)) continue;
        if (!have_taps) {
            Pr = resize_taps(dh, h, y, lr, wr);
            Pc = resize_taps(dw, w, x, lc, wc);
            have_taps = true;
        }
        const float4 u = resize_with<ROWS_FIRST>([&](int xx, int yy) { return walk.d(i, xx, yy); }, dh, dw, Pr, lr, wr, Pc, lc, wc);
        const float4 g = *walk.pixel(i);
        acc[0] = acc[0] + (g.x - u.x) * g.w;
        acc[1] = acc[1] + (g.y - u.y) * g.w;
        acc[2] = acc[2] + (g.z - u.z) * g.w;
    }
}

// ---- host-side helpers shared by both render translation units ------------------------------------
inline Taps make_taps(float sigma) {
    Taps tp;
    const int r = (int)std::ceil(2.0 * (double)sigma);
    APS_REQUIRE(r >= 0 && r <= 8, APS_E_ARG, "MBBsigma %g needs a %d-tap filter (max 17 supported)",
                (double)sigma, 2 * r + 1);
    double t[17], s = 0;
    for (int i = 0; i <= 2 * r; ++i) {
        const double x = (double)(i - r);
        t[i] = std::exp(-(x * x) / (2.0 * (double)sigma * (double)sigma));
        s += t[i];
    }
    for (int i = 0; i <= 2 * r; ++i) tp.k[i] = (float)(t[i] / s);
    tp.r = r;
    return tp;
}

inline bool rows_first(int h, int w, int oh, int ow) { return (double)oh / h <= (double)ow / w; }

inline Rect clip_rect(Rect r, int w, int h) {
    r.x0 = std::max(r.x0, 0);
    r.y0 = std::max(r.y0, 0);
    r.x1 = std::min(r.x1, w);
    r.y1 = std::min(r.y1, h);
    if (r.x1 <= r.x0 || r.y1 <= r.y0) r = Rect{0, 0, 0, 0};
    return r;
}
// Output pixels of imresize (in_len -> out_len, antialiased triangle of half-width max(1, 1/scale)) that can see
// the input interval [a, b): o in [a*s + 0.5*s - 1.5, (b-1)*s + 0.5*s + 0.5] for s < 1; padded by one more pixel.
inline void map_interval(int a, int b, int in_len, int out_len, int& oa, int& ob) {
    if (b <= a) {
        oa = ob = 0;
        return;
    }
    const double s = (double)out_len / in_len;
    const double half = s < 1.0 ? 1.0 : s;  // support in output pixels
    oa = (int)std::floor(a * s - half - 2.0);
    ob = (int)std::ceil(b * s + half + 2.0);
    oa = std::max(oa, 0);
    ob = std::min(ob, out_len);
    if (ob <= oa) oa = ob = 0;
}
inline Rect map_rect(const Rect& r, int h, int w, int oh, int ow) {
    Rect o;
    map_interval(r.x0, r.x1, w, ow, o.x0, o.x1);
    map_interval(r.y0, r.y1, h, oh, o.y0, o.y1);
    if (o.x1 <= o.x0 || o.y1 <= o.y0) o = Rect{0, 0, 0, 0};
    return o;
}

// ---- the shape of a multiband pyramid, derived from sizes and footprints alone ---------------------------------------------------
// Level count (multiBandBlending.m:98-109: at most floor(log2(min(h, w)))) and level sizes (floor halving, at least 1).
inline void pyramid_levels(int h, int w, int levels, std::vector<int>& lh, std::vector<int>& lw) {
    const int maxl = (int)std::floor(std::log2((double)std::min(h, w)));
    const int L = std::max(1, std::min(levels, maxl));
    lh.assign(L, h);
    lw.assign(L, w);
    for (int l = 1; l < L; ++l) {
        lh[l] = std::max(1, lh[l - 1] / 2);
        lw[l] = std::max(1, lw[l - 1] / 2);
    }
}
// One level's step of a footprint, G_(l+1) = map(clip(grow(G_l))): B_l = the blurred G_l (grown by the filter radius, clipped
// to the h x w level), G_(l+1) = B_l mapped through the resize to oh x ow.  An empty footprint stays empty.
inline Rect blurred_footprint(const Rect& g, int radius, int h, int w) {
    return g.x1 <= g.x0 ? g : clip_rect(Rect{g.x0 - radius, g.y0 - radius, g.x1 + radius, g.y1 + radius}, w, h);
}
inline Rect next_footprint(const Rect& g, int radius, int h, int w, int oh, int ow) {
    return g.x1 <= g.x0 ? g : map_rect(blurred_footprint(g, radius, h, w), h, w, oh, ow);
}
// Footprints per level from the level-0 footprints g0 (clipped to the level): G_l and B_l of every level.
inline void pyramid_footprints(const std::vector<Rect>& g0, int radius, const std::vector<int>& lh, const std::vector<int>& lw,
                               std::vector<std::vector<Rect>>& gr, std::vector<std::vector<Rect>>& br) {
    const int L = (int)lh.size();
    gr.assign(L, g0);
    br.assign(L, g0);
    for (int l = 0; l < L; ++l)
        for (size_t k = 0; k < g0.size(); ++k) {
            br[l][k] = blurred_footprint(gr[l][k], radius, lh[l], lw[l]);
            if (l + 1 < L) gr[l + 1][k] = next_footprint(gr[l][k], radius, lh[l], lw[l], lh[l + 1], lw[l + 1]);
        }
}
// The cover pass (cover_kernel / footprint_kernel in render.hip, their rw_ twins in render_batch.hip) records the block columns
// an image touches as bits of ONE 64-bit word per block row: bit (block column >> xshift).  A tile of more than 64 columns of
// 32-pixel blocks shares a bit between 2^xshift neighbouring columns: the smallest shift at which the last column's bit is <= 63.
inline int cover_xshift(int wt) {
    const int nbx = cdiv(wt, 32);
    int xs = 0;
    while ((nbx >> xs) > 64 || ((nbx - 1) >> xs) > 63) ++xs;
    return xs;
}
// Pixels of levels from..to-1.
inline int64_t pyramid_px(const std::vector<int>& lh, const std::vector<int>& lw, int from, int to) {
    int64_t px = 0;
    for (int l = from; l < to; ++l) px += (int64_t)lh[l] * lw[l];
    return px;
}
// Bytes of what every multiband composite holds beside its layers: F, the numerator pyramid (levels 0..L-1) and the collapse
// buffers (levels 1..L-2).
inline int64_t pyramid_result_bytes(const std::vector<int>& lh, const std::vector<int>& lw) {
    const int L = (int)lh.size();
    return 16 * (pyramid_px(lh, lw, 0, 1) + pyramid_px(lh, lw, 0, L) + pyramid_px(lh, lw, 1, L - 1));
}


// ---- the batched multiband path (render_batch.hip) ----------------------------------------------------
struct TileRect {
    int r0, c0, ht, wt;
};
// Renders the given tiles of the canvas with multiband blending, all tiles in one launch sequence.  dimgs: the
// prepared device image table, himgs its host copy (the analytic footprints read the cameras there).  pano/covered are DEVICE pointers.  Returns false when the configuration is outside
// what the batched kernels are built for (the caller then takes the per-tile path).
// need_images(used): called once, before the first kernel that samples pixels, with used[i] != 0 for every image that meets one
// of the tiles - the caller converts those images' pixels then (and no others).
using NeedImages = std::function<void(const std::vector<char>& used)>;
bool render_multiband_batched(const DevImage* dimgs, const DevImage* himgs, int n_img, const DevCanvas& cv, const aps_render_opts& o,
                              const std::vector<TileRect>& tiles, int out_layout, uint8_t* pano, uint8_t* covered,
                              const NeedImages& need_images);
bool render_fuse_batched(const DevImage* dimgs, const DevImage* himgs, int n_img, const DevCanvas& cv, const aps_render_opts& o,
                              const std::vector<TileRect>& tiles, int out_layout, uint8_t* pano, uint8_t* covered,
                              const NeedImages& need_images);

// ------------------------------------------------------------------------------------------------
// shared between render.hip and planar.hip
// ------------------------------------------------------------------------------------------------
struct HWarp {
    double A[9];  // adjugate of H/H(3,3)
    double det;
};
// (render.hip) adjugate and determinant of H / H(3,3), H f64 3x3 column-major
void make_hwarp(const double* H, HWarp& hw);
// (render.hip) multiBandBlending on K float4 layers with normalised weights, optional footprints; result in F (unclamped)
void multiband_device(const std::vector<float4*>& layers, const Rect* rects, int h, int w, int levels, float sigma, float4* F);
// (render.hip) the collapse (multiBandBlending.m:163-167): F_l = imresize(F_(l+1), size_l) + Num_l from the coarsest level down;
// num[l]: the numerator of level l (lh[l] x lw[l]); F_0 is written to F.  One level: the caller's numerator IS F.
void multiband_collapse(const std::vector<Ws<float4>>& num, const std::vector<int>& lh, const std::vector<int>& lw, float4* F);

constexpr int kGainSlots = 128;  // per-workgroup pair table
constexpr int kGainMaxCover = 16;

// The pair sums of one workgroup of both gain-statistics kernels: a small LDS hash table keyed by the image pair (the points
// of a 16 x 16 patch share a handful of pairs), flushed with one double atomicAdd per touched entry; a full table sends the
// contribution straight to memory.  Outputs are n x n (x 3) column-major, entry (i, j), i < j.
struct GainPairTable {
    unsigned int key[kGainSlots];
    unsigned int cnt[kGainSlots];
    double sum[kGainSlots][6];
    __device__ __forceinline__ void init() {
        for (int e = threadIdx.x; e < kGainSlots; e += blockDim.x) {
            key[e] = 0u;
            cnt[e] = 0u;
#pragma unroll
            for (int c = 0; c < 6; ++c) sum[e][c] = 0.0;
        }
        __syncthreads();
    }
    __device__ __forceinline__ void add(int n_img, int i, int j, const float* ci, const float* cj, double* __restrict__ Nij,
                                        double* __restrict__ sCi, double* __restrict__ sCj) {
        const unsigned int k = (unsigned int)(i * n_img + j) + 1u;
        unsigned int slot = (k * 2654435761u) >> 25;
        for (int probe = 0; probe < kGainSlots; ++probe) {
            const unsigned int old = atomicCAS(&key[slot], 0u, k);
            if (old == 0u || old == k) {
                atomicAdd(&cnt[slot], 1u);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    atomicAdd(&sum[slot][c], (double)ci[c]);
                    atomicAdd(&sum[slot][3 + c], (double)cj[c]);
                }
                return;
            }
            slot = (slot + 1) & (kGainSlots - 1);
        }
        const size_t nn = (size_t)n_img * n_img, e = (size_t)i + (size_t)n_img * j;  // table full: straight to memory
        atomicAdd(&Nij[e], 1.0);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            atomicAdd(&sCi[e + nn * c], (double)ci[c]);
            atomicAdd(&sCj[e + nn * c], (double)cj[c]);
        }
    }
    __device__ __forceinline__ void flush(int n_img, double* __restrict__ Nij, double* __restrict__ sCi, double* __restrict__ sCj) {
        __syncthreads();
        const size_t nn = (size_t)n_img * n_img;
        for (int e = threadIdx.x; e < kGainSlots; e += blockDim.x) {
            const unsigned int k = key[e];
            if (!k) continue;
            const int i = (int)((k - 1u) / (unsigned int)n_img), j = (int)((k - 1u) % (unsigned int)n_img);
            const size_t o = (size_t)i + (size_t)n_img * j;
            atomicAdd(&Nij[o], (double)cnt[e]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                atomicAdd(&sCi[o + nn * c], sum[e][c]);
                atomicAdd(&sCj[o + nn * c], sum[e][3 + c]);
            }
        }
    }
};

}  // namespace aps
