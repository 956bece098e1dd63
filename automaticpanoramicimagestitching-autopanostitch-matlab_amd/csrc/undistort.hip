// undistort.hip - lens distortion ("Lens distortion contract"): undistortImage and undistortPoints of the Computer
// Vision Toolbox for the polynomial model fx, fy, cx, cy, k1, k2, k3, p1, p2 (no skew), in the project's 1-based pixel frame.
// All arithmetic is f64, written exactly as the contract parenthesises it (the library is built -ffp-contract=off) and has no
// transcendentals, so tests/undistort_mirror.py restates both kernels bit for bit.
#include <cmath>

#include "aps_internal.h"

namespace aps {
namespace {

// rad, dx, dy of the forward (distorting) map at the normalised point (x, y)
struct LensTerms {
    double rad, dx, dy;
};
__device__ __forceinline__ LensTerms lens_terms(const aps_lens& L, double x, double y) {
    const double r2 = x * x + y * y;
    LensTerms t;
    t.rad = 1 + r2 * (L.k1 + r2 * (L.k2 + r2 * L.k3));
    t.dx = ((2 * L.p1) * x) * y + L.p2 * (r2 + (2 * x) * x);
    t.dy = L.p1 * (r2 + (2 * y) * y) + ((2 * L.p2) * x) * y;
    return t;
}

// ---- the image kernel ------------------------------------------------------------------------------------------------------------
// Output pixels are numbered in storage order (HWC: row by row; MATLAB: column by column within a plane) and lane t owns pixel t:
// neighbouring lanes read neighbouring texels (a wave's load of one tap spans 64 * C bytes of a source row when the map is
// smooth), the f64 chain runs once per pixel and the channels share it.  The stores of HWC storage are packed: the four lanes of
// a quad hold 4 * C bytes that start at a multiple of four bytes, each lane reads the other three pixels across the quad (DPP) and
// lane d < C of the quad stores dword d, so a wave stores 16 * C contiguous dwords and no single bytes.  A buffer that is not
// dword-aligned, the quad the image ends in, and MATLAB storage store bytes (there consecutive lanes are consecutive bytes of a
// plane).  Sizes are checked on the host: every byte offset fits 31 bits.
constexpr int kLanes = 256;

// lane b of every quad, to all four lanes of the quad (all lanes of the wave must be active)
template <int B>
__device__ __forceinline__ uint32_t quad_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, B * 0x55, 0xf, 0xf, false);  // quad_perm:[B,B,B,B]
}

template <int C, int LAYOUT>
__global__ __launch_bounds__(kLanes) void undistort_image_kernel(const uint8_t* __restrict__ in, int h, int w, aps_lens L, int identity,
                                                                 int out_h, int out_w, int x0, int y0, uint8_t fill, int packed,
                                                                 uint8_t* __restrict__ out) {
    constexpr bool HWC = LAYOUT == APS_IMG_U8_HWC;
    const unsigned int total = (unsigned int)out_h * (unsigned int)out_w;
    const unsigned int t = blockIdx.x * (unsigned int)kLanes + threadIdx.x;
    const bool inside = t < total;  // (no early return: the quad exchange below needs every lane)
    const unsigned int major = HWC ? (unsigned int)out_w : (unsigned int)out_h;  // pixels per storage line
    const unsigned int line = t / major, pos = t - line * major;
    const int i = HWC ? (int)line : (int)pos, j = HWC ? (int)pos : (int)line;
    uint32_t px = 0;  // channel c in bits 8c .. 8c + 7
#pragma unroll
    for (int c = 0; c < C; ++c) px |= (uint32_t)fill << (8 * c);
    if (inside) {
        const double u = (double)(x0 + j), v = (double)(y0 + i);
        double ud = u, vd = v;
        if (!identity) {
            const double x = (u - L.cx) / L.fx, y = (v - L.cy) / L.fy;
            const LensTerms m = lens_terms(L, x, y);
            ud = L.fx * (x * m.rad + m.dx) + L.cx;
            vd = L.fy * (y * m.rad + m.dy) + L.cy;
        }
        if (ud >= 1 && ud <= w && vd >= 1 && vd <= h) {  // (a NaN fails)
            const double fx1 = floor(ud), fy1 = floor(vd);
            const int x1 = (int)fx1, y1 = (int)fy1, x2 = min(x1 + 1, w), y2 = min(y1 + 1, h);
            const double wx = ud - fx1, wy = vd - fy1;
            const double w11 = (1 - wx) * (1 - wy), w12 = (1 - wx) * wy, w21 = wx * (1 - wy), w22 = wx * wy;
            px = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                // tap (row r, column q), 1-based, channel c
                auto tap = [&](int r, int q) -> double {
                    const size_t at = HWC ? ((size_t)(r - 1) * w + (q - 1)) * C + c : ((size_t)c * h * w + (size_t)(q - 1) * h) + (r - 1);
                    return (double)in[at];
                };
                const double p11 = tap(y1, x1), p12 = tap(y2, x1), p21 = tap(y1, x2), p22 = tap(y2, x2);
                const double s = ((w11 * p11 + w12 * p12) + w21 * p21) + w22 * p22;
                // round half away from zero, clamp to 0..255: the weights lie in [0, 1] and the taps are bytes, so s >= 0 and only
                // the upper clamp can act; s - trunc(s) is exact, so the tie test is too
                const double f = trunc(s);
                const double r = fmin(f + (s - f >= 0.5 ? 1.0 : 0.0), 255.0);
                px |= (uint32_t)(int)r << (8 * c);
            }
        }
    }
    if (HWC) {
        const uint32_t q0 = quad_lane<0>(px), q1 = quad_lane<1>(px), q2 = quad_lane<2>(px), q3 = quad_lane<3>(px);
        const unsigned int d = t & 3u, quad = t & ~3u;
        if (packed && quad + 4 <= total) {  // the quad's 4 * C bytes = C dwords at the byte offset quad * C, a multiple of 4
            if (d < (unsigned int)C) {
                uint32_t word;
                if (C == 1)
                    word = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
                else
                    word = d == 0 ? (q0 | (q1 << 24)) : d == 1 ? ((q1 >> 8) | (q2 << 16)) : ((q2 >> 16) | (q3 << 8));
                reinterpret_cast<uint32_t*>(out + (size_t)quad * C)[d] = word;
            }
            return;
        }
    }
    if (inside)
#pragma unroll
        for (int c = 0; c < C; ++c) out[HWC ? (size_t)t * C + c : (size_t)c * total + t] = (uint8_t)(px >> (8 * c));
}

// ---- the point kernel ------------------------------------------------------------------------------------------------------------
constexpr int kInverseSteps = 20;

__global__ __launch_bounds__(256) void undistort_points_kernel(const double* __restrict__ pts, int64_t n, int64_t ld, aps_lens L,
                                                               double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double xd = (pts[k] - L.cx) / L.fx, yd = (pts[ld + k] - L.cy) / L.fy;
    double x = xd, y = yd;
    for (int it = 0; it < kInverseSteps; ++it) {  // a fixed count, no convergence test: the mirror runs the same chain
        const LensTerms t = lens_terms(L, x, y);
        x = (xd - t.dx) / t.rad;
        y = (yd - t.dy) / t.rad;
    }
    out[k] = L.fx * x + L.cx;
    out[ld + k] = L.fy * y + L.cy;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
void check_lens(const aps_lens* lens) {
    APS_REQUIRE(lens, APS_E_ARG, "NULL argument");
    APS_REQUIRE(std::isfinite(lens->fx) && std::isfinite(lens->fy) && lens->fx > 0 && lens->fy > 0, APS_E_ARG,
                "fx and fy must be finite and above 0");
    for (double v : {lens->cx, lens->cy, lens->k1, lens->k2, lens->k3, lens->p1, lens->p2})
        APS_REQUIRE(std::isfinite(v), APS_E_ARG, "the principal point and the distortion coefficients must be finite");
}

bool is_identity(const aps_lens& L) { return L.k1 == 0 && L.k2 == 0 && L.k3 == 0 && L.p1 == 0 && L.p2 == 0; }

// n points of device memory (x at [k], y at [ld + k]) through the inverse map
void launch_points(const double* d_pts, int64_t n, int64_t ld, const aps_lens& lens, double* d_out) {
    undistort_points_kernel<<<cdiv((size_t)n, 256), 256, 0, stream()>>>(d_pts, n, ld, lens, d_out);
    check_launch("undistort_points_kernel");
}

template <int C, int LAYOUT>
void launch_image(const uint8_t* in, int h, int w, const aps_lens& lens, int out_h, int out_w, int x0, int y0, uint8_t fill,
                  uint8_t* out) {
    const size_t total = (size_t)out_h * out_w;
    const int packed = LAYOUT == APS_IMG_U8_HWC && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    undistort_image_kernel<C, LAYOUT><<<cdiv(total, kLanes), kLanes, 0, stream()>>>(
        in, h, w, lens, is_identity(lens) ? 1 : 0, out_h, out_w, x0, y0, fill, packed, out);
    check_launch("undistort_image_kernel");
}

}  // namespace
}  // namespace aps

using namespace aps;

extern "C" {

int aps_undistort_image_u8(const uint8_t* img, int h, int w, int c, int img_layout, const aps_lens* lens, int out_h, int out_w,
                           int x0, int y0, int fill, uint8_t* out) {
    return guarded([&] {
        APS_REQUIRE(img && out, APS_E_ARG, "NULL argument");
        check_lens(lens);
        APS_REQUIRE(h > 0 && w > 0 && out_h > 0 && out_w > 0, APS_E_DIM, "empty image");
        APS_REQUIRE((int64_t)h * w * 3 < (int64_t)1 << 31 && (int64_t)out_h * out_w * 3 < (int64_t)1 << 31, APS_E_DIM,
                    "images of 2^31 bytes or more are not built");
        APS_REQUIRE(c == 1 || c == 3, APS_E_DIM, "channels must be 1 or 3");
        APS_REQUIRE(img_layout == APS_IMG_U8_HWC || img_layout == APS_IMG_U8_MATLAB, APS_E_TYPE, "unknown image layout");
        APS_REQUIRE(fill >= 0 && fill <= 255, APS_E_ARG, "fill must be in 0..255");
        APS_REQUIRE(std::abs((int64_t)x0) < (1 << 24) && std::abs((int64_t)y0) < (1 << 24), APS_E_ARG, "origin out of range");
        ctx();
        In<uint8_t> di(img, (size_t)h * w * c);
        Out<uint8_t> dout(out, (size_t)out_h * out_w * c);
        const bool hwc = img_layout == APS_IMG_U8_HWC;
        auto go = c == 3 ? (hwc ? launch_image<3, APS_IMG_U8_HWC> : launch_image<3, APS_IMG_U8_MATLAB>)
                         : (hwc ? launch_image<1, APS_IMG_U8_HWC> : launch_image<1, APS_IMG_U8_MATLAB>);
        {
            Prof prof("undistort_image_u8");
            go(di, h, w, *lens, out_h, out_w, x0, y0, (uint8_t)fill, dout.get());
        }
        dout.commit();
        APS_HIP(hipStreamSynchronize(stream()));
    });
}

int aps_undistort_points(const double* pts, int64_t n, int64_t ld, const aps_lens* lens, double* out) {
    return guarded([&] {
        check_lens(lens);
        APS_REQUIRE(n >= 0 && n < (int64_t)1 << 31, APS_E_DIM, "n out of range");
        if (n == 0) return;
        APS_REQUIRE(pts && out, APS_E_ARG, "NULL argument");
        APS_REQUIRE(ld >= n, APS_E_DIM, "the leading dimension is below n");
        ctx();
        In<double> din(pts, (size_t)ld + n);
        Out<double> dout(out, (size_t)ld + n);
        launch_points(din, n, ld, *lens, dout.get());
        dout.commit_2d((size_t)n, 2, (size_t)ld);
        APS_HIP(hipStreamSynchronize(stream()));
    });
}

int aps_undistort_valid_view(int h, int w, const aps_lens* lens, int* x0, int* y0, int* out_h, int* out_w) {
    return guarded([&] {
        APS_REQUIRE(x0 && y0 && out_h && out_w, APS_E_ARG, "NULL argument");
        check_lens(lens);
        APS_REQUIRE(h > 0 && w > 0 && (int64_t)h * w < (int64_t)1 << 31, APS_E_DIM, "empty image");
        ctx();
        // the pixel centres of the border: top row, bottom row, left column, right column
        const size_t n = 2 * ((size_t)w + h);
        std::vector<double> p(2 * n), q(2 * n);
        size_t k = 0;
        for (int row : {1, h})
            for (int j = 1; j <= w; ++j, ++k) p[k] = j, p[n + k] = row;
        for (int col : {1, w})
            for (int i = 1; i <= h; ++i, ++k) p[k] = col, p[n + k] = i;
        In<double> din(p.data(), 2 * n);
        Out<double> dout(q.data(), 2 * n);
        launch_points(din, (int64_t)n, (int64_t)n, *lens, dout.get());
        dout.commit();
        const double *ux = q.data(), *uy = q.data() + n;
        double top = uy[0], bottom = uy[w], left = ux[2 * (size_t)w], right = ux[2 * (size_t)w + h];
        bool finite = true;
        for (size_t t = 0; t < n; ++t) finite = finite && std::isfinite(ux[t]) && std::isfinite(uy[t]);
        for (int j = 0; j < w; ++j) top = std::max(top, uy[j]), bottom = std::min(bottom, uy[(size_t)w + j]);
        for (int i = 0; i < h; ++i) left = std::max(left, ux[2 * (size_t)w + i]), right = std::min(right, ux[2 * (size_t)w + h + i]);
        APS_REQUIRE(finite && std::fabs(left) < (1 << 24) && std::fabs(right) < (1 << 24) && std::fabs(top) < (1 << 24) &&
                        std::fabs(bottom) < (1 << 24), APS_E_ARG, "the border does not map to a finite rectangle");
        const double ax = std::ceil(left), bx = std::floor(right), ay = std::ceil(top), by = std::floor(bottom);
        APS_REQUIRE(bx >= ax && by >= ay, APS_E_ARG, "the valid view is empty");
        *x0 = (int)ax;
        *y0 = (int)ay;
        *out_h = (int)(by - ay) + 1;
        *out_w = (int)(bx - ax) + 1;
    });
}

}  // extern "C"
