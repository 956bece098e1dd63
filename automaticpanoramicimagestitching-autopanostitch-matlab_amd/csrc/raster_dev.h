// raster_dev.h — the exact pixel-centre tests of the raster contracts ("Annotation contract" rule 3 and "Mark
// contract"), stated once for annotate.hip (polygon edges) and marks.hip (segments and rings).  Host and device.
//
// All values are lattice units (1/16 px).  Ranges for the segment test: end points |q| <= 2^24, pixel centres 16 * c <= 2^35
// for any int canvas, so differences stay below 2^36, and the dot and cross products of a difference with an edge vector
// (|D| components <= 2^25) stay below 2^62: inside int64.  The squares cross^2 and R^2 * (D.D) do NOT fit 64 bits (up to
// 2^124); they are compared as 128-bit products (high and low words), so nothing is ever truncated.  The end-point test
// squares a difference only after |Ax| <= R and |Ay| <= R have been checked.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace aps {

__host__ __device__ __forceinline__ uint64_t ann_mulhi(uint64_t x, uint64_t y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(x, y);
#else
    return (uint64_t)(((unsigned __int128)x * y) >> 64);
#endif
}

// |ax|^2 + |ay|^2 <= R^2 (squares taken only of values already known to be <= R)
__host__ __device__ __forceinline__ bool ann_disc(int64_t ax, int64_t ay, int64_t R) {
    if (ax < 0) ax = -ax;
    if (ay < 0) ay = -ay;
    if (ax > R || ay > R) return false;
    return ax * ax + ay * ay <= R * R;
}

// Exact: squared distance from (cx, cy) to the closed segment (x0, y0)-(x1, y1) <= R^2.  See the header for the ranges.
__host__ __device__ __forceinline__ bool ann_seg_hit(int64_t cx, int64_t cy, int64_t x0, int64_t y0, int64_t x1, int64_t y1,
                                                     int64_t R) {
    const int64_t Dx = x1 - x0, Dy = y1 - y0, Ax = cx - x0, Ay = cy - y0;
    const int64_t DD = Dx * Dx + Dy * Dy;
    const int64_t t = Ax * Dx + Ay * Dy;
    if (t <= 0) return ann_disc(Ax, Ay, R);  // before the start point, or a zero-length edge (a dot)
    if (t >= DD) return ann_disc(cx - x1, cy - y1, R);
    int64_t cr = Ax * Dy - Ay * Dx;
    if (cr < 0) cr = -cr;
    const uint64_t u = (uint64_t)cr, r2 = (uint64_t)(R * R), dd = (uint64_t)DD;
    const uint64_t lhi = ann_mulhi(u, u), llo = u * u, rhi = ann_mulhi(r2, dd), rlo = r2 * dd;
    return lhi < rhi || (lhi == rhi && llo <= rlo);
}

// Exact: lo^2 <= |A|^2 <= hi^2 for A = (ax, ay), with 0 <= lo <= hi < 2^17 (a ring of mean radius (lo + hi) / 2, or a disc when
// lo = 0).  The squares are taken only after |ax| <= hi and |ay| <= hi have been checked, so they stay below 2^35.
__host__ __device__ __forceinline__ bool ann_ring_hit(int64_t ax, int64_t ay, int64_t lo, int64_t hi) {
    if (ax < 0) ax = -ax;
    if (ay < 0) ay = -ay;
    if (ax > hi || ay > hi) return false;
    const int64_t d2 = ax * ax + ay * ay;
    return d2 >= lo * lo && d2 <= hi * hi;
}

}  // namespace aps
