// integral_dev.h — rgb2gray's integer plane and the exact 32-bit integral image, shared by surf.hip and fast.hip (not part of the ABI).
// Every sum is an integer: the chain has one result whatever the order of its additions.
//   integral_rowscan_kernel   gray value per pixel (kept as a u8 plane if the caller wants it) + prefix sums along each row
//                             (workgroup per row, carried across 1024-px chunks)
//   integral_colscan_kernel   column prefix sums inside chunks of 64 rows, in place
//   integral_colcarry_kernel  adds the totals of the chunks above and writes the (h+1) x (w+1) integral image
// Every launch works on a group of 1 .. kGroupViews images of one shape: the view is the last grid dimension, and the view's
// image comes from a table of pointers, its scratch, integral image and gray plane from a pitch.
#pragma once
#include <hip/hip_runtime.h>

#include "aps_internal.h"

namespace aps {
namespace {

constexpr int kColChunk = 64;  // rows per chunk of the column scan
constexpr int kGroupViews = 16;  // views of one call (APS_SURF_MAX_VIEWS, APS_FAST_MAX_VIEWS)

// the images of a group, one device pointer per view (a kernel argument, by value)
struct ViewImgs {
    const uint8_t* p[kGroupViews];
};

// the caller's check: the whole image at full brightness has to fit the 32-bit sums
inline bool integral_fits(int height, int width) { return (uint64_t)height * (uint64_t)width * 255u < ((uint64_t)1 << 32); }

__device__ __forceinline__ uint32_t gray_at(const uint8_t* __restrict__ img, int h, int w, int c, int layout, int y, int x) {
    if (c == 1) return layout == APS_IMG_U8_HWC ? img[(size_t)y * w + x] : img[(size_t)x * h + y];
    uint8_t ch[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) ch[q] = layout == APS_IMG_U8_HWC ? img[((size_t)y * w + x) * 3 + q] : img[(size_t)q * h * w + (size_t)x * h + y];
    // rgb2gray's integer plane, exactly as sift.hip's gray_u8_kernel builds it
    const double d = 0.298936021293775 * ch[0] + 0.587043074451121 * ch[1] + 0.114020904255103 * ch[2];
    return (uint32_t)(uint8_t)(float)floor(d + 0.5);
}

// T[y][x] = sum of gray[y][0..x]: one workgroup per row, 4 pixels per thread and pass, the running total carried from pass to pass.
// gray, if not NULL, receives the h x w row-major gray plane itself.
__global__ __launch_bounds__(256) void integral_rowscan_kernel(const ViewImgs imgs, int h, int w, int c, int layout,
                                                               uint32_t* __restrict__ T, size_t t_pitch, uint8_t* __restrict__ gray,
                                                               size_t gray_pitch) {
    __shared__ uint32_t s_tot[2][4];
    const int y = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* __restrict__ img = imgs.p[blockIdx.y];
    T += blockIdx.y * t_pitch;
    if (gray) gray += blockIdx.y * gray_pitch;
    uint32_t carry = 0;
    int it = 0;
    for (int x0 = 0; x0 < w; x0 += 1024, ++it) {
        const int xb = x0 + tid * 4;
        uint32_t g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = xb + k < w ? gray_at(img, h, w, c, layout, y, xb + k) : 0u;
        if (gray) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (xb + k < w) gray[(size_t)y * w + xb + k] = (uint8_t)g[k];
        }
        g[1] += g[0];
        g[2] += g[1];
        g[3] += g[2];
        uint32_t incl = g[3];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (lane == 63) s_tot[it & 1][wave] = incl;
        __syncthreads();  // (the slot of pass it is written again in pass it + 2, behind the barrier of pass it + 1)
        uint32_t base = carry + (incl - g[3]), tot = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t t = s_tot[it & 1][q];
            if (q < wave) base += t;
            tot += t;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (xb + k < w) T[(size_t)y * w + xb + k] = base + g[k];
        carry += tot;
    }
}

// Column prefix sums inside each chunk of kColChunk rows, in place.
__global__ __launch_bounds__(256) void integral_colscan_kernel(uint32_t* __restrict__ T, size_t t_pitch, int h, int w) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    T += blockIdx.z * t_pitch;
    const int y0 = blockIdx.y * kColChunk, y1 = min(h, y0 + kColChunk);
    uint32_t acc = 0;
    for (int y = y0; y < y1; ++y) {
        acc += T[(size_t)y * w + x];
        T[(size_t)y * w + x] = acc;
    }
}

// I[y+1][x+1] = T[y][x] + the last rows of the chunks above; column 0 of I and, by the first chunk, row 0 are written here.
__global__ __launch_bounds__(256) void integral_colcarry_kernel(const uint32_t* __restrict__ T, size_t t_pitch, int h, int w,
                                                                uint32_t* __restrict__ I, size_t i_pitch) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    T += blockIdx.z * t_pitch;
    I += blockIdx.z * i_pitch;
    if (blockIdx.y == 0) {
        I[x + 1] = 0u;
        if (x == 0) I[0] = 0u;
    }
    const int y0 = blockIdx.y * kColChunk, y1 = min(h, y0 + kColChunk);
    uint32_t carry = 0;
    for (int k = 0; k < (int)blockIdx.y; ++k) carry += T[(size_t)(k * kColChunk + kColChunk - 1) * w + x];
    const size_t ws = (size_t)w + 1;
    for (int y = y0; y < y1; ++y) {
        I[(size_t)(y + 1) * ws + x + 1] = T[(size_t)y * w + x] + carry;
        if (x == 0) I[(size_t)(y + 1) * ws] = 0u;
    }
}

// The three launches on the calling thread's stream, for nv views: view v reads imgs.p[v], uses T + v * t_pitch (H x W scratch) and
// receives the (H+1) x (W+1) integral image at I + v * i_pitch and, with gray not NULL, the H x W gray plane at gray + v * gray_pitch.
inline void integral_image(const ViewImgs& imgs, int nv, int H, int W, int channels, int img_layout, uint32_t* T, size_t t_pitch,
                           uint32_t* I, size_t i_pitch, uint8_t* gray, size_t gray_pitch) {
    integral_rowscan_kernel<<<dim3(H, nv), 256, 0, stream()>>>(imgs, H, W, channels, img_layout, T, t_pitch, gray, gray_pitch);
    check_launch("integral_rowscan_kernel");
    const dim3 cg(cdiv(W, 256), cdiv(H, kColChunk), nv);
    integral_colscan_kernel<<<cg, 256, 0, stream()>>>(T, t_pitch, H, W);
    check_launch("integral_colscan_kernel");
    integral_colcarry_kernel<<<cg, 256, 0, stream()>>>(T, t_pitch, H, W, I, i_pitch);
    check_launch("integral_colcarry_kernel");
}

// Sum of gray over rows r0..r1, columns c0..c1 (inclusive).  Wrapping u32 arithmetic: exact whenever the true value fits.
__device__ __forceinline__ uint32_t box(const uint32_t* __restrict__ I, size_t ws, int r0, int r1, int c0, int c1) {
    return I[(size_t)(r1 + 1) * ws + c1 + 1] - I[(size_t)r0 * ws + c1 + 1] - I[(size_t)(r1 + 1) * ws + c0] + I[(size_t)r0 * ws + c0];
}

}  // namespace
}  // namespace aps
