// marks.hip — segments and rings on a resident image, and the side-by-side montage of two images, on gfx950.
//
// The drawing half of showMatchedFeatures(I1, I2, p1, p2, 'montage') as refineMatch uses it under input.showKeypointsPlot
// (PP/imageMatching/imageMatching.m:257-269): the two images side by side, lines between matched points, a circle on every
// point of image 1 and a plus on every point of image 2.  The toolbox call is closed; the raster rule is this project's own and
// is stated in DESIGN.md ("Mark contract"); tests/marks_mirror.py restates it in Python, byte for byte.
//
// Shape of the work, as in annotate.hip: drawing is sparse.  One copy brings the source to the destination (none in place).
// The host half tests validity, quantises to sixteenths of a pixel and bins every mark to the 64 x 64 pixel tiles it can touch
// (conservatively: the exact test in the kernel decides), then uploads one CSR list.  One workgroup runs per TOUCHED tile and
// walks its list in ascending order, however long it is; a lane owns 16 pixels of the tile, keeps what it painted in registers
// and stores each painted pixel once.  Marks are opaque, so no pixel is ever loaded.  Radius and colour come per item.
//
// Arithmetic: integers only.  The segment test and its ranges are raster_dev.h's.  A ring has Rq <= 2^16 and R <= 2^9, so both
// radii of its test stay below 2^17 and their squares, like those of a difference already known to be below them, below 2^35.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "aps_internal.h"
#include "raster_dev.h"

namespace aps {

constexpr int kMarkTile = 64;                // tile side in pixels
constexpr int kMarkMaxWidth = 64;            // largest line width
constexpr int64_t kMarkCoordMax = 1 << 20;   // |coordinate| bound of a valid mark, in pixels
constexpr double kMarkRadiusMax = 4096.0;    // largest ring radius, in pixels

// One entry of a tile's list, lattice units.  A segment: (a, b) -> (c, d).  A ring: centre (a, b), c = Rq, d unused.
// rgb = r | g << 8 | b << 16; R = 8 * line_width.
struct MarkItem {
    int32_t a, b, c, d;
    uint32_t rgb;
    uint16_t R, kind;
};

// One workgroup per touched tile; lane t owns column (t & 63) and the 16 rows (t >> 6) + 4 i of the tile.
__global__ __launch_bounds__(256) void mark_tiles_kernel(uint8_t* __restrict__ img, int64_t H, int64_t W,
                                                         const int32_t* __restrict__ tile_xy, const int32_t* __restrict__ tile_off,
                                                         const int32_t* __restrict__ item_idx, const MarkItem* __restrict__ items) {
    const int tile = blockIdx.x;
    const int64_t c = (int64_t)tile_xy[2 * tile] * kMarkTile + (threadIdx.x & 63) + 1;            // 1-based column
    const int64_t r_first = (int64_t)tile_xy[2 * tile + 1] * kMarkTile + (threadIdx.x >> 6) + 1;  // 1-based row of i = 0
    if (c > W || r_first > H) return;
    uint32_t px[16];
    uint32_t have = 0;  // bit i: px[i] holds the pixel's final-so-far colour
#pragma unroll
    for (int i = 0; i < 16; ++i) px[i] = 0;
    const int64_t cx = 16 * c;
    const int k_end = tile_off[tile + 1];
    for (int k = tile_off[tile]; k < k_end; ++k) {
        const MarkItem it = items[item_idx[k]];
        const int64_t R = it.R;
        if (it.kind == APS_MARK_SEGMENT) {
            const int64_t x0 = it.a, y0 = it.b, x1 = it.c, y1 = it.d;
            // a painted pixel lies within R of the segment's bounding box
            if (cx < (x0 < x1 ? x0 : x1) - R || cx > (x0 < x1 ? x1 : x0) + R) continue;
            const int64_t ylo = (y0 < y1 ? y0 : y1) - R, yhi = (y0 < y1 ? y1 : y0) + R;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t r = r_first + 4 * i;
                const int64_t cy = 16 * r;
                if (r <= H && cy >= ylo && cy <= yhi && ann_seg_hit(cx, cy, x0, y0, x1, y1, R)) {
                    px[i] = it.rgb;
                    have |= 1u << i;
                }
            }
        } else {
            const int64_t hi = (int64_t)it.c + R, lo = (int64_t)it.c > R ? (int64_t)it.c - R : 0;
            const int64_t ax = cx - it.a;
            if (ax < -hi || ax > hi) continue;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t r = r_first + 4 * i;
                if (r <= H && ann_ring_hit(ax, 16 * r - it.b, lo, hi)) {
                    px[i] = it.rgb;
                    have |= 1u << i;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if ((have >> i) & 1u) {
            const int64_t r = r_first + 4 * i;  // (bit i is only ever set for r <= H)
            uint8_t* q = img + ((r - 1) * W + (c - 1)) * 3;
            q[0] = (uint8_t)(px[i] & 255u);
            q[1] = (uint8_t)((px[i] >> 8) & 255u);
            q[2] = (uint8_t)((px[i] >> 16) & 255u);
        }
    }
}

// ---- the host half: validity, quantisation, binning ---------------------------------------------------------------------

// q(v) = floor(16 v + 0.5) in IEEE f64 (v finite, |v| <= 2^20: exact product, |q| <= 2^24)
static inline int64_t mark_quant(double v) { return (int64_t)std::floor(16.0 * v + 0.5); }

static inline bool mark_coord_ok(double v) { return std::isfinite(v) && std::fabs(v) <= (double)kMarkCoordMax; }

static inline int64_t mark_floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }  // b > 0
static inline int64_t mark_ceil_div(int64_t a, int64_t b) { return -mark_floor_div(-a, b); }

// Calls f(ty, tx_lo, tx_hi) for runs of tiles, ascending in ty, that together hold every pixel of the H x W canvas the item can
// paint (and maybe some it cannot).  Deterministic: the counting pass and the filling pass below see the same runs.
template <class F>
static void mark_tile_runs(const MarkItem& it, int64_t H, int64_t W, F&& f) {
    const int64_t R = it.R;
    // a tile's pixel centres lie within 504 lattice units of its centre along each axis: half diagonal < 713
    const int64_t tile_span = 16 * kMarkTile, tile_ctr = 16 + 8 * (kMarkTile - 1), tile_rad = 713;
    if (it.kind == APS_MARK_SEGMENT) {
        int64_t x0 = it.a, y0 = it.b, x1 = it.c, y1 = it.d;
        if (y0 > y1) {
            std::swap(x0, x1);
            std::swap(y0, y1);
        }
        // pixels (1-based) whose centre lies within R of the segment's bounding box, clipped to the canvas
        const int64_t c_lo = std::max<int64_t>(1, mark_ceil_div(std::min(x0, x1) - R, 16));
        const int64_t c_hi = std::min<int64_t>(W, mark_floor_div(std::max(x0, x1) + R, 16));
        const int64_t r_lo = std::max<int64_t>(1, mark_ceil_div(y0 - R, 16));
        const int64_t r_hi = std::min<int64_t>(H, mark_floor_div(y1 + R, 16));
        if (c_lo > c_hi || r_lo > r_hi) return;
        const int64_t Dx = x1 - x0, Dy = y1 - y0;  // Dy >= 0
        for (int64_t ty = (r_lo - 1) / kMarkTile; ty <= (r_hi - 1) / kMarkTile; ++ty) {
            // a pixel of this tile row within R of a point S of the segment has S.y inside the row's band grown by R, and its
            // x within R of S.x: the part of the segment inside that band, its x range grown by R
            const int64_t ya = std::max(y0, 16 * (ty * kMarkTile + 1) - R), yb = std::min(y1, 16 * (ty * kMarkTile + kMarkTile) + R);
            if (ya > yb) continue;
            int64_t xa, xb;
            if (Dy == 0) {
                xa = std::min(x0, x1);
                xb = std::max(x0, x1);
            } else {  // x at ya and at yb, rounded outwards ((y - y0) * Dx stays below 2^51)
                const int64_t na = (ya - y0) * Dx, nb = (yb - y0) * Dx;
                xa = x0 + std::min(mark_floor_div(na, Dy), mark_floor_div(nb, Dy));
                xb = x0 + std::max(mark_ceil_div(na, Dy), mark_ceil_div(nb, Dy));
            }
            const int64_t p_lo = std::max(c_lo, mark_ceil_div(xa - R, 16)), p_hi = std::min(c_hi, mark_floor_div(xb + R, 16));
            if (p_lo <= p_hi) f(ty, (p_lo - 1) / kMarkTile, (p_hi - 1) / kMarkTile);
        }
    } else {
        const int64_t px = it.a, py = it.b, hi = (int64_t)it.c + R, lo = (int64_t)it.c - R;
        const int64_t c_lo = std::max<int64_t>(1, mark_ceil_div(px - hi, 16)), c_hi = std::min<int64_t>(W, mark_floor_div(px + hi, 16));
        const int64_t r_lo = std::max<int64_t>(1, mark_ceil_div(py - hi, 16)), r_hi = std::min<int64_t>(H, mark_floor_div(py + hi, 16));
        if (c_lo > c_hi || r_lo > r_hi) return;
        const int64_t out = hi + tile_rad, in = lo - tile_rad;
        for (int64_t ty = (r_lo - 1) / kMarkTile; ty <= (r_hi - 1) / kMarkTile; ++ty) {
            int64_t run = -1;  // first tile of the open run
            const int64_t tx_end = (c_hi - 1) / kMarkTile;
            for (int64_t tx = (c_lo - 1) / kMarkTile; tx <= tx_end + 1; ++tx) {
                bool keep = false;
                if (tx <= tx_end) {
                    // the tile's centre lies within a tile of the ring's bounding box: |d| < 2^18, the squares inside int64
                    const int64_t dx = tx * tile_span + tile_ctr - px, dy = ty * tile_span + tile_ctr - py;
                    const int64_t d2 = dx * dx + dy * dy;
                    keep = d2 <= out * out && (in <= 0 || d2 >= in * in);
                }
                if (keep && run < 0) run = tx;
                if (!keep && run >= 0) {
                    f(ty, run, tx - 1);
                    run = -1;
                }
            }
        }
    }
}

struct MarkPlan {
    std::vector<MarkItem> items;
    std::vector<int32_t> tile_xy, tile_off, item_idx;
    int64_t n_drawn = 0;
};

static MarkPlan mark_plan(int64_t H, int64_t W, const aps_mark* marks, int64_t n) {
    MarkPlan P;
    for (int64_t k = 0; k < n; ++k) {
        const aps_mark& m = marks[k];
        MarkItem it{};
        if (!mark_coord_ok(m.x0) || !mark_coord_ok(m.y0)) continue;
        if (m.kind == APS_MARK_SEGMENT) {
            if (!mark_coord_ok(m.x1) || !mark_coord_ok(m.y1)) continue;
            it.c = (int32_t)mark_quant(m.x1);
            it.d = (int32_t)mark_quant(m.y1);
        } else {
            if (!(std::isfinite(m.x1) && m.x1 >= 0.0 && m.x1 <= kMarkRadiusMax)) continue;
            it.c = (int32_t)mark_quant(m.x1);
        }
        ++P.n_drawn;  // valid: drawn, if only clipped to nothing
        it.a = (int32_t)mark_quant(m.x0);
        it.b = (int32_t)mark_quant(m.y0);
        it.rgb = (uint32_t)m.rgb[0] | ((uint32_t)m.rgb[1] << 8) | ((uint32_t)m.rgb[2] << 16);
        it.R = (uint16_t)(8 * m.line_width);
        it.kind = (uint16_t)m.kind;
        bool touches = false;
        mark_tile_runs(it, H, W, [&](int64_t, int64_t, int64_t) { touches = true; });
        if (touches) P.items.push_back(it);
    }
    APS_REQUIRE(P.items.size() < (size_t)INT32_MAX, APS_E_ARG, "too many marks on the canvas (%zu)", P.items.size());
    if (P.items.empty()) return P;
    // counting pass: a difference array over the dense tile grid (one cell per 12 KB of canvas), then its running sum
    const int64_t ntx = (W + kMarkTile - 1) / kMarkTile, nty = (H + kMarkTile - 1) / kMarkTile;
    std::vector<int32_t> cell((size_t)(ntx * nty) + 1, 0);
    int64_t total = 0;
    for (const MarkItem& it : P.items)
        mark_tile_runs(it, H, W, [&](int64_t ty, int64_t a, int64_t b) {
            total += b - a + 1;
            APS_REQUIRE(total < (int64_t)INT32_MAX, APS_E_ARG, "the tile lists of these marks do not fit 32-bit indexing");
            ++cell[(size_t)(ty * ntx + a)];
            --cell[(size_t)(ty * ntx + b) + 1];
        });
    // cell[t] becomes the start of tile t's list (the cursor of the filling pass); touched tiles get their CSR entry
    int32_t count = 0, start = 0;
    for (int64_t t = 0; t < ntx * nty; ++t) {
        count += cell[(size_t)t];
        cell[(size_t)t] = start;
        if (count > 0) {
            P.tile_xy.push_back((int32_t)(t % ntx));
            P.tile_xy.push_back((int32_t)(t / ntx));
            P.tile_off.push_back(start);
        }
        start += count;
    }
    P.tile_off.push_back(start);
    // filling pass, in item order: inside a tile the items stay in ascending index
    P.item_idx.resize((size_t)total);
    for (size_t id = 0; id < P.items.size(); ++id)
        mark_tile_runs(P.items[id], H, W, [&](int64_t ty, int64_t a, int64_t b) {
            for (int64_t tx = a; tx <= b; ++tx) P.item_idx[(size_t)cell[(size_t)(ty * ntx + tx)]++] = (int32_t)id;
        });
    return P;
}

static inline bool ranges_overlap(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) { return a < b + nb && b < a + na; }

}  // namespace aps

using namespace aps;

extern "C" int aps_draw_marks(const uint8_t* src, int64_t h, int64_t w, const aps_mark* marks, int64_t n, uint8_t* dst,
                              int64_t* n_drawn) {
    return guarded([&] {
        APS_REQUIRE(src && dst, APS_E_ARG, "NULL argument");
        APS_REQUIRE(h >= 1 && w >= 1 && h <= INT32_MAX && w <= INT32_MAX, APS_E_ARG, "bad canvas size %lld x %lld", (long long)h,
                    (long long)w);
        APS_REQUIRE(n >= 0, APS_E_ARG, "negative mark count");
        APS_REQUIRE(n == 0 || marks, APS_E_ARG, "NULL mark table");
        for (int64_t k = 0; k < n; ++k) {
            APS_REQUIRE(marks[k].kind == APS_MARK_SEGMENT || marks[k].kind == APS_MARK_RING, APS_E_ARG,
                        "mark %lld: kind must be APS_MARK_SEGMENT or APS_MARK_RING (got %d)", (long long)k, marks[k].kind);
            APS_REQUIRE(marks[k].line_width >= 1 && marks[k].line_width <= kMarkMaxWidth, APS_E_ARG,
                        "mark %lld: line width must be in 1..%d (got %d)", (long long)k, kMarkMaxWidth, marks[k].line_width);
        }
        const size_t bytes = (size_t)h * (size_t)w * 3;
        APS_REQUIRE(src == dst || !ranges_overlap(src, bytes, dst, bytes), APS_E_ARG,
                    "source and destination overlap without being the same buffer");
        const MarkPlan P = mark_plan(h, w, marks, n);  // (host work only; refuses lists beyond 32-bit indexing)
        ctx();
        // the canvas: one copy from the source into the buffer that is drawn on (none in place)
        const bool src_dev = is_device_ptr(src), dst_dev = is_device_ptr(dst);
        Ws<uint8_t> tmp;
        uint8_t* d = dst;
        if (!dst_dev) {
            tmp.alloc(bytes);
            d = tmp.p;
        }
        if (d != src) {
            Prof prof("marks_copy");
            APS_HIP(hipMemcpyAsync(d, src, bytes, src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream()));
        }
        const int n_tiles = (int)(P.tile_xy.size() / 2);
        std::vector<uint8_t> pack;  // (host and device copies of the lists live until the synchronisation below)
        Ws<uint8_t> dp;
        if (n_tiles > 0) {
            // one upload: items | tile_xy | tile_off | item_idx
            const size_t b_items = P.items.size() * sizeof(MarkItem), b_xy = P.tile_xy.size() * 4, b_off = P.tile_off.size() * 4,
                         b_idx = P.item_idx.size() * 4;
            pack.resize(b_items + b_xy + b_off + b_idx);
            std::memcpy(pack.data(), P.items.data(), b_items);
            std::memcpy(pack.data() + b_items, P.tile_xy.data(), b_xy);
            std::memcpy(pack.data() + b_items + b_xy, P.tile_off.data(), b_off);
            std::memcpy(pack.data() + b_items + b_xy + b_off, P.item_idx.data(), b_idx);
            dp.alloc(pack.size());
            APS_HIP(hipMemcpyAsync(dp.p, pack.data(), pack.size(), hipMemcpyHostToDevice, stream()));
            {
                Prof prof("mark_tiles");
                mark_tiles_kernel<<<(unsigned)n_tiles, 256, 0, stream()>>>(
                    d, h, w, reinterpret_cast<const int32_t*>(dp.p + b_items), reinterpret_cast<const int32_t*>(dp.p + b_items + b_xy),
                    reinterpret_cast<const int32_t*>(dp.p + b_items + b_xy + b_off), reinterpret_cast<const MarkItem*>(dp.p));
            }
            check_launch("mark_tiles_kernel");
        }
        if (!dst_dev) APS_HIP(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, stream()));
        // one synchronisation, always: the packed lists are host memory of this call, and a resident result is complete on return
        APS_HIP(hipStreamSynchronize(stream()));
        if (n_drawn) *n_drawn = P.n_drawn;
    });
}

extern "C" int aps_montage_pair(const uint8_t* img1, int64_t h1, int64_t w1, const uint8_t* img2, int64_t h2, int64_t w2,
                                uint8_t* dst) {
    return guarded([&] {
        APS_REQUIRE(img1 && img2 && dst, APS_E_ARG, "NULL argument");
        APS_REQUIRE(h1 >= 1 && w1 >= 1 && h2 >= 1 && w2 >= 1 && h1 <= INT32_MAX && h2 <= INT32_MAX && w1 + w2 <= INT32_MAX, APS_E_ARG,
                    "bad image sizes %lld x %lld, %lld x %lld", (long long)h1, (long long)w1, (long long)h2, (long long)w2);
        const int64_t H = std::max(h1, h2), W = w1 + w2;
        const size_t bytes = (size_t)H * (size_t)W * 3, pitch = (size_t)W * 3;
        APS_REQUIRE(!ranges_overlap(img1, (size_t)h1 * w1 * 3, dst, bytes) && !ranges_overlap(img2, (size_t)h2 * w2 * 3, dst, bytes),
                    APS_E_ARG, "the destination overlaps a source image");
        ctx();
        const bool dst_dev = is_device_ptr(dst);
        Ws<uint8_t> tmp;
        uint8_t* d = dst;
        if (!dst_dev) {
            tmp.alloc(bytes);
            d = tmp.p;
        }
        {
            Prof prof("montage_pair");
            // the rows under the shorter image are 0; then one strided copy per image
            if (h1 < H) APS_HIP(hipMemset2DAsync(d + (size_t)h1 * pitch, pitch, 0, (size_t)w1 * 3, (size_t)(H - h1), stream()));
            if (h2 < H) APS_HIP(hipMemset2DAsync(d + (size_t)h2 * pitch + (size_t)w1 * 3, pitch, 0, (size_t)w2 * 3, (size_t)(H - h2), stream()));
            APS_HIP(hipMemcpy2DAsync(d, pitch, img1, (size_t)w1 * 3, (size_t)w1 * 3, (size_t)h1,
                                     is_device_ptr(img1) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream()));
            APS_HIP(hipMemcpy2DAsync(d + (size_t)w1 * 3, pitch, img2, (size_t)w2 * 3, (size_t)w2 * 3, (size_t)h2,
                                     is_device_ptr(img2) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream()));
        }
        if (!dst_dev) APS_HIP(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, stream()));
        APS_HIP(hipStreamSynchronize(stream()));  // host sources and a host destination are the caller's again on return
    });
}
