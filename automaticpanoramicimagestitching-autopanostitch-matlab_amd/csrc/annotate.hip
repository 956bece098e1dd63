// annotate.hip — the annotated panorama on gfx950: image outlines and image numbers drawn on the resident canvas.
//
// Restates the drawing step of PP/renderPanorama/renderPanorama.m:438-477 (ray renderer) and :653-679 (planar scans):
// insertShape(panorama, 'Polygon', ..., 'LineWidth', 2) followed by insertText(..., centers, labels, 'BoxColor', 'red',
// 'TextColor', 'white').  Both toolbox calls are closed; the raster rule is this project's own and is stated operation by
// operation in DESIGN.md ("Annotation contract"); tests/annotate_mirror.py restates it in numpy, byte for byte.
//
// Shape of the work: drawing is sparse.  One copy brings the source canvas to the destination (none when drawing in
// place).  The host half quantises the corners to sixteenths of a pixel, bins every edge and every label box to the
// 64 x 64 pixel tiles it can touch, and uploads one CSR list.  One workgroup runs per TOUCHED tile and walks its list in
// ascending order (all edges by polygon, then all labels by number); a lane owns 16 pixels of the tile, keeps what it
// painted in registers and stores each painted pixel once.  An outline pixel needs no load (it is overwritten); only
// pixels under a label box are read.  No kernel visits a tile that nothing touches.
//
// Arithmetic: integers only.  Lattice coordinates (1/16 px) of valid corners satisfy |q| <= 2^24, pixel centres
// 16 * c <= 2^35 for any int canvas, so differences stay below 2^36, and the dot and cross products of a difference with
// an edge vector (|D| components <= 2^25) stay below 2^62: inside int64.  The squares cross^2 and R^2 * (D.D) do NOT fit
// 64 bits (up to 2^124); they are compared as 128-bit products (high and low words), so nothing is ever truncated.  The
// end-point test squares a difference only after |Ax| <= R and |Ay| <= R have been checked.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "aps_internal.h"
#include "raster_dev.h"  // ann_mulhi / ann_disc / ann_seg_hit: the exact edge test, shared with marks.hip

namespace aps {

constexpr int kAnnTile = 64;        // tile side in pixels
constexpr int kAnnMaxWidth = 64;    // largest line width
constexpr int64_t kAnnCoordMax = 1 << 20;  // |coordinate| bound of a valid polygon, in pixels
// label geometry: 5 x 7 glyphs scaled by 3, 3 px between glyphs, 4 px of padding around the text
constexpr int kGlyphScale = 3, kGlyphW = 5 * kGlyphScale, kGlyphH = 7 * kGlyphScale, kGlyphGap = 3, kLabelPad = 4;
constexpr int kLabelH = kGlyphH + 2 * kLabelPad;

// The ten digits as bit rows, top row first, bit 4 = leftmost column.
__constant__ uint8_t kGlyphRows[10][7] = {
    {0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110},  // 0
    {0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110},  // 1
    {0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111},  // 2
    {0b11111, 0b00010, 0b00100, 0b00010, 0b00001, 0b10001, 0b01110},  // 3
    {0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010},  // 4
    {0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110},  // 5
    {0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110},  // 6
    {0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000},  // 7
    {0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110},  // 8
    {0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100},  // 9
};

// One entry of a tile's list.  kind 0, an edge: (a, b) -> (c, d) in lattice units (x, y), e = colour (r | g << 8 | b << 16).
// kind 1, a label: a, b = row and column (1-based) of the box's top-left pixel, c = number of digits, d / e = the digits,
// four bits each, most significant digit in bits 0-3 of d, the ninth and tenth in e.
struct AnnItem {
    int32_t a, b, c, d;
    uint32_t e;
    uint32_t kind;
};

// One workgroup per touched tile; lane t owns column (t & 63) and the 16 rows (t >> 6) + 4 i of the tile.
__global__ __launch_bounds__(256) void annotate_tiles_kernel(uint8_t* __restrict__ img, int64_t H, int64_t W,
                                                             const int32_t* __restrict__ tile_xy,
                                                             const int32_t* __restrict__ tile_off,
                                                             const int32_t* __restrict__ item_idx,
                                                             const AnnItem* __restrict__ items, int R) {
    const int tile = blockIdx.x;
    const int64_t c = (int64_t)tile_xy[2 * tile] * kAnnTile + (threadIdx.x & 63) + 1;       // 1-based column
    const int64_t r_first = (int64_t)tile_xy[2 * tile + 1] * kAnnTile + (threadIdx.x >> 6) + 1;  // 1-based row of i = 0
    if (c > W || r_first > H) return;
    uint32_t px[16];
    uint32_t have = 0;  // bit i: px[i] holds the pixel's final-so-far colour
#pragma unroll
    for (int i = 0; i < 16; ++i) px[i] = 0;
    const int64_t cx = 16 * c;
    const int k_end = tile_off[tile + 1];
    for (int k = tile_off[tile]; k < k_end; ++k) {
        const AnnItem it = items[item_idx[k]];
        if (it.kind == 0) {
            const int64_t x0 = it.a, y0 = it.b, x1 = it.c, y1 = it.d;
            // a painted pixel lies within R of the edge's bounding box
            if (cx < (x0 < x1 ? x0 : x1) - R || cx > (x0 < x1 ? x1 : x0) + R) continue;
            const int64_t ylo = (y0 < y1 ? y0 : y1) - R, yhi = (y0 < y1 ? y1 : y0) + R;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t r = r_first + 4 * i;
                const int64_t cy = 16 * r;
                if (r <= H && cy >= ylo && cy <= yhi && ann_seg_hit(cx, cy, x0, y0, x1, y1, R)) {
                    px[i] = it.e;
                    have |= 1u << i;
                }
            }
        } else {
            const int64_t r0 = it.a, c0 = it.b;
            const int nd = it.c;
            const int64_t bw = 2 * kLabelPad + (int64_t)nd * kGlyphW + (int64_t)(nd - 1) * kGlyphGap;
            if (c < c0 || c >= c0 + bw) continue;
            const int x = (int)(c - c0) - kLabelPad;  // column inside the text area
            int col_bit = -1, digit = 0;             // glyph column 0..4 under this lane, or none
            if (x >= 0) {
                const int g = x / (kGlyphW + kGlyphGap), xin = x - g * (kGlyphW + kGlyphGap);
                if (g < nd && xin < kGlyphW) {
                    col_bit = 4 - xin / kGlyphScale;
                    digit = (int)(((g < 8 ? (uint32_t)it.d >> (4 * g) : it.e >> (4 * (g - 8)))) & 15u);
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t r = r_first + 4 * i;
                if (r > H || r < r0 || r >= r0 + kLabelH) continue;
                const int y = (int)(r - r0) - kLabelPad;
                const bool text = col_bit >= 0 && y >= 0 && y < kGlyphH && ((kGlyphRows[digit][y / kGlyphScale] >> col_bit) & 1);
                if (text) {
                    px[i] = 0x00FFFFFFu;
                } else {
                    if (!((have >> i) & 1u)) {
                        const uint8_t* q = img + ((r - 1) * W + (c - 1)) * 3;
                        px[i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
                    }
                    const uint32_t s = px[i];
                    // 60 % of the box colour (255, 0, 0): out = (2 src + 3 box + 2) / 5 per channel
                    const uint32_t rr = (2u * (s & 255u) + 3u * 255u + 2u) / 5u;
                    const uint32_t gg = (2u * ((s >> 8) & 255u) + 2u) / 5u;
                    const uint32_t bb = (2u * ((s >> 16) & 255u) + 2u) / 5u;
                    px[i] = rr | (gg << 8) | (bb << 16);
                }
                have |= 1u << i;
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
static inline int64_t ann_quant(double v) { return (int64_t)std::floor(16.0 * v + 0.5); }

static inline bool ann_coord_ok(double v) { return std::isfinite(v) && std::fabs(v) <= (double)kAnnCoordMax; }

struct AnnPlan {
    std::vector<AnnItem> items;
    std::vector<int32_t> tile_xy, tile_off, item_idx;
    int n_drawn = 0;
};

static inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

static AnnPlan ann_plan(int64_t H, int64_t W, const double* polys, const double* anchors, const uint8_t* colors, int n,
                        int line_width) {
    AnnPlan P;
    const int64_t R = 8 * (int64_t)line_width;
    const int64_t ntx = (W + kAnnTile - 1) / kAnnTile;
    std::vector<std::pair<int64_t, int32_t>> bins;  // (tile, item), appended in item order
    // a tile's pixel centres lie within 504 lattice units of its centre along each axis: half diagonal < 713
    const int64_t tile_span = 16 * kAnnTile, tile_ctr = 16 + 8 * (kAnnTile - 1), tile_rad = 713;
    struct Label {
        int64_t r0, c0;
        int number;
    };
    std::vector<Label> labels;
    for (int p = 0; p < n; ++p) {
        const double* v = polys + 8 * (size_t)p;
        bool ok = true;
        for (int e = 0; e < 8; ++e) ok = ok && ann_coord_ok(v[e]);
        if (!ok) continue;  // skipped and not numbered
        const int number = ++P.n_drawn;
        int64_t qx[4], qy[4];
        for (int e = 0; e < 4; ++e) {
            qx[e] = ann_quant(v[2 * e]);
            qy[e] = ann_quant(v[2 * e + 1]);
        }
        const uint32_t col = (uint32_t)colors[3 * (size_t)p] | ((uint32_t)colors[3 * (size_t)p + 1] << 8) |
                             ((uint32_t)colors[3 * (size_t)p + 2] << 16);
        for (int e = 0; e < 4; ++e) {
            const int64_t x0 = qx[e], y0 = qy[e], x1 = qx[(e + 1) & 3], y1 = qy[(e + 1) & 3];
            // pixels (1-based) whose centre lies within R of the edge's bounding box, clipped to the canvas
            const int64_t c_lo = std::max<int64_t>(1, -floor_div(-(std::min(x0, x1) - R), 16));
            const int64_t c_hi = std::min<int64_t>(W, floor_div(std::max(x0, x1) + R, 16));
            const int64_t r_lo = std::max<int64_t>(1, -floor_div(-(std::min(y0, y1) - R), 16));
            const int64_t r_hi = std::min<int64_t>(H, floor_div(std::max(y0, y1) + R, 16));
            if (c_lo > c_hi || r_lo > r_hi) continue;
            const int32_t id = (int32_t)P.items.size();
            P.items.push_back(AnnItem{(int32_t)x0, (int32_t)y0, (int32_t)x1, (int32_t)y1, col, 0u});
            for (int64_t ty = (r_lo - 1) / kAnnTile; ty <= (r_hi - 1) / kAnnTile; ++ty)
                for (int64_t tx = (c_lo - 1) / kAnnTile; tx <= (c_hi - 1) / kAnnTile; ++tx)
                    // conservative: the same exact test from the tile's centre with the radius grown by its half diagonal
                    if (ann_seg_hit(tx * tile_span + tile_ctr, ty * tile_span + tile_ctr, x0, y0, x1, y1, R + tile_rad))
                        bins.emplace_back(ty * ntx + tx, id);
        }
        const double ax = anchors[2 * (size_t)p], ay = anchors[2 * (size_t)p + 1];
        if (ann_coord_ok(ax) && ann_coord_ok(ay))  // (a label whose anchor is not a valid coordinate is not drawn)
            labels.push_back(Label{(int64_t)std::floor(ay + 0.5), (int64_t)std::floor(ax + 0.5), number});
    }
    for (const Label& L : labels) {  // after all outlines, ascending
        int digits[10], nd = 0;
        for (int v = L.number; v > 0; v /= 10) digits[nd++] = v % 10;  // least significant first
        const int64_t bw = 2 * kLabelPad + (int64_t)nd * kGlyphW + (int64_t)(nd - 1) * kGlyphGap;
        const int64_t c_lo = std::max<int64_t>(1, L.c0), c_hi = std::min<int64_t>(W, L.c0 + bw - 1);
        const int64_t r_lo = std::max<int64_t>(1, L.r0), r_hi = std::min<int64_t>(H, L.r0 + kLabelH - 1);
        if (c_lo > c_hi || r_lo > r_hi) continue;
        uint32_t d = 0, e = 0;
        for (int g = 0; g < nd; ++g) {
            const uint32_t dg = (uint32_t)digits[nd - 1 - g];
            if (g < 8) d |= dg << (4 * g);
            else e |= dg << (4 * (g - 8));
        }
        const int32_t id = (int32_t)P.items.size();
        P.items.push_back(AnnItem{(int32_t)L.r0, (int32_t)L.c0, nd, (int32_t)d, e, 1u});
        for (int64_t ty = (r_lo - 1) / kAnnTile; ty <= (r_hi - 1) / kAnnTile; ++ty)
            for (int64_t tx = (c_lo - 1) / kAnnTile; tx <= (c_hi - 1) / kAnnTile; ++tx) bins.emplace_back(ty * ntx + tx, id);
    }
    APS_REQUIRE(bins.size() < (size_t)INT32_MAX, APS_E_DIM, "too many (tile, item) pairs to annotate (%zu)", bins.size());
    // by tile; the item order inside a tile is the order of appending: edges by polygon, then labels by number
    std::stable_sort(bins.begin(), bins.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    P.item_idx.reserve(bins.size());
    for (size_t k = 0; k < bins.size(); ++k) {
        if (k == 0 || bins[k].first != bins[k - 1].first) {
            P.tile_xy.push_back((int32_t)(bins[k].first % ntx));
            P.tile_xy.push_back((int32_t)(bins[k].first / ntx));
            P.tile_off.push_back((int32_t)k);
        }
        P.item_idx.push_back(bins[k].second);
    }
    P.tile_off.push_back((int32_t)bins.size());
    return P;
}

// a small host-or-device array, read on the host
template <class T>
static std::vector<T> ann_fetch(const T* p, size_t count) {
    std::vector<T> v(count);
    if (count == 0) return v;
    if (is_device_ptr(p)) {
        APS_HIP(hipMemcpyAsync(v.data(), p, count * sizeof(T), hipMemcpyDeviceToHost, stream()));
        APS_HIP(hipStreamSynchronize(stream()));
    } else {
        std::memcpy(v.data(), p, count * sizeof(T));
    }
    return v;
}

}  // namespace aps

using namespace aps;

extern "C" int aps_annotate_panorama(const uint8_t* src, int64_t h, int64_t w, const double* polys, const double* anchors,
                                     const uint8_t* colors, int n, int line_width, uint8_t* dst, int* n_drawn) {
    return guarded([&] {
        APS_REQUIRE(src && dst && n_drawn, APS_E_ARG, "NULL argument");
        APS_REQUIRE(h >= 1 && w >= 1 && h <= INT32_MAX && w <= INT32_MAX, APS_E_ARG, "bad canvas size %lld x %lld", (long long)h,
                    (long long)w);
        APS_REQUIRE(n >= 0, APS_E_ARG, "negative polygon count");
        APS_REQUIRE(n == 0 || (polys && anchors && colors), APS_E_ARG, "NULL polygon, anchor or colour table");
        APS_REQUIRE(line_width >= 1 && line_width <= kAnnMaxWidth, APS_E_ARG, "line width must be in 1..%d (got %d)", kAnnMaxWidth,
                    line_width);
        const size_t bytes = (size_t)h * (size_t)w * 3;
        APS_REQUIRE(src == dst || src + bytes <= dst || dst + bytes <= src, APS_E_ARG,
                    "source and destination overlap without being the same buffer");
        ctx();
        const std::vector<double> hp = ann_fetch(polys, 8 * (size_t)n), ha = ann_fetch(anchors, 2 * (size_t)n);
        const std::vector<uint8_t> hc = ann_fetch(colors, 3 * (size_t)n);
        const AnnPlan P = ann_plan(h, w, hp.data(), ha.data(), hc.data(), n, line_width);
        // the canvas: one copy from the source into the buffer that is drawn on (none in place)
        const bool src_dev = is_device_ptr(src), dst_dev = is_device_ptr(dst);
        Ws<uint8_t> tmp;
        uint8_t* d = dst;
        if (!dst_dev) {
            tmp.alloc(bytes);
            d = tmp.p;
        }
        if (d != src) {
            Prof prof("annotate_copy");
            APS_HIP(hipMemcpyAsync(d, src, bytes, src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream()));
        }
        const int n_tiles = (int)(P.tile_xy.size() / 2);
        std::vector<uint8_t> pack;  // (host and device copies of the lists live until the synchronisation below)
        Ws<uint8_t> dp;
        if (n_tiles > 0) {
            // one upload: items | tile_xy | tile_off | item_idx
            const size_t b_items = P.items.size() * sizeof(AnnItem), b_xy = P.tile_xy.size() * 4, b_off = P.tile_off.size() * 4,
                         b_idx = P.item_idx.size() * 4;
            pack.resize(b_items + b_xy + b_off + b_idx);
            std::memcpy(pack.data(), P.items.data(), b_items);
            std::memcpy(pack.data() + b_items, P.tile_xy.data(), b_xy);
            std::memcpy(pack.data() + b_items + b_xy, P.tile_off.data(), b_off);
            std::memcpy(pack.data() + b_items + b_xy + b_off, P.item_idx.data(), b_idx);
            dp.alloc(pack.size());
            APS_HIP(hipMemcpyAsync(dp.p, pack.data(), pack.size(), hipMemcpyHostToDevice, stream()));
            {
                Prof prof("annotate_tiles");
                annotate_tiles_kernel<<<(unsigned)n_tiles, 256, 0, stream()>>>(
                    d, h, w, reinterpret_cast<const int32_t*>(dp.p + b_items), reinterpret_cast<const int32_t*>(dp.p + b_items + b_xy),
                    reinterpret_cast<const int32_t*>(dp.p + b_items + b_xy + b_off), reinterpret_cast<const AnnItem*>(dp.p), 8 * line_width);
            }
            check_launch("annotate_tiles_kernel");
        }
        if (!dst_dev) APS_HIP(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, stream()));
        // one synchronisation, always: the packed lists are host memory of this call, and a resident result is complete on return
        APS_HIP(hipStreamSynchronize(stream()));
        *n_drawn = P.n_drawn;
    });
}
