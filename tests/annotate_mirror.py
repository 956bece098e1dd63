"""The annotation contract ("Annotation contract") restated in plain Python / NumPy: what aps_annotate_panorama must
produce, byte for byte.  Integer arithmetic throughout: the exact comparisons are made on Python integers, which cannot overflow.

Holds its own copy of the glyph table; it shares no code with the library."""
import math

import numpy as np

COORD_MAX = 2 ** 20
GLYPH_SCALE, GLYPH_GAP, PAD = 3, 3, 4
GLYPH_W, GLYPH_H = 5 * GLYPH_SCALE, 7 * GLYPH_SCALE
LABEL_H = GLYPH_H + 2 * PAD
BOX = (255, 0, 0)

# 5 x 7 digits, top row first, '#' = ink
GLYPHS = {
    0: (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    1: ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    2: (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    3: ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    4: ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    5: ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    6: ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    7: ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    8: (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    9: (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
}


def quant(v):
    """q(v) = floor(16 v + 0.5) in IEEE f64, as a Python int."""
    return int(math.floor(16.0 * float(v) + 0.5))


def coord_ok(v):
    v = float(v)
    return math.isfinite(v) and abs(v) <= COORD_MAX


def valid_polygon(poly):
    return all(coord_ok(v) for v in np.asarray(poly, np.float64).reshape(-1))


def seg_hit(cx, cy, x0, y0, x1, y1, R):
    """The exact test of one pixel centre (cx, cy) against the closed segment, all Python ints (lattice units)."""
    Dx, Dy, Ax, Ay = x1 - x0, y1 - y0, cx - x0, cy - y0
    DD = Dx * Dx + Dy * Dy
    t = Ax * Dx + Ay * Dy
    if t <= 0:
        return Ax * Ax + Ay * Ay <= R * R
    if t >= DD:
        Bx, By = cx - x1, cy - y1
        return Bx * Bx + By * By <= R * R
    cross = Ax * Dy - Ay * Dx
    return cross * cross <= R * R * DD


def edge_mask(H, W, p0, p1, line_width):
    """bool H x W: the pixels an edge between the (already quantised, lattice) points p0 -> p1 paints."""
    R = 8 * int(line_width)
    x0, y0, x1, y1 = int(p0[0]), int(p0[1]), int(p1[0]), int(p1[1])
    m = np.zeros((H, W), bool)
    # only pixels within R of the bounding box can be hit (1-based c with 16 c in [xmin - R, xmax + R])
    c_lo, c_hi = max(1, -((-(min(x0, x1) - R)) // 16)), min(W, (max(x0, x1) + R) // 16)
    r_lo, r_hi = max(1, -((-(min(y0, y1) - R)) // 16)), min(H, (max(y0, y1) + R) // 16)
    for r in range(r_lo, r_hi + 1):
        for c in range(c_lo, c_hi + 1):
            if seg_hit(16 * c, 16 * r, x0, y0, x1, y1, R):
                m[r - 1, c - 1] = True
    return m


def label_layout(number):
    digits = [int(ch) for ch in str(int(number))]
    return digits, 2 * PAD + len(digits) * GLYPH_W + (len(digits) - 1) * GLYPH_GAP


def draw_label(img, r0, c0, number):
    """Blend the box and write the text of one label whose top-left pixel is (r0, c0), 1-based; clipped."""
    H, W = img.shape[:2]
    digits, bw = label_layout(number)
    for r in range(max(1, r0), min(H, r0 + LABEL_H - 1) + 1):
        for c in range(max(1, c0), min(W, c0 + bw - 1) + 1):
            x, y = c - c0 - PAD, r - r0 - PAD
            text = False
            if x >= 0 and 0 <= y < GLYPH_H:
                g, xin = divmod(x, GLYPH_W + GLYPH_GAP)
                if g < len(digits) and xin < GLYPH_W:
                    text = GLYPHS[digits[g]][y // GLYPH_SCALE][xin // GLYPH_SCALE] == "#"
            if text:
                img[r - 1, c - 1] = (255, 255, 255)
            else:
                s = img[r - 1, c - 1].astype(np.int64)
                img[r - 1, c - 1] = [(2 * int(s[k]) + 3 * BOX[k] + 2) // 5 for k in range(3)]


def annotate(src, polys, anchors, colors, line_width=2):
    """(annotated copy of src, number of polygons drawn)."""
    out = np.array(src, np.uint8, copy=True)
    assert out.ndim == 3 and out.shape[2] == 3
    H, W = out.shape[:2]
    polys = np.asarray(polys, np.float64).reshape(-1, 4, 2)
    anchors = np.asarray(anchors, np.float64).reshape(-1, 2)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    labels = []
    drawn = 0
    for p in range(len(polys)):
        if not valid_polygon(polys[p]):
            continue  # skipped and not numbered
        drawn += 1
        q = [(quant(x), quant(y)) for x, y in polys[p]]
        for e in range(4):
            out[edge_mask(H, W, q[e], q[(e + 1) % 4], line_width)] = colors[p]
        ax, ay = anchors[p]
        if coord_ok(ax) and coord_ok(ay):
            labels.append((int(math.floor(ay + 0.5)), int(math.floor(ax + 0.5)), drawn))
    for r0, c0, number in labels:  # after all outlines, ascending
        draw_label(out, r0, c0, number)
    return out, drawn


def allowed_change_mask(H, W, polys, anchors, line_width=2):
    """bool H x W: where an annotation may differ from its panorama - within line_width / 2 + 1 px of an outline (Euclidean, from
    the unquantised corners, in floating point with the margin that pixel of slack gives) or inside a label box."""
    m = np.zeros((H, W), bool)
    rr, cc = np.mgrid[1:H + 1, 1:W + 1].astype(np.float64)
    number = 0
    for p, poly in enumerate(np.asarray(polys, np.float64).reshape(-1, 4, 2)):
        if not valid_polygon(poly):
            continue
        number += 1
        for e in range(4):
            (x0, y0), (x1, y1) = poly[e], poly[(e + 1) % 4]
            dx, dy = x1 - x0, y1 - y0
            dd = dx * dx + dy * dy
            t = np.clip(((cc - x0) * dx + (rr - y0) * dy) / dd, 0, 1) if dd > 0 else np.zeros_like(cc)
            dist = np.hypot(cc - (x0 + t * dx), rr - (y0 + t * dy))
            m |= dist <= line_width / 2 + 1
        ax, ay = np.asarray(anchors, np.float64).reshape(-1, 2)[p]
        if coord_ok(ax) and coord_ok(ay):
            r0, c0 = int(math.floor(ay + 0.5)), int(math.floor(ax + 0.5))
            _, bw = label_layout(number)
            m[max(0, r0 - 1):max(0, r0 - 1 + LABEL_H), max(0, c0 - 1):max(0, c0 - 1 + bw)] = True
    return m
