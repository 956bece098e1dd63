"""The mark contract ("Mark contract") restated in plain Python / NumPy: what aps_draw_marks, aps_montage_pair and the
match and keypoint plots above them must produce, byte for byte.  Integer arithmetic throughout: the exact comparisons are made
on Python integers, which cannot overflow.

A mark here is anything indexable by field name ('x0', 'y0', 'x1', 'y1', 'kind', 'line_width', 'rgb'): the dicts segment() and
ring() make, or the rows of a NumPy record array.  It shares no code with the library."""
import math

import numpy as np

COORD_MAX = 2 ** 20
RADIUS_MAX = 4096
SEGMENT, RING = 0, 1
PLOT_COLORS = ((255, 0, 0), (0, 255, 0), (255, 255, 0))  # points of image 1, points of image 2, lines


def segment(x0, y0, x1, y1, rgb, line_width=1):
    return {"x0": float(x0), "y0": float(y0), "x1": float(x1), "y1": float(y1), "kind": SEGMENT, "line_width": int(line_width),
            "rgb": tuple(int(v) for v in rgb)}


def ring(x, y, radius, rgb, line_width=1):
    return {"x0": float(x), "y0": float(y), "x1": float(radius), "y1": 0.0, "kind": RING, "line_width": int(line_width),
            "rgb": tuple(int(v) for v in rgb)}


def quant(v):
    """q(v) = floor(16 v + 0.5) in IEEE f64, as a Python int."""
    return int(math.floor(16.0 * float(v) + 0.5))


def coord_ok(v):
    v = float(v)
    return math.isfinite(v) and abs(v) <= COORD_MAX


def radius_ok(v):
    v = float(v)
    return math.isfinite(v) and 0 <= v <= RADIUS_MAX


def mark_ok(m):
    if int(m["kind"]) == SEGMENT:
        return all(coord_ok(m[k]) for k in ("x0", "y0", "x1", "y1"))
    return coord_ok(m["x0"]) and coord_ok(m["y0"]) and radius_ok(m["x1"])


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


def ring_hit(cx, cy, px, py, Rq, R):
    d2 = (cx - px) ** 2 + (cy - py) ** 2
    return max(Rq - R, 0) ** 2 <= d2 <= (Rq + R) ** 2


def _ceil16(v):
    return -((-v) // 16)


def seg_hit_grid(cx, cy, x0, y0, x1, y1, R):
    """seg_hit on int64 grids cx, cy: the same three cases.  Only for operands small enough that no product leaves int64
    (mark_mask checks: every lattice value within 2^14, so |cross|^2 <= 2^62 and R^2 D.D < 2^50)."""
    Dx, Dy, Ax, Ay = x1 - x0, y1 - y0, cx - x0, cy - y0
    DD = Dx * Dx + Dy * Dy
    t = Ax * Dx + Ay * Dy
    Bx, By = cx - x1, cy - y1
    cross = Ax * Dy - Ay * Dx
    return np.where(t <= 0, Ax * Ax + Ay * Ay <= R * R, np.where(t >= DD, Bx * Bx + By * By <= R * R, cross * cross <= R * R * DD))


def mark_mask(H, W, m, python_ints=False):
    """bool H x W: the pixels a valid mark paints.  The test is made pixel by pixel on Python ints; where every lattice value
    is within 2^14 (canvases and coordinates up to 1024 px) the same test runs on int64 grids, which cannot overflow there
    (python_ints=True keeps the pixel loop; tests/test_marks_mirror.py holds the two against each other)."""
    R = 8 * int(m["line_width"])
    out = np.zeros((H, W), bool)
    if int(m["kind"]) == SEGMENT:
        x0, y0, x1, y1 = (quant(m[k]) for k in ("x0", "y0", "x1", "y1"))
        lo_x, hi_x, lo_y, hi_y = min(x0, x1) - R, max(x0, x1) + R, min(y0, y1) - R, max(y0, y1) + R
        hit = lambda cx, cy: seg_hit(cx, cy, x0, y0, x1, y1, R)  # noqa: E731
        grid = lambda cx, cy: seg_hit_grid(cx, cy, x0, y0, x1, y1, R)  # noqa: E731
        reach = max(abs(v) for v in (x0, y0, x1, y1))
    else:
        px, py, Rq = quant(m["x0"]), quant(m["y0"]), quant(m["x1"])
        lo_x, hi_x, lo_y, hi_y = px - Rq - R, px + Rq + R, py - Rq - R, py + Rq + R
        hit = lambda cx, cy: ring_hit(cx, cy, px, py, Rq, R)  # noqa: E731
        grid = lambda cx, cy: (max(Rq - R, 0) ** 2 <= (cx - px) ** 2 + (cy - py) ** 2) & ((cx - px) ** 2 + (cy - py) ** 2 <= (Rq + R) ** 2)  # noqa: E731
        reach = max(abs(px), abs(py))
    # only pixels whose centre (16 c, 16 r) lies in the mark's bounding box grown by R can be hit
    r_lo, r_hi, c_lo, c_hi = max(1, _ceil16(lo_y)), min(H, hi_y // 16), max(1, _ceil16(lo_x)), min(W, hi_x // 16)
    if r_lo > r_hi or c_lo > c_hi:
        return out
    if not python_ints and max(reach, 16 * H, 16 * W) <= 2 ** 14:
        cy, cx = np.meshgrid(16 * np.arange(r_lo, r_hi + 1, dtype=np.int64), 16 * np.arange(c_lo, c_hi + 1, dtype=np.int64), indexing="ij")
        out[r_lo - 1:r_hi, c_lo - 1:c_hi] = grid(cx, cy)
        return out
    for r in range(r_lo, r_hi + 1):
        for c in range(c_lo, c_hi + 1):
            if hit(16 * c, 16 * r):
                out[r - 1, c - 1] = True
    return out


def draw_marks(src, marks):
    """(copy of src with the marks drawn in ascending index, number of valid marks)."""
    out = np.array(src, np.uint8, copy=True)
    assert out.ndim == 3 and out.shape[2] == 3
    H, W = out.shape[:2]
    for m in marks:  # an argument error for the whole call, before anything is drawn
        if int(m["kind"]) not in (SEGMENT, RING) or not 1 <= int(m["line_width"]) <= 64:
            raise ValueError("bad kind or line_width")
    drawn = 0
    for m in marks:
        if not mark_ok(m):
            continue  # skipped and not counted
        drawn += 1
        out[mark_mask(H, W, m)] = [int(v) for v in m["rgb"]][:3]
    return out, drawn


def montage_pair(I1, I2):
    I1, I2 = (np.repeat(a.reshape(a.shape[0], a.shape[1], 1), 3, axis=2) if a.ndim == 2 or a.shape[2] == 1 else a
              for a in (np.asarray(I1, np.uint8), np.asarray(I2, np.uint8)))
    (h1, w1), (h2, w2) = I1.shape[:2], I2.shape[:2]
    out = np.zeros((max(h1, h2), w1 + w2, 3), np.uint8)
    out[:h1, :w1] = I1
    out[:h2, w1:] = I2
    return out


def match_plot_marks(p1, p2, w1, markerRadius=3, lineWidth=1, colors=None):
    """Lines, then rings on the points of image 1, then a plus per point of image 2 (shifted by w1); rows with a non-finite
    coordinate contribute nothing."""
    c1, c2, cl = PLOT_COLORS if colors is None else colors
    rows = [(float(a[0]), float(a[1]), float(b[0]) + float(w1), float(b[1])) for a, b in zip(p1, p2)
            if all(math.isfinite(float(v)) for v in (a[0], a[1], b[0], b[1]))]
    m = float(markerRadius)
    marks = [segment(xa, ya, xb, yb, cl, lineWidth) for xa, ya, xb, yb in rows]
    marks += [ring(xa, ya, m, c1, lineWidth) for xa, ya, _, _ in rows]
    for _, _, xb, yb in rows:
        marks += [segment(xb - m, yb, xb + m, yb, c2, lineWidth), segment(xb, yb - m, xb, yb + m, c2, lineWidth)]
    return marks


def match_plot(I1, I2, p1, p2, **style):
    return draw_marks(montage_pair(I1, I2), match_plot_marks(p1, p2, np.asarray(I1).shape[1], **style))[0]


def keypoint_marks(points, scales=None, angles_deg=None, color=(0, 255, 0), markerRadius=3, lineWidth=1):
    """A ring per keypoint, then (with angles) a segment per keypoint from the centre to centre + radius (cos a, -sin a)."""
    pts = [(float(x), float(y)) for x, y in points]
    radii = [float(markerRadius)] * len(pts) if scales is None else [float(s) for s in scales]
    marks = [ring(x, y, r, color, lineWidth) for (x, y), r in zip(pts, radii)]
    if angles_deg is not None:
        a = np.deg2rad(np.asarray(angles_deg, np.float64).reshape(-1))  # (arrays, as the wrapper: NumPy f64 element-wise)
        ca, sa = np.cos(a), np.sin(a)
        for k, ((x, y), r) in enumerate(zip(pts, radii)):
            marks.append(segment(x, y, x + r * float(ca[k]), y + r * -float(sa[k]), color, lineWidth))
    return marks
