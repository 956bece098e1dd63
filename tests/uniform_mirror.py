"""NumPy restatement of uniform-N selection (DESIGN.md "Uniform-N selection") -- test infrastructure, not a test.

Written from the contract, not from the kernels.  Candidates, strengths, groups and canonical order are those of the detector's
strongest-N rule (strongest_mirror.py, fast_strongest_mirror.py); what is added here is the cell of a candidate, the water-filling of
a group's budget over its cells, and the selection within a cell by (strength descending, canonical index ascending).  Integer
arithmetic throughout.  The per-detector providers return the 0-based pixel (py, px) of every candidate and its plane (Hp, Wp).
"""
import numpy as np

import fast_pyramid_mirror as pmir
import fast_strongest_mirror as smir
import surf_mirror

DEFAULT_GRID = (8, 8)


def cell(py, px, Hp, Wp, grid):
    """Cell index of the 0-based integer pixels (py, px) of an Hp x Wp plane in a (rows, cols) grid; arrays broadcast."""
    rows, cols = grid
    py, px = np.asarray(py, np.int64), np.asarray(px, np.int64)
    assert ((0 <= py) & (py < Hp) & (0 <= px) & (px < Wp)).all()
    return (py * rows // Hp) * cols + px * cols // Wp


def waterfill(counts, Q):
    """keep[k] per cell: with the budget min(Q, sum c), t is the largest integer with S(t) = sum min(c, t) <= budget, every cell keeps
    min(c, t), and the first budget - S(t) cells in ascending k with c > t keep one more.  t comes from the sorted counts (with the i
    smallest cells below the level, S(t) = their sum + (m - i) t) and is then checked against its definition."""
    c = np.asarray(counts, np.int64)
    assert c.ndim == 1 and (c >= 0).all()
    Q = min(int(Q), int(c.sum()))
    srt = [int(v) for v in np.sort(c)]
    t, below = (srt[-1] if srt else 0), 0
    for i, v in enumerate(srt):
        level = (Q - below) // (len(srt) - i)
        if level < v:
            t = level
            break
        below += v
    S = lambda lv: sum(min(v, lv) for v in srt)  # noqa: E731
    assert S(t) <= Q and (t == (srt[-1] if srt else 0) or S(t + 1) > Q)
    out = np.minimum(c, t)
    r = Q - int(out.sum())
    above = np.flatnonzero(c > t)
    assert 0 <= r and (r < len(above) or (r == 0 and len(above) == 0))
    out[above[:r]] += 1
    return out


def keep(strength, segment, budgets, cells=DEFAULT_GRID[0] * DEFAULT_GRID[1]):
    """Ascending indices of the kept candidates.  strength: f32 (non-negative) or int64 per candidate; segment = group * cells + cell;
    budgets[g]: the rows group g keeps (at most its candidates)."""
    strength, segment = np.asarray(strength), np.asarray(segment, np.int64)
    assert strength.ndim == 1 and strength.shape == segment.shape and strength.dtype in (np.float32, np.int64)
    key = strength.astype(np.float64) if strength.dtype == np.float32 else strength   # (f32 -> f64 is exact and keeps the order)
    kept = [np.zeros(0, np.int64)]
    for g, Q in enumerate(budgets):
        counts = np.bincount(segment[(segment >= g * cells) & (segment < (g + 1) * cells)] - g * cells, minlength=cells)
        assert Q <= counts.sum()
        for k, n in enumerate(waterfill(counts, Q)):
            at = np.flatnonzero(segment == g * cells + k)
            kept.append(at[np.argsort(-key[at], kind="stable")[:n]])   # stable: ties to the lower canonical index
    return np.sort(np.concatenate(kept))


def occupancy(segment, at, n_segments):
    """Rows per segment among the candidates `at`."""
    return np.bincount(np.asarray(segment, np.int64)[at], minlength=n_segments)


# ---- SIFT: rows of the unselected result; the pixel comes from the row's 1-based f64 location -------------------------------
def sift_pixels(loc, shape):
    H, W = shape[:2]
    px = np.clip(np.floor(loc[:, 0]).astype(np.int64) - 1, 0, W - 1)
    py = np.clip(np.floor(loc[:, 1]).astype(np.int64) - 1, 0, H - 1)
    return py, px, (H, W)


def sift_keep(result, shape, N, grid=DEFAULT_GRID):
    """Indices into the unselected (desc, loc, aux) that NumUniform = N keeps."""
    if N < 1:
        raise ValueError("NumUniform must be at least 1")
    d, loc, aux = result
    py, px, (H, W) = sift_pixels(loc, shape)
    return keep(aux[:, 2], cell(py, px, H, W, grid), [min(N, len(loc))], grid[0] * grid[1])


# ---- SURF: the candidates of surf_mirror.detect; the pixel is the detection sample (i * step, j * step) -------------------
def surf_pixels(img, MetricThreshold=1000.0):
    k = surf_mirror.detect(surf_mirror.integral(surf_mirror.gray_plane(img)), MetricThreshold)
    step = 1 << (k["o"] - 1)
    return k["i"] * step, k["j"] * step, img.shape[:2], k["metric"]


def surf_keep(img, result, MetricThreshold, N, grid=DEFAULT_GRID):
    if N < 1:
        raise ValueError("NumUniform must be at least 1")
    py, px, (H, W), metric = surf_pixels(img, MetricThreshold)
    assert np.array_equal(metric, result[2][:, 2])   # the same candidates in the same order as the unselected rows
    return keep(metric, cell(py, px, H, W, grid), [min(N, len(metric))], grid[0] * grid[1])


# ---- FAST: fast_strongest_mirror.candidates; the pixel is the candidate's level pixel, the plane its level's ------------------
def fast_pixels(cand):
    """(py, px, level, shapes) of candidates(): the level pixels behind the level-0 locations (pmir.loc_of inverted, and checked)."""
    desc, loc, aux, R, shapes = cand
    level = aux[:, 2].astype(np.int64)
    hl, wl = (np.array([s[a] for s in shapes], np.int64)[level] for a in (0, 1))
    h0, w0 = shapes[0]
    px = np.rint(((loc[:, 0] - 0.5) * 2 * wl / w0 - 1) / 2).astype(np.int64)
    py = np.rint(((loc[:, 1] - 0.5) * 2 * hl / h0 - 1) / 2).astype(np.int64)
    for l, s in enumerate(shapes):
        m = level == l
        assert np.array_equal(pmir.loc_of(px[m], py[m], s, shapes[0]), loc[m])
    return py, px, level, shapes


def fast_keep(cand, N, grid=DEFAULT_GRID):
    if N < 1:
        raise ValueError("NumUniform must be at least 1")
    desc, loc, aux, R, shapes = cand
    py, px, level, _ = fast_pixels(cand)
    cells = grid[0] * grid[1]
    segment = np.zeros(len(R), np.int64)
    for l, (h, w) in enumerate(shapes):
        m = level == l
        segment[m] = l * cells + cell(py[m], px[m], h, w, grid)
    M_l = np.bincount(level, minlength=len(shapes)).tolist()
    budgets = smir.kept_per_level(M_l, smir.quotas(shapes, N), N)   # the rows the strongest-N call keeps on every level
    return keep(R, segment, budgets, cells), segment


def fast_pick(cand, N, grid=DEFAULT_GRID):
    """(desc, loc, aux) of the call with NumUniform = N; aux[:, 3] = f32(R) as in the strongest call."""
    desc, loc, aux, R, shapes = cand
    at, _ = fast_keep(cand, N, grid)
    out = aux[at].copy()
    out[:, 3] = R[at].astype(np.float32)
    return desc[at].copy(), loc[at].copy(), out
