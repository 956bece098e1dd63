"""NumPy restatement of the FAST/FREAK scale pyramid (DESIGN.md "FAST/FREAK scale pyramid") -- test infrastructure, not a test.

Written from the contract, not from the kernel.  The per-level work is fast_mirror's; what is added here is the plan of the
levels, the integer bilinear resampling and the mapping of a level's pixel back to level-0 coordinates.  Everything is integer
arithmetic up to the one f64 division and addition of a location, so ``extract`` returns what ``aps_fast_extract_pyramid``
returns, bit for bit.
"""
import numpy as np

import fast_mirror as fmir

MAX_LEVELS = 16


def scale_rational(ScaleFactor):
    """ScaleFactor as (num, den) with den = 10^6."""
    return int(round(float(ScaleFactor) * 1000000)), 1000000


def plan(h, w, n_levels, num, den, margin):
    """[(h_l, w_l)]: each level sized from the previous one, rounding half up; ends before the first level with no pixel at least
    `margin` from every edge, or at n_levels.  Level 0 always exists."""
    if not (1 <= n_levels <= MAX_LEVELS and 0 < den < num <= 2 * den):
        raise ValueError("n_levels in 1..16 and 1 < ScaleFactor <= 2")
    out = [(int(h), int(w))]
    while len(out) < n_levels:
        h, w = ((2 * s * den + num) // (2 * num) for s in out[-1])
        if min(h, w) < 2 * margin + 1:
            break
        out.append((h, w))
    return out


def axis(n_src, n_dst):
    """(first tap, second tap, weight of the second tap in 1/256) per destination index: half-pixel centres."""
    x = np.arange(n_dst, dtype=np.int64)
    X = (2 * x + 1) * n_src - n_dst
    x0 = X // (2 * n_dst)   # (floor division)
    fx = X - 2 * n_dst * x0
    wx = (256 * fx) // (2 * n_dst)
    return np.clip(x0, 0, n_src - 1), np.clip(x0 + 1, 0, n_src - 1), wx


def resample(src, h, w):
    """The (h, w) plane resampled from the integer plane src: bilinear, 8-bit weights, rounded half up."""
    src = np.asarray(src, np.int64)
    y0, y1, wy = axis(src.shape[0], h)
    x0, x1, wx = axis(src.shape[1], w)
    wy = wy[:, None]
    top = (256 - wx) * src[y0][:, x0] + wx * src[y0][:, x1]
    bot = (256 - wx) * src[y1][:, x0] + wx * src[y1][:, x1]
    return ((256 - wy) * top + wy * bot + 32768) >> 16


def planes(img, NumLevels, ScaleFactor, margin):
    """The integer level planes: level 0 is rgb2gray's plane, level l is level l - 1 resampled."""
    out = [fmir.gray_plane(img)]
    for (h, w) in plan(*out[0].shape, NumLevels, *scale_rational(ScaleFactor), margin)[1:]:
        out.append(resample(out[-1], h, w))
    return out


def loc_of(xs, ys, level_shape, shape0):
    """[n, 2] f64 [x y], 1-based, of level pixels (xs, ys) in level-0 coordinates: one division and one addition."""
    (hl, wl), (h0, w0) = level_shape, shape0
    lx = ((2 * np.asarray(xs, np.int64) + 1) * w0).astype(np.float64) / np.float64(2 * wl) + 0.5
    ly = ((2 * np.asarray(ys, np.int64) + 1) * h0).astype(np.float64) / np.float64(2 * hl) + 0.5
    return np.stack([lx, ly], 1)


def extract(img, tb, NumLevels=1, ScaleFactor=1.2, MinContrast=0.2, MinQuality=0.1):
    """(desc uint8 [n, 64], loc float64 [n, 2] 1-based [x y] in level-0 coordinates, aux float32 [n, 4] = [score, bin, level, 0]),
    in ascending (level, row, col) order: fast_mirror.extract on every level's plane."""
    lv = planes(img, NumLevels, ScaleFactor, tb.margin)
    D, L, A = [np.zeros((0, 64), np.uint8)], [np.zeros((0, 2), np.float64)], [np.zeros((0, 4), np.float32)]
    for l, g in enumerate(lv):
        d, loc, aux = fmir.extract(g.astype(np.uint8), tb, MinContrast=MinContrast, MinQuality=MinQuality)
        aux[:, 2] = l
        D.append(d)
        L.append(loc_of(loc[:, 0].astype(np.int64) - 1, loc[:, 1].astype(np.int64) - 1, g.shape, lv[0].shape))
        A.append(aux)
    return np.concatenate(D), np.concatenate(L), np.concatenate(A)
