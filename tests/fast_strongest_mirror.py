"""NumPy restatement of FAST/FREAK strongest-N (DESIGN.md "FAST/FREAK strongest-N") -- test infrastructure, not a test.

Written from the contract, not from the kernel.  The candidates are fast_pyramid_mirror's rows; what is added here is the
integer Harris response of a candidate, the quota of a level, the carry from short coarse levels to finer ones and the
selection by (R descending, canonical index ascending).  Everything is int64 arithmetic up to the one conversion of R to
f32, so ``extract`` returns what ``aps_fast_extract_strongest`` returns, bit for bit.
"""
import math

import numpy as np

import fast_mirror as fmir
import fast_pyramid_mirror as pmir

WINDOW = 3   # the response sums over |v - y| <= 3, |u - x| <= 3; with the Sobel taps the reach is 4 pixels


def harris(plane, ys, xs):
    """int64 R = 25 (A B - C^2) - (A + B)^2 per pixel (ys[i], xs[i]) of the integer plane: A, B, C are the sums of Ix^2, Iy^2 and
    Ix Iy (3 x 3 Sobel) over the 7 x 7 window.  Every pixel must lie at least 4 from each edge."""
    g = np.asarray(plane, np.int64)
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    A, B, Cc = (np.zeros(len(ys), np.int64) for _ in range(3))
    for dv in range(-WINDOW, WINDOW + 1):
        for du in range(-WINDOW, WINDOW + 1):
            v, u = ys + dv, xs + du
            ix = (g[v - 1, u + 1] + 2 * g[v, u + 1] + g[v + 1, u + 1]) - (g[v - 1, u - 1] + 2 * g[v, u - 1] + g[v + 1, u - 1])
            iy = (g[v + 1, u - 1] + 2 * g[v + 1, u] + g[v + 1, u + 1]) - (g[v - 1, u - 1] + 2 * g[v - 1, u] + g[v - 1, u + 1])
            A += ix * ix
            B += iy * iy
            Cc += ix * iy
    return 25 * (A * B - Cc * Cc) - (A + B) ** 2


def quotas(shapes, N):
    """q_l of the plan [(h_l, w_l)]: floor(N weight_l / W) with weight_l = h_l + w_l, the remainder one each to levels 0 .. r - 1."""
    weight = [int(h) + int(w) for h, w in shapes]
    W = sum(weight)
    q = [int(N) * wl // W for wl in weight]
    r = int(N) - sum(q)
    assert 0 <= r < len(shapes)
    return [ql + (1 if l < r else 0) for l, ql in enumerate(q)]


def kept_per_level(M_l, q_l, N):
    """k_l: everything when the candidates number at most N; else from the coarsest level down, a short level hands its unused
    quota to the finer ones (what is left after level 0 is dropped)."""
    M_l = [int(m) for m in M_l]
    if sum(M_l) <= N:
        return M_l
    k, c = [0] * len(M_l), 0
    for l in range(len(M_l) - 1, -1, -1):
        k[l] = min(M_l[l], q_l[l] + c)
        c = q_l[l] + c - k[l]
    return k


def candidates(img, tb, NumLevels=1, ScaleFactor=1.2, MinContrast=0.2, MinQuality=0.1):
    """(desc, loc, aux, R int64 [n], shapes): fast_pyramid_mirror.extract's rows with the response of each."""
    desc, loc, aux = pmir.extract(img, tb, NumLevels, ScaleFactor, MinContrast, MinQuality)
    lv = pmir.planes(img, NumLevels, ScaleFactor, tb.margin)
    t = int(math.floor(MinContrast * 255))
    R = [np.zeros(0, np.int64)]
    for g in lv:
        ys, xs, _ = fmir.detect(g, t, *fmir.quality_rational(MinQuality), tb.margin)
        R.append(harris(g, ys, xs))
    R = np.concatenate(R)
    assert len(R) == len(desc)
    return desc, loc, aux, R, [p.shape for p in lv]


def rank_order(R):
    """Indices of one level's candidates in (R descending, index ascending) order."""
    return np.argsort(-np.asarray(R, np.int64), kind="stable")


def select(levels, R, shapes, N):
    """Ascending indices of the kept candidates; `levels` is the level of each candidate (ascending)."""
    levels = np.asarray(levels, np.int64)
    M_l = np.bincount(levels, minlength=len(shapes)).tolist()
    k_l = kept_per_level(M_l, quotas(shapes, N), N)
    keep, at = [np.zeros(0, np.int64)], 0
    for m, k in zip(M_l, k_l):
        keep.append(at + rank_order(R[at:at + m])[:k])
        at += m
    return np.sort(np.concatenate(keep))


def extract(img, tb, NumLevels=1, ScaleFactor=1.2, MinContrast=0.2, MinQuality=0.1, NumStrongest=1):
    """(desc uint8 [n, 64], loc float64 [n, 2], aux float32 [n, 4] = [score, bin, level, f32(R)]) of the kept rows, in ascending
    (level, row, col) order."""
    return pick(candidates(img, tb, NumLevels, ScaleFactor, MinContrast, MinQuality), NumStrongest)


def pick(cand, N):
    """extract's result from candidates()'s (which the tests compute once per image and share)."""
    if N < 1:
        raise ValueError("NumStrongest must be at least 1")
    desc, loc, aux, R, shapes = cand
    keep = select(aux[:, 2], R, shapes, N)
    out = aux[keep].copy()
    out[:, 3] = R[keep].astype(np.float32)   # (round to nearest)
    return desc[keep].copy(), loc[keep].copy(), out
