"""NumPy restatement of the Harris corner detector (DESIGN.md "Harris corner contract") -- test infrastructure, not a test.

Written from the contract, not from the kernel.  The level planes are fast_pyramid_mirror's, the response is
fast_strongest_mirror.harris at every pixel, the descriptors are fast_mirror's (FREAK) or orb_mirror's (ORB), and the selections
are fast_strongest_mirror.pick and uniform_mirror.fast_pick on ``candidates``.  What is added here is the dense response, the
strict 3 x 3 suppression inside the band, and the gate in Python integers (its products pass 2^64).  Everything is integer
arithmetic up to the one conversion of R to f32, so ``extract`` returns what ``aps_corner_extract`` returns with
corner = APS_CORNER_HARRIS, bit for bit.
"""
import numpy as np

import fast_mirror as fmir
import fast_pyramid_mirror as pmir
import fast_strongest_mirror as smir
import orb_mirror as om

REACH = smir.WINDOW + 1   # Sobel 1 + window 3: the pixels at least this far from every edge have a response
Q_DEN_MAX = 1 << 24


def quality_rational(MinQuality):
    """MinQuality as (num, den): a pair is taken as it is, a number as fast_mirror.quality_rational's num / 10^6."""
    q = tuple(int(v) for v in MinQuality) if isinstance(MinQuality, (tuple, list)) else fmir.quality_rational(MinQuality)
    assert 0 <= q[0] <= q[1] <= Q_DEN_MAX and q[1] > 0
    return q


def dense(plane):
    """int64 [h, w]: R at every pixel at least REACH from each edge, 0 elsewhere (what aps_harris_planes reports for a level)."""
    g = np.asarray(plane, np.int64)
    h, w = g.shape
    R = np.zeros((h, w), np.int64)
    if h >= 2 * REACH + 1 and w >= 2 * REACH + 1:
        ys, xs = np.mgrid[REACH:h - REACH, REACH:w - REACH]
        R[REACH:h - REACH, REACH:w - REACH] = smir.harris(g, ys.ravel(), xs.ravel()).reshape(ys.shape)
    return R


def suppress(R, margin):
    """bool [h, w]: the band pixels with R > 0 and R strictly above all eight neighbours' R (the neighbours just outside the band
    count with their own R; margin >= REACH + 1 gives every one of them a full window)."""
    assert margin >= REACH + 1
    h, w = R.shape
    keep = np.zeros((h, w), bool)
    if h < 2 * margin + 1 or w < 2 * margin + 1:
        return keep
    band = (slice(margin, h - margin), slice(margin, w - margin))
    c = R[band]
    k = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dy, dx) != (0, 0):
                k &= c > R[margin + dy:h - margin + dy, margin + dx:w - margin + dx]
    keep[band] = k
    return keep


def gate(Rc, q_num, q_den):
    """bool per candidate: R q_den >= Rmax q_num in exact (Python) integers, Rmax the largest of the candidates' R."""
    Rc = [int(v) for v in Rc]
    top = max(Rc, default=0)
    return np.array([r * q_den >= top * q_num for r in Rc], bool)


def detect(plane, q_num, q_den, margin):
    """(ys, xs, R int64) of one level plane in ascending (row, col) order, with the number of candidates before the gate."""
    R = dense(plane)
    ys, xs = np.nonzero(suppress(R, margin))
    ok = gate(R[ys, xs], q_num, q_den)
    return ys[ok], xs[ok], R[ys[ok], xs[ok]], len(ys)


def describe(g, ys, xs, descriptor, tb):
    """(bins, desc) of the level pixels: FREAK on the integral image with the tables tb, or ORB on the plane."""
    if descriptor == "ORB":
        width = om.BYTES
        if len(ys) == 0:
            return np.zeros(0, np.int64), np.zeros((0, width), np.uint8)
        bins = om.bin_of(*om.moments(g, ys, xs))
        return bins, om.describe(g, ys, xs, bins)
    assert descriptor == "FREAK"
    if len(ys) == 0:
        return np.zeros(0, np.int64), np.zeros((0, 64), np.uint8)
    I = fmir.integral(g)
    bins = fmir.orientation(I, ys, xs, tb)
    return bins, fmir.describe(I, ys, xs, bins, tb)


def candidates(img, tb, descriptor="FREAK", NumLevels=1, ScaleFactor=1.2, MinQuality=0.01):
    """(desc, loc, aux, R int64 [n], shapes) in the form of fast_strongest_mirror.candidates: the rows of the call without a
    selection, aux = [f32(R), bin, level, 0], in ascending (level, row, col) order."""
    margin = tb.margin
    assert margin == om.MARGIN
    qn, qd = quality_rational(MinQuality)
    lv = pmir.planes(img, NumLevels, ScaleFactor, margin)
    D, L, A, Rs = [], [], [], []
    for l, g in enumerate(lv):
        ys, xs, R, _ = detect(g, qn, qd, margin)
        bins, d = describe(g, ys, xs, descriptor, tb)
        aux = np.zeros((len(ys), 4), np.float32)
        aux[:, 0], aux[:, 1], aux[:, 2] = R.astype(np.float32), bins, l   # (int64 -> f32 rounds to nearest)
        D.append(d)
        L.append(pmir.loc_of(xs, ys, g.shape, lv[0].shape).reshape(-1, 2))
        A.append(aux)
        Rs.append(R)
    return np.concatenate(D), np.concatenate(L), np.concatenate(A), np.concatenate(Rs), [p.shape for p in lv]


def extract(img, tb, descriptor="FREAK", NumLevels=1, ScaleFactor=1.2, MinQuality=0.01):
    """(desc uint8 [n, 64 | 32], loc float64 [n, 2] 1-based [x y] in level-0 coordinates, aux float32 [n, 4])."""
    return candidates(img, tb, descriptor, NumLevels, ScaleFactor, MinQuality)[:3]


def dense_planes(img, NumLevels, ScaleFactor, margin):
    """int64, the levels' dense R one after the other, each row-major: aps_harris_planes' output."""
    return np.concatenate([dense(g).ravel() for g in pmir.planes(img, NumLevels, ScaleFactor, margin)])
