"""NumPy restatement of the FAST/ORB contract (DESIGN.md "FAST/ORB contract") -- test infrastructure, not a test.

Written from the contract, not from the kernel.  Candidates, levels and selection are those of the FAST/FREAK mirrors
(fast_mirror, fast_pyramid_mirror, fast_strongest_mirror, uniform_mirror: the candidate set does not depend on the descriptor);
what is added here is ORB's own half: the generated test pattern, the steering tables, the intensity-centroid moments, the bin
and the 256-bit descriptor.  Everything is integer arithmetic (int64 here), so ``extract`` returns what ``aps_fast_orb_extract``
returns, bit for bit.
"""
import functools
import math

import numpy as np

import fast_mirror as fmir
import fast_pyramid_mirror as pmir
import fast_strongest_mirror as smir

N_TESTS, N_BINS, BYTES = 256, 256, 32
MARGIN = 23          # FREAK's: the candidate set is that of the FAST/FREAK entries
DISC_R2, TEST_R2 = 225, 169
REACH = 16           # 13 (steered point) + 2 (5 x 5 box) + 1


def generate_tests():
    """(tests int64 [256, 4] = (xa, ya, xb, yb), number of draws): the contract's generator."""
    s, draws = 1, 0

    def draw():
        nonlocal s, draws
        s = (1103515245 * s + 12345) % (1 << 31)
        draws += 1
        return ((s >> 16) % 27) - 13

    tests, seen = [], set()
    while len(tests) < N_TESTS:
        xa, ya, xb, yb = draw(), draw(), draw(), draw()
        if xa * xa + ya * ya > TEST_R2 or xb * xb + yb * yb > TEST_R2:
            continue
        if (xa - xb) ** 2 + (ya - yb) ** 2 < 16:
            continue
        key = frozenset(((xa, ya), (xb, yb)))
        if key in seen:
            continue
        seen.add(key)
        tests.append((xa, ya, xb, yb))
    return np.array(tests, np.int64), draws


def cos_sin():
    """[256, 2]: floor(2^14 (cos, sin)(2 pi k / 256) + 0.5) for k < 64, exact quarter turns beyond (FREAK's table)."""
    cs = np.zeros((N_BINS, 2), np.int64)
    for k in range(64):
        c = int(math.floor(16384.0 * math.cos(2.0 * math.pi * k / 256.0) + 0.5))
        s = int(math.floor(16384.0 * math.sin(2.0 * math.pi * k / 256.0) + 0.5))
        for q in range(4):
            cs[k + 64 * q] = (c, s)
            c, s = -s, c
    return cs


def steer(tests, cs):
    """[256 bins, 256 tests, 4]: bins 0..63 by the rounded rotation, 64..255 exact quarter turns (dx, dy) -> (-dy, dx)."""
    table = np.zeros((N_BINS, N_TESTS, 4), np.int64)
    for k in range(64):
        c, s = int(cs[k, 0]), int(cs[k, 1])
        pts = []
        for j in (0, 2):
            x, y = tests[:, j], tests[:, j + 1]
            pts.append(((x * c - y * s + (1 << 13)) >> 14, (x * s + y * c + (1 << 13)) >> 14))   # (arithmetic shift)
        for q in range(4):
            table[k + 64 * q] = np.stack([pts[0][0], pts[0][1], pts[1][0], pts[1][1]], 1)
            pts = [(-dy, dx) for dx, dy in pts]
    return table


def disc():
    """[709, 2] (u, v) with u^2 + v^2 <= 225, in ascending (v, u) order."""
    return np.array([(u, v) for v in range(-15, 16) for u in range(-15, 16) if u * u + v * v <= DISC_R2], np.int64)


@functools.lru_cache(maxsize=None)
def pattern():
    """(tests [256, 4], table [256, 256, 4], disc [709, 2], cos_sin [256, 2]), read-only."""
    tests, _ = generate_tests()
    cs = cos_sin()
    out = (tests, steer(tests, cs), disc(), cs)
    for a in out:
        a.setflags(write=False)
    return out


def reach(table):
    return int(np.abs(table).max()) + 2 + 1


def moments(g, ys, xs):
    """(m10, m01) per keypoint: sums of u g[y + v, x + u] and v g[y + v, x + u] over the disc."""
    g = np.asarray(g, np.int64)
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    d = pattern()[2]
    P = g[ys[:, None] + d[None, :, 1], xs[:, None] + d[None, :, 0]]
    return (P * d[None, :, 0]).sum(1), (P * d[None, :, 1]).sum(1)


def bin_of(m10, m01):
    """The bin 0..255 that maximises m10 c_k + m01 s_k (ties to the lower bin; a zero moment gives bin 0)."""
    cs = pattern()[3]
    proj = np.asarray(m10, np.int64)[:, None] * cs[None, :, 0] + np.asarray(m01, np.int64)[:, None] * cs[None, :, 1]
    return np.argmax(proj, axis=1).astype(np.int64)   # (argmax returns the first of equals)


def box5(g):
    """S[y, x] = the 5 x 5 box sum of g centred on (y, x), for 2 <= y < h - 2, 2 <= x < w - 2 (0 elsewhere)."""
    g = np.asarray(g, np.int64)
    h, w = g.shape
    I = fmir.integral(g)
    S = np.zeros((h, w), np.int64)
    S[2:h - 2, 2:w - 2] = I[5:, 5:] - I[:-5, 5:] - I[5:, :-5] + I[:-5, :-5]
    return S


def describe(g, ys, xs, bins):
    """[n, 32] uint8: bit i = S(a_i) < S(b_i) on the table of the keypoint's bin, LSB first in byte i // 8."""
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    S = box5(g)
    t = pattern()[1][np.asarray(bins, np.int64)]   # [n, 256, 4]
    a = S[ys[:, None] + t[..., 1], xs[:, None] + t[..., 0]]
    b = S[ys[:, None] + t[..., 3], xs[:, None] + t[..., 2]]
    return np.packbits((a < b).astype(np.uint8).reshape(len(ys), BYTES, 8), axis=2, bitorder="little").reshape(len(ys), BYTES)


def level_rows(g, MinContrast, MinQuality):
    """(ys, xs, scores, bins, desc) of one level plane, in ascending (row, col) order."""
    g = np.asarray(g, np.int64)
    ys, xs, sc = fmir.detect(g, int(math.floor(MinContrast * 255)), *fmir.quality_rational(MinQuality), MARGIN)
    if len(ys) == 0:
        return ys, xs, sc, np.zeros(0, np.int64), np.zeros((0, BYTES), np.uint8)
    bins = bin_of(*moments(g, ys, xs))
    return ys, xs, sc, bins, describe(g, ys, xs, bins)


def extract(img, NumLevels=1, ScaleFactor=1.2, MinContrast=0.2, MinQuality=0.1):
    """(desc uint8 [n, 32], loc float64 [n, 2] 1-based [x y] in level-0 coordinates, aux float32 [n, 4] = [score, bin, level, 0]),
    in ascending (level, row, col) order."""
    lv = pmir.planes(img, NumLevels, ScaleFactor, MARGIN)
    D, L, A = [np.zeros((0, BYTES), np.uint8)], [np.zeros((0, 2), np.float64)], [np.zeros((0, 4), np.float32)]
    for l, g in enumerate(lv):
        ys, xs, sc, bins, d = level_rows(g, MinContrast, MinQuality)
        aux = np.zeros((len(ys), 4), np.float32)
        aux[:, 0], aux[:, 1], aux[:, 2] = sc, bins, l
        D.append(d)
        L.append(pmir.loc_of(xs, ys, g.shape, lv[0].shape).reshape(-1, 2))
        A.append(aux)
    return np.concatenate(D), np.concatenate(L), np.concatenate(A)


def candidates(img, NumLevels=1, ScaleFactor=1.2, MinContrast=0.2, MinQuality=0.1):
    """(desc, loc, aux, R int64 [n], shapes): extract's rows with the Harris response of each, in the form of
    fast_strongest_mirror.candidates - fast_strongest_mirror.pick and uniform_mirror.fast_pick select from it as they do from FREAK's."""
    desc, loc, aux = extract(img, NumLevels, ScaleFactor, MinContrast, MinQuality)
    lv = pmir.planes(img, NumLevels, ScaleFactor, MARGIN)
    R = [np.zeros(0, np.int64)]
    for g in lv:
        ys, xs, _ = fmir.detect(g, int(math.floor(MinContrast * 255)), *fmir.quality_rational(MinQuality), MARGIN)
        R.append(smir.harris(g, ys, xs))
    R = np.concatenate(R)
    assert len(R) == len(desc)
    return desc, loc, aux, R, [p.shape for p in lv]


def load_pattern(capi):
    """(tests, table, disc, reach) as aps_orb_pattern reports them (needs the library, no device)."""
    import ctypes as C

    tests, table, dsc = np.zeros((N_TESTS, 4), np.int32), np.zeros((N_BINS, N_TESTS, 4), np.int32), np.zeros((709, 2), np.int32)
    r = C.c_int(0)
    capi.check(capi.lib.aps_orb_pattern(capi.ptr(tests), capi.ptr(table), capi.ptr(dsc), C.byref(r)))
    return tests.astype(np.int64), table.astype(np.int64), dsc.astype(np.int64), int(r.value)
