"""NumPy restatement of the FAST/FREAK contract (DESIGN.md "FAST/FREAK contract") -- test infrastructure, not a test.

Written from the contract, not from the kernel.  Everything is integer arithmetic (int64 here), so ``extract`` returns what
``aps_fast_extract`` returns, bit for bit.  The integer pattern tables are an argument (``Tables``): the tests hand in what
``aps_freak_pattern`` reports; ``contract_tables`` evaluates the contract's f64 layout itself, for the table tests.
"""
import math
from collections import namedtuple

import numpy as np

# fields [256, 43, 3] (dx, dy, r); pairs [512, 2]; ori_pairs [45, 2]; ori_dir [45, 2]; cos_sin [256, 2]; margin
Tables = namedtuple("Tables", "fields pairs ori_pairs ori_dir cos_sin margin")

# the 16-pixel Bresenham circle of radius 3, clockwise from the top (x right, y down): (dx, dy)
RING = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3)]
N_FIELDS, SCALE = 43, 22.0


def ring_of(f):
    return f // 6 if f < 42 else 7


def layout0():
    """The f64 layout at orientation 0: (x, y, sigma) per field, in pixels."""
    bigR, smallR = 2.0 / 3.0, 2.0 / 24.0
    u = (bigR - smallR) / 21.0
    radius = [bigR - s * u for s in (0, 6, 11, 15, 18, 20)] + [smallR]
    out = []
    for f in range(42):
        r, j = divmod(f, 6)
        th = j * math.pi / 3.0 + (r & 1) * math.pi / 6.0
        out.append((radius[r] * SCALE * math.cos(th), radius[r] * SCALE * math.sin(th), radius[r] / 2.0 * SCALE))
    out.append((0.0, 0.0, smallR / 2.0 * SCALE))
    return out


def _rhu(v):
    return int(math.floor(v + 0.5))


def contract_tables():
    """The integer tables as the contract derives them from the f64 layout."""
    bigR, smallR = 2.0 / 3.0, 2.0 / 24.0
    u = (bigR - smallR) / 21.0
    radius = [bigR - s * u for s in (0, 6, 11, 15, 18, 20)] + [smallR, 0.0]
    fields = np.zeros((256, N_FIELDS, 3), np.int64)
    cs = np.zeros((256, 2), np.int64)
    for k in range(64):
        for f in range(N_FIELDS):
            r, j = ring_of(f), f % 6
            th = (j * math.pi / 3.0 + (r & 1) * math.pi / 6.0 if f < 42 else 0.0) + 2.0 * math.pi * k / 256.0
            dx = _rhu(radius[r] * SCALE * math.cos(th)) if f < 42 else 0
            dy = _rhu(radius[r] * SCALE * math.sin(th)) if f < 42 else 0
            hs = _rhu((radius[r] if f < 42 else smallR) / 2.0 * SCALE)
            for q in range(4):  # exact quarter turns
                fields[k + 64 * q, f] = (dx, dy, hs)
                dx, dy = -dy, dx
        c, s = _rhu(16384.0 * math.cos(2.0 * math.pi * k / 256.0)), _rhu(16384.0 * math.sin(2.0 * math.pi * k / 256.0))
        for q in range(4):
            cs[k + 64 * q] = (c, s)
            c, s = -s, c
    allp = sorted(((ring_of(a) + ring_of(b), a, b) for a in range(N_FIELDS) for b in range(a + 1, N_FIELDS)))
    pairs = np.array([(a, b) for _, a, b in allp[:512]], np.int64)
    l0 = layout0()
    op, od = [], []
    for r in range(3):
        for a in range(6 * r, 6 * r + 6):
            for b in range(a + 1, 6 * r + 6):
                ex, ey = l0[a][0] - l0[b][0], l0[a][1] - l0[b][1]
                n = math.sqrt(ex * ex + ey * ey)
                op.append((a, b))
                od.append((_rhu(1024.0 * ex / n), _rhu(1024.0 * ey / n)))
    margin = int((np.maximum(np.abs(fields[..., 0]), np.abs(fields[..., 1])) + fields[..., 2] + 1).max())
    return Tables(fields, pairs, np.array(op, np.int64), np.array(od, np.int64), cs, margin)


def gray_plane(img):
    """rgb2gray's integer plane (0..255); a gray input is passed through."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.astype(np.int64)
    d = 0.298936021293775 * img[..., 0].astype(np.float64) + 0.587043074451121 * img[..., 1].astype(np.float64)
    d = d + 0.114020904255103 * img[..., 2].astype(np.float64)
    return np.floor(d + 0.5).astype(np.int64)


def integral(gray):
    """(h+1) x (w+1), I[y+1][x+1] = sum of gray[0..y][0..x]; exact integers."""
    h, w = gray.shape
    if h * w * 255 >= 2 ** 32:
        raise ValueError("image exceeds the 32-bit integral image")
    I = np.zeros((h + 1, w + 1), np.int64)
    I[1:, 1:] = np.cumsum(np.cumsum(gray.astype(np.int64), 0), 1)
    return I


def box(I, r0, r1, c0, c1):
    """Sum over rows r0..r1, columns c0..c1 (inclusive); index arrays broadcast."""
    return I[r1 + 1, c1 + 1] - I[r0, c1 + 1] - I[r1 + 1, c0] + I[r0, c0]


def scores(gray, t, margin):
    """The FAST-9 score plane: s where s > t and the pixel is at least `margin` from every edge, else 0."""
    h, w = gray.shape
    S = np.zeros((h, w), np.int64)
    if h < 2 * margin + 1 or w < 2 * margin + 1:
        return S
    ys, xs = slice(margin, h - margin), slice(margin, w - margin)
    ctr = gray[ys, xs]
    d = np.stack([gray[margin + dy:h - margin + dy, margin + dx:w - margin + dx] - ctr for dx, dy in RING])  # ring - centre
    best = None
    for a in range(16):
        arc = d[[(a + j) % 16 for j in range(9)]]
        v = np.maximum(arc.min(0), (-arc).min(0))
        best = v if best is None else np.maximum(best, v)
    S[ys, xs] = np.where(best > t, best, 0)
    return S


def suppress(S):
    """Keep a corner iff its score is strictly greater than all 8 neighbours'."""
    h, w = S.shape
    P = np.zeros((h + 2, w + 2), np.int64)
    P[1:-1, 1:-1] = S
    keep = S > 0
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                keep &= S > P[dy:dy + h, dx:dx + w]
    return np.where(keep, S, 0)


def detect(gray, t, q_num, q_den, margin):
    """Keypoints (rows, cols, scores) in ascending (row, col) order."""
    K = suppress(scores(gray, t, margin))
    smax = int(K.max()) if K.size else 0
    ok = (K > 0) & (K * q_den >= smax * q_num)
    ys, xs = np.nonzero(ok)
    return ys, xs, K[ys, xs]


def field_sums(I, ys, xs, tab):
    """[n, 43] box sums; tab is [43, 3] for all keypoints or [n, 43, 3] per keypoint."""
    tab = np.broadcast_to(tab, (len(ys),) + tab.shape[-2:])
    cy, cx, r = ys[:, None] + tab[..., 1], xs[:, None] + tab[..., 0], tab[..., 2]
    return box(I, cy - r, cy + r, cx - r, cx + r)


def moment(I, ys, xs, tb):
    """(Mx, My) per keypoint: the 45 pairs on the orientation-0 table."""
    S = field_sums(I, ys, xs, tb.fields[0])
    area = (2 * tb.fields[0][:, 2] + 1) ** 2
    a, b = tb.ori_pairs[:, 0], tb.ori_pairs[:, 1]
    D = S[:, a] * area[b] - S[:, b] * area[a]
    return (D * tb.ori_dir[:, 0]).sum(1), (D * tb.ori_dir[:, 1]).sum(1)


def bin_of(mx, my, tb):
    """The bin 0..255 that maximises Mx c_k + My s_k (ties to the lower bin; a zero moment gives bin 0)."""
    mx, my = np.asarray(mx, np.int64), np.asarray(my, np.int64)
    proj = mx[:, None] * tb.cos_sin[:, 0][None, :] + my[:, None] * tb.cos_sin[:, 1][None, :]
    return np.argmax(proj, axis=1).astype(np.int64)  # (argmax returns the first of equals)


def orientation(I, ys, xs, tb):
    """The bin 0..255 per keypoint."""
    return bin_of(*moment(I, ys, xs, tb), tb)


def describe(I, ys, xs, bins, tb):
    """[n, 64] uint8: bit i = mean(a_i) > mean(b_i) on the table of the keypoint's bin, LSB first in byte i // 8."""
    S = field_sums(I, ys, xs, tb.fields[bins])
    area = (2 * tb.fields[0][:, 2] + 1) ** 2
    a, b = tb.pairs[:, 0], tb.pairs[:, 1]
    bits = (S[:, a] * area[b] > S[:, b] * area[a]).astype(np.uint8)
    return np.packbits(bits.reshape(len(ys), 64, 8), axis=2, bitorder="little").reshape(len(ys), 64)


def quality_rational(MinQuality):
    """MinQuality as (num, den) with den = 10^6."""
    return int(round(float(MinQuality) * 1000000)), 1000000


def extract(img, tb, MinContrast=0.2, MinQuality=0.1):
    """(desc uint8 [n, 64], loc float64 [n, 2] 1-based [x y], aux float32 [n, 4] = [score, bin, 0, 0])."""
    gray = gray_plane(img)
    t = int(math.floor(MinContrast * 255))
    qn, qd = quality_rational(MinQuality)
    ys, xs, sc = detect(gray, t, qn, qd, tb.margin)
    n = len(ys)
    if n == 0:
        return np.zeros((0, 64), np.uint8), np.zeros((0, 2), np.float64), np.zeros((0, 4), np.float32)
    I = integral(gray)
    bins = orientation(I, ys, xs, tb)
    desc = describe(I, ys, xs, bins, tb)
    loc = np.stack([xs + 1, ys + 1], 1).astype(np.float64)
    aux = np.zeros((n, 4), np.float32)
    aux[:, 0], aux[:, 1] = sc, bins
    return desc, loc, aux


def load_tables(capi):
    """Tables as aps_freak_pattern reports them (needs the library, no device)."""
    import ctypes as C

    fields = np.zeros((256, N_FIELDS, 3), np.int32)
    pairs, op, od, cs = np.zeros((512, 2), np.int32), np.zeros((45, 2), np.int32), np.zeros((45, 2), np.int32), np.zeros((256, 2), np.int32)
    margin = C.c_int(0)
    capi.check(capi.lib.aps_freak_pattern(capi.ptr(fields), capi.ptr(pairs), capi.ptr(op), capi.ptr(od), capi.ptr(cs), C.byref(margin)))
    return Tables(*(a.astype(np.int64) for a in (fields, pairs, op, od, cs)), int(margin.value))
