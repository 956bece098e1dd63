"""Seeded test images and NumPy restatements shared by the FAST/FREAK tests (helper, not a test)."""
import functools

import numpy as np

import fast_mirror as fmir


@functools.lru_cache(maxsize=None)
def tables():
    """The integer pattern tables as aps_freak_pattern reports them (library, no device)."""
    import apsamd

    return fmir.load_tables(apsamd._capi)


def noise_rects(seed, h, w, channels=1, n_rects=None):
    """uint8 h x w (x channels): seeded uniform noise blended half and half with filled rectangles of random gray."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(channels):
        base = rng.integers(0, 256, (h, w)).astype(np.float64)
        rect = np.full((h, w), 128.0)
        for _ in range(n_rects if n_rects is not None else max(4, h * w // 600)):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            rect[y0:y0 + int(rng.integers(3, 24)), x0:x0 + int(rng.integers(3, 24))] = float(rng.integers(0, 256))
        out.append(np.clip(np.round(0.5 * base + 0.5 * rect), 0, 255).astype(np.uint8))
    return out[0] if channels == 1 else np.stack(out, -1)


def noise_lattice(seed, h=64, w=64, margin=23):
    """For an image whose admissible area (pixels at least `margin` from every edge) is too small for noise to carry 50
    keypoints: noise_rects outside, and over the admissible area (+3 for the rings) mid-gray 128 with the densest packing of
    strict 3 x 3 maxima, one keypoint per 2 x 2 pixels - single bright pixels at column pitch 2 and row pitch 4, single dark
    pixels on the same lattice shifted by (1 column, 2 rows).  No lattice offset (2a, 4b) is a ring offset, so every ring
    pixel of a bright pixel is gray or dark and of a dark pixel gray or bright: both score at least their own contrast, no
    two of them are neighbours, and a gray pixel never has 9 contiguous ring pixels on one side.  Contrasts are distinct
    per row and column, 60..127, so all pass the quality gate.  The descriptors still see the noise around the patch."""
    img = noise_rects(seed, h, w)
    img[margin - 3:h - margin + 3, margin - 3:w - margin + 3] = 128
    for y in range(margin, h - margin, 2):
        for x in range(margin + (y - margin) // 2 % 2, w - margin, 2):
            v = 60 + (7 * (y - margin) + 3 * (x - margin)) % 68
            img[y, x] = 128 + v if (y - margin) % 4 == 0 else 128 - v
    return img


def planted(h=150, w=200, margin=23):
    """Flat gray 20 with single bright pixels of distinct heights planted where the chain has seams: the four admissible
    corners, the first and last admissible row and column, both sides of the 8-row and 64-column tile seams (the latter are
    the seams of the 64-bit bitmap words too).  Planted pixels are at least 8 apart (Chebyshev), so none lies on another's
    ring or beside it: a single pixel v above a flat field scores exactly v - 20 (every ring pixel is darker by that much),
    no other pixel scores (its ring holds at most one bright pixel), and every planted pixel is a keypoint.
    Returns (image, [(row, col, score)] in ascending (row, col) order)."""
    lo_y, hi_y, lo_x, hi_x = margin, h - 1 - margin, margin, w - 1 - margin
    want = [(lo_y, lo_x), (lo_y, hi_x), (hi_y, lo_x), (hi_y, hi_x)]
    want += [(y, 40 + 9 * i) for i, y in enumerate([lo_y, 31, 32, 39, 40, 63, 64, 71, 72, 95, 96, hi_y])]
    want += [(36 + 9 * j, x) for j, x in enumerate([lo_x, 63, 64, 65, 127, 128, 129, hi_x])]
    pts = []
    for (y, x) in want:
        if lo_y <= y <= hi_y and lo_x <= x <= hi_x and all(max(abs(y - py), abs(x - px)) >= 8 for py, px, _ in pts):
            pts.append((y, x, 60 + 5 * len(pts)))   # scores 60, 65, ...: all above the default threshold 51 and the gate
    img = np.full((h, w), 20, np.uint8)
    for (y, x, s) in pts:
        img[y, x] = 20 + s
    return img, sorted(pts)


# ---- NumPy restatements of the reference's binary matching -------------------------------------------------------------
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(A, B):
    """[n1, n2] bit distances of packed rows."""
    return _POP[A[:, None, :] ^ B[None, :, :]].sum(-1)


def hamming_2nn(A, B):
    """nearest2HammingExhaustiveMEX's rule: best by strict <, second by <= (the first of equals is the nearest, the last
    candidate that ties the running second replaces it - the value is what matters); one candidate: second = 8 * nbytes."""
    D = hamming(A, B)
    n1, n2 = D.shape
    idx = np.argmin(D, 1)   # the first of equals
    d1 = D[np.arange(n1), idx]
    if n2 == 1:
        d2 = np.full(n1, 8 * A.shape[1], np.int64)
    else:
        D2 = D.copy()
        D2[np.arange(n1), idx] = 1 << 30
        d2 = D2.min(1)
    return (idx + 1).astype(np.uint32), d1.astype(np.float32), d2.astype(np.float32)


def match_binary(A, B, MaxRatio, MatchThreshold, Unique=True):
    """matchFeaturesScratch.m:81-211 for packed binary rows, in NumPy (single arithmetic where MATLAB has single)."""
    if len(A) == 0 or len(B) == 0:
        return np.zeros((0, 2), np.uint32), np.zeros(0, np.float32)
    nBits = np.float32(8 * A.shape[1])
    idx2, d1, d2 = hamming_2nn(A, B)
    d2 = np.where(~np.isfinite(d2) | (d2 == 0), nBits, d2).astype(np.float32)   # :318
    best, second = (d1 / nBits) * np.float32(100), (d2 / nBits) * np.float32(100)   # :120-121
    keep = (best <= np.float32(MaxRatio) * second) & (best <= np.float32(MatchThreshold)) & np.isfinite(best) & np.isfinite(second)
    i1, i2, d = np.flatnonzero(keep) + 1, idx2[keep], best[keep]
    if Unique and len(i1):
        order = np.argsort(d, kind="stable")
        used1, used2, sel = set(), set(), []
        for k in order:
            if i1[k] not in used1 and i2[k] not in used2:
                used1.add(i1[k])
                used2.add(i2[k])
                sel.append(k)
        sel = np.array(sel, np.int64)
        i1, i2, d = i1[sel], i2[sel], d[sel]
    return np.stack([i1, i2], 1).astype(np.uint32), d.astype(np.float32)


def global_binary(sets, ratio, k):
    """featureMatchingGlobal.m:54-161 for packed binary sets, in NumPy: {(i, j): [[li, lj], ...]} with 0-based image ids and
    1-based local indices, in query order.  k-NN: ascending distance, ties to the lower index (the device search's rule)."""
    counts = [len(s) for s in sets]
    pool = np.concatenate([s for s in sets if len(s)])
    img = np.repeat(np.arange(len(sets)), counts)
    local = np.concatenate([np.arange(1, c + 1) for c in counts])
    D = hamming(pool, pool)
    out = {}
    eps = np.float32(np.finfo(np.float32).eps)
    for q in range(len(pool)):
        nn = np.argsort(D[q], kind="stable")[:k]
        nn = nn[nn != q]
        nn = nn[img[nn] != img[q]]
        if len(nn) < 2:
            continue
        d1, d2 = np.float32(D[q, nn[0]]), np.float32(D[q, nn[1]])
        if d1 / max(d2, eps) > np.float32(ratio):
            continue
        qi, j = int(img[q]), int(img[nn[0]])
        if qi < j:
            out.setdefault((qi, j), []).append([local[q], local[nn[0]]])
        else:
            out.setdefault((j, qi), []).append([local[nn[0]], local[q]])
    return {key: np.array(v, np.float64) for key, v in out.items()}


@functools.lru_cache(maxsize=None)
def scene():
    """Three overlapping 240 x 320 views of the procedural world (CPU rendering, so the CPU check and the device see the same
    bytes) and their intrinsics."""
    from importlib import import_module

    import apsamd

    synth = import_module(apsamd.__name__ + ".synth")
    w, h, f = 320, 240, 450.0
    cams = synth.grid_cameras(3, 1, w, h, f, 2 * np.arctan(w / (2 * f)) * 0.3, 0.0, 1.0, 7)
    views = [np.ascontiguousarray(np.asarray(synth.render_view(cams[i], h, w, 7, "cpu", finest_px=1.0))) for i in range(3)]
    return views, cams
