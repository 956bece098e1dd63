"""NumPy mirror of the max-weight multiband contract ("Max-weight multiband contract").

partition(W)      the weights b_k: 1.0 for the FIRST layer of maximal raw weight where that maximum is > 0, else 0.0
owner(W)          that layer's index per pixel, -1 where no weight is > 0
owner_colour(C, W) the owner's colour per pixel (0 where there is no owner)
pure_mask(B, ...) the pixels of one tile whose blended value is the owner's own sample up to float rounding: every weight
                  the pyramid multiplies into them is exactly 1 for the owner and exactly 0 for every other layer
paint(F, cov, white) the tiled renderer's uint8 rule (paint_kernel: roundf(255.0f * v), clamped; the canvas colour where
                  nothing covers)
"""
import numpy as np

import oracle


def owner(W):
    """W: K x h x w.  The compare is `w > best` from best = 0 in layer order: ties go to the first layer, a NaN, a zero and
    a negative weight never own."""
    W = np.asarray(W, np.float32)
    best = np.zeros(W.shape[1:], np.float32)
    own = np.full(W.shape[1:], -1, np.int64)
    for k in range(W.shape[0]):
        with np.errstate(invalid="ignore"):
            up = W[k] > best
        best = np.where(up, W[k], best)
        own = np.where(up, k, own)
    return own


def partition(W):
    own = owner(W)
    return (np.arange(np.asarray(W).shape[0])[:, None, None] == own[None]).astype(np.float32)


def owner_colour(C, W):
    """C: K x h x w x 3 -> h x w x 3, zeros where no layer owns the pixel."""
    own = owner(W)
    C = np.asarray(C, np.float32)
    out = np.take_along_axis(C, np.maximum(own, 0)[None, :, :, None], 0)[0]
    out[own < 0] = 0
    return out


def level_sizes(h, w, levels):
    """pyramid_levels (render_dev.h): L = max(1, min(levels, floor(log2(min(h, w))))), halving with floor."""
    L = max(1, min(int(levels), int(np.floor(np.log2(min(h, w))))))
    sizes = [(h, w)]
    for _ in range(1, L):
        sizes.append((max(1, sizes[-1][0] // 2), max(1, sizes[-1][1] // 2)))
    return sizes


def pure_mask(B, levels, sigma):
    """B: K x h x w, the partition of ONE tile (pyramids are tile-local).  Every layer's binary mask goes down the pyramid's
    own weight chain, W_(l+1) = imresize(gaussfilt(W_l, sigma), size_(l+1)); each level is brought back to level 0 through the
    collapse's own resize chain (imresize level by level).  A pixel is pure when at EVERY level that upsampled weight is
    exactly 1 for its owner and exactly 0 for every other layer: then every band's numerator there is the owner's own
    Laplacian and the collapse telescopes to the owner's sample.  No distance is tuned: the reach follows from the taps."""
    B = np.asarray(B, np.float32)
    K, h, w = B.shape
    sizes = level_sizes(h, w, levels)
    own = owner(B)
    pure = own >= 0
    cur = [B[k] for k in range(K)]
    for l in range(len(sizes)):
        if l > 0:
            cur = [oracle.imresize(oracle.gaussfilt(c, sigma), sizes[l][0], sizes[l][1]) for c in cur]
        for k in range(K):
            up = cur[k]
            for m in range(l - 1, -1, -1):
                up = oracle.imresize(up, sizes[m][0], sizes[m][1])
            pure &= np.where(own == k, up == 1.0, up == 0.0)
    return pure


def paint(F, cov, white=False):
    """paint_kernel: uint8(roundf(255.0f * v)) with round half away from zero, clamped to [0, 255]; the canvas colour where
    cov is 0."""
    t = np.float32(255.0) * np.asarray(F, np.float32)
    r = np.trunc(t)
    r = r + np.sign(t) * (np.abs(t - r) >= 0.5)  # (t - r is exact in f32)
    with np.errstate(invalid="ignore"):
        r = np.where(r > 0, r, 0)
    out = np.minimum(r, 255).astype(np.uint8)
    out[~np.asarray(cov, bool)] = 255 if white else 0
    return out
