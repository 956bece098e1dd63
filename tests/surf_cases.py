"""Seeded NumPy test images of the SURF tests (helper, not a test): band-limited noise and the frozen homography pair."""
import functools

import numpy as np


def band_limited(seed, h, w, sigma=3.0, contrast=1.0, channels=1):
    """uint8 h x w (x channels) noise, low-passed by a Gaussian of `sigma` pixels in the Fourier domain (periodic), stretched
    to the full gray range; `contrast` < 1 pulls it towards mid gray."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(channels):
        n = rng.standard_normal((h, w))
        fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
        g = np.exp(-2.0 * (np.pi * sigma) ** 2 * (fx * fx + fy * fy))
        f = np.real(np.fft.ifft2(np.fft.fft2(n) * g))
        f = (f - f.min()) / (f.max() - f.min())
        out.append(np.clip(np.round(255.0 * (0.5 + contrast * (f - 0.5))), 0, 255).astype(np.uint8))
    return out[0] if channels == 1 else np.stack(out, -1)


# the frozen pair: image A, the homography (0-based pixel coordinates, x' ~ H x maps A to B) and image B = A warped by it
PAIR_H = np.array([[1.02, 0.03, 6.0], [-0.025, 0.99, 4.0], [4e-5, -3e-5, 1.0]])


def warp_bilinear(img, H, fill=128):
    """B[y', x'] = A at H^-1 (x', y'), bilinear; outside A: `fill`."""
    h, w = img.shape
    Hi = np.linalg.inv(H)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = Hi[2, 0] * xx + Hi[2, 1] * yy + Hi[2, 2]
    sx = (Hi[0, 0] * xx + Hi[0, 1] * yy + Hi[0, 2]) / d
    sy = (Hi[1, 0] * xx + Hi[1, 1] * yy + Hi[1, 2]) / d
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    ok = (x0 >= 0) & (y0 >= 0) & (x0 + 1 < w) & (y0 + 1 < h)
    x0c, y0c = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    ax, ay = sx - x0, sy - y0
    a = img.astype(np.float64)
    v = ((1 - ay) * ((1 - ax) * a[y0c, x0c] + ax * a[y0c, x0c + 1]) + ay * ((1 - ax) * a[y0c + 1, x0c] + ax * a[y0c + 1, x0c + 1]))
    return np.where(ok, np.clip(np.round(v), 0, 255), fill).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pair():
    """(A, B) 240 x 320 uint8."""
    A = band_limited(2024, 240, 320, sigma=2.5)
    B = warp_bilinear(A, PAIR_H)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def transfer_error(locA, locB, H=PAIR_H):
    """Distance (pixels) between H applied to A's 1-based points and B's 1-based points."""
    p = np.concatenate([locA - 1.0, np.ones((len(locA), 1))], 1) @ H.T
    return np.hypot(p[:, 0] / p[:, 2] - (locB[:, 0] - 1.0), p[:, 1] / p[:, 2] - (locB[:, 1] - 1.0))


def ratio_matches(dA, dB, ratio=0.6):
    """Brute-force 2-NN ratio test on squared distances (ratio^2), NumPy; returns index pairs [k, 2] (0-based)."""
    d2 = ((dA.astype(np.float64)[:, None, :] - dB.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    order = np.argsort(d2, 1)
    best, second = order[:, 0], order[:, 1]
    r = np.arange(len(dA))
    keep = d2[r, best] <= ratio * ratio * d2[r, second]
    return np.stack([r[keep], best[keep]], 1)
