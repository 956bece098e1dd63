"""Seeded test images of the Harris corner tests (helper, not a test): the smallest images that reach each risk of the chain.

Tiles are 64 x 8 pixels from the plane's origin and the band starts 23 pixels from every edge, so the seams inside the band lie at
x = 63 | 64, 127 | 128 and at y = 23 | 24, 31 | 32, 39 | 40.
"""
import functools
from collections import namedtuple

import numpy as np

MARGIN = 23

# build: () -> uint8 image; quality: MinQuality as a number or an exact (num, den); min_rows: the least number of rows the case must
# yield - 8 wherever the construction does not bound the count, 0 where no row may come out
Case = namedtuple("Case", "build levels scale quality min_rows")


def lattice(seed, h, w, y_anchor=MARGIN, x_anchor=MARGIN, period=8, amp=(20, 62)):
    """Square pyramids of side `period`, apex on (y_anchor + period i, x_anchor + period j), of seeded heights.  The box window of
    the response makes the corners of a block plateaus several pixels wide and keeps strict maxima at least a window apart, so a band
    of a few rows holds too few block corners; an apex is the strict maximum of its own 3 x 3 (the window there sees the four faces
    in equal parts, and one pixel aside it does not), which puts rows exactly on chosen pixels: the one-pixel band, the single band
    row, the last band row and column, and the pixels on both sides of a seam."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    r = period // 2
    dy, dx = (y - y_anchor + r) % period - r, (x - x_anchor + r) % period - r
    cy, cx = (y - y_anchor + r) // period, (x - x_anchor + r) // period
    height = rng.integers(amp[0], amp[1] + 1, (h // period + 3, w // period + 3))
    return np.clip(height[cy + 1, cx + 1] * (r - np.maximum(abs(dy), abs(dx))), 0, 255).astype(np.uint8)


def blocks(seed, h, w, n=None, noise=6):
    """Axis-aligned blocks of random gray on gray 110 with seeded noise of `noise` levels, which breaks the ties of a box window;
    6 x 6 blocks have a corner on each seam of the tiling inside the band, alternately on either side of it."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 110, np.int64)
    for _ in range(n if n is not None else max(6, h * w // 400)):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[y0:y0 + int(rng.integers(4, 20)), x0:x0 + int(rng.integers(4, 20))] = int(rng.integers(0, 256))
    for k, y in enumerate(range(32, h - MARGIN, 8)):
        for j, x in enumerate(range(64, w - MARGIN, 64)):
            img[y - (k & 1):y - (k & 1) + 6, x - (j & 1):x - (j & 1) + 6] = 250 - 60 * ((k + j) & 1)
    img += rng.integers(0, noise + 1, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def blocks_and_seams(seed, h, w):
    """blocks() with a patch of lattice() whose apexes lie on the far side of the seams: (32, 64), (32, 72), (40, 64), (40, 72)."""
    img = blocks(seed, h, w)
    img[26:47, 58:79] = lattice(seed, h, w, 32, 64, amp=(40, 62))[26:47, 58:79]
    return img


def saturated(seed, h, w):
    """0 / 255 blocks only: the responses reach their largest values, so Rmax * q_num passes 2^64 with a denominator of 2^24."""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.uint8)
    for _ in range(h * w // 150):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[y0:y0 + int(rng.integers(3, 15)), x0:x0 + int(rng.integers(3, 15))] = 255 * int(rng.integers(0, 2))
    return img


def step_edge(h=64, w=96):
    """A pure vertical step: Iy = 0 everywhere, so A B - C^2 = 0 and R = -(A + B)^2 <= 0."""
    img = np.full((h, w), 30, np.uint8)
    img[:, w // 2:] = 220
    return img


def plateau(h=80, w=81):
    """An h x (w - 1) plane mirrored about the boundary between its two middle columns: R(y, x) = R(y, w - 2 - x), so the two pixels
    next to the axis tie.  A bright 6 x 6 block straddles the axis: its response peaks on the axis' two columns, and neither pixel
    of such a pair may be kept."""
    half = blocks(41, h, (w - 1) // 2, n=4)
    half[36:42, -3:] = 255
    return np.concatenate([half, half[:, ::-1]], 1)


THIRD = (5592405, 16777215)   # 1 / 3 exactly, on a denominator just below 2^24

CASES = {
    "47x47": Case(lambda: lattice(3, 47, 47), 1, 1.2, 0.01, 1),          # the band is one pixel: the apex on it is the one row
    "47x129": Case(lambda: lattice(3, 47, 129), 1, 1.2, 0.01, 8),        # one band row, a 64-column seam, partial tiles
    "55x64": Case(lambda: lattice(3, 55, 64), 1, 1.2, 0.01, 8),          # one tile column; the 8-row seam 31 | 32 ends the band
    "63x65": Case(lambda: lattice(3, 63, 65), 1, 1.2, 0.01, 8),          # a second tile column of one pixel
    "70x200": Case(lambda: blocks_and_seams(5, 70, 200), 1, 1.2, 0.01, 8),   # seams at 63 | 64 and 127 | 128, 31 | 32 and 39 | 40
    "constant": Case(lambda: np.full((60, 70), 93, np.uint8), 1, 1.2, 0.01, 0),
    "edge": Case(step_edge, 1, 1.2, 0.01, 0),
    "plateau": Case(plateau, 1, 1.2, 0.01, 1),
    "saturated_top": Case(lambda: saturated(6, 80, 120), 1, 1.2, ((1 << 24) - 1, 1 << 24), 1),   # only Rmax itself passes
    "saturated_third": Case(lambda: saturated(7, 80, 120), 1, 1.2, THIRD, 8),
    "pyramid": Case(lambda: blocks(8, 96, 128), 3, 1.2, 0.01, 8),
}
DEGENERATE = ("constant", "edge")
SATURATED = ("saturated_top", "saturated_third")


@functools.lru_cache(maxsize=None)
def image(name):
    img = CASES[name].build()
    img.setflags(write=False)
    return img
