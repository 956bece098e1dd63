"""The FAST/FREAK parameter matrix of test_fast_params_gpu.py (helper, not a test): the parameter sets, the edge of
fast_detect_kernel / fast_gate_kernel each one is there for, and the mirror's keypoints on the CPU.

What the rest of the suite runs is MinContrast in {0.05, 0.1, 0.2} with MinQuality 0.1 = 100000 / 1000000.  The edges that
set never touches (csrc/fast.hip):
  fast_gate_kernel    `s * q_den >= smax * q_num` with q_num = 0 (everything that survived suppression), q_num = q_den (ties
                      with the maximum only), q_den at the ABI's bound 2^24 (with s = 255 the product is 255 * 2^24, above
                      2^31), and a ratio for which smax * q_num / q_den is exactly a score of the image (`>=` keeps it)
  fast_detect_kernel  `s <= thr` at thr = 0 (the densest plane) and thr = 255 (nothing is left, not even a score of 255)
  the score plane     a corner of score 255, the top of uint8
test_fast_param_cases.py holds every case to the edge it is named for and to at least 50 keypoints.

fast_cases.planted() carries 22 corners, below that floor: it is the base of no case here."""
import functools
import math
from collections import namedtuple

import numpy as np

import fast_cases as fc
import fast_mirror as fmir

FLOOR = 50
DEN_MAX = 1 << 24   # aps_fast_extract refuses a larger quality_den


def black_white_rects(seed=5, h=120, w=160, n_rects=1500):
    """uint8 h x w of 0 and 255 only: seeded rectangles, 1..7 pixels a side, black or white, painted over each other on black.
    Every ring difference is 0 or +-255, so every FAST score is 0 or 255: all corners sit at the top of the uint8 score plane.
    Corners that survive the strict 3 x 3 maximum are the isolated ones (two adjacent corners tie at 255 and both go)."""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.uint8)
    for _ in range(n_rects):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[y0:y0 + int(rng.integers(1, 8)), x0:x0 + int(rng.integers(1, 8))] = 255 * int(rng.integers(0, 2))
    return img


IMAGES = {
    "70x131": lambda: fc.noise_rects(13, 70, 131),    # tile and 64-bit word boundaries not aligned
    "100x140": lambda: fc.noise_rects(21, 100, 140),  # enough corners that half the maximum still leaves over 50
    "bw": black_white_rects,
}

# Wrapper cases give MinContrast / MinQuality (featureMatching.fast_extract turns them into the integers, the mirror does
# the same); raw cases give threshold, quality_num, quality_den to the C ABI and to fast_mirror.detect as they are.
# count: the mirror's keypoints, measured on the CPU (test_fast_param_cases.py asserts them).
Case = namedtuple("Case", "id image mc mq thr num den count what")

# the boundary ratio on 100x140 at threshold 25: smax = 88, 16 corners score exactly 46, and 88 * 46000 = 46 * 88000
BOUNDARY_SMAX, BOUNDARY_SCORE, BOUNDARY_NUM, BOUNDARY_DEN = 88, 46, 46000, 88000

CASES = (
    Case("q0", "100x140", 0.1, 0.0, None, None, None, 324, "q_num = 0: everything that survived suppression"),
    Case("q0-small", "70x131", 0.1, 0.0, None, None, None, 131, "q_num = 0, words and tiles not aligned"),
    Case("q0.5", "100x140", 0.1, 0.5, None, None, None, 102, "s >= smax / 2 with smax = 88: 44 is on the boundary"),
    Case("q1", "100x140", 0.1, 1.0, None, None, None, 1, "q_num = q_den: ties with the maximum only"),
    Case("thr0", "70x131", 0.0, 0.0, None, None, None, 229, "threshold 0, q_num 0: the densest bitmap"),
    Case("thr0-large", "100x140", 0.0, 0.0, None, None, None, 538, "threshold 0, q_num 0"),
    Case("thr255", "70x131", None, None, 255, 0, 1, 0, "s <= 255 always: empty"),
    Case("thr255-bw", "bw", None, None, 255, 0, 1, 0, "corners of score 255 sit exactly on s <= thr: empty"),
    Case("boundary", "100x140", None, None, 25, BOUNDARY_NUM, BOUNDARY_DEN, 93, "smax * num / den = 46 exactly: the rows at 46 stay"),
    Case("boundary+1", "100x140", None, None, 25, BOUNDARY_NUM + 1, BOUNDARY_DEN, 77, "one more in the numerator: the rows at 46 go"),
    Case("den-max-one", "bw", None, None, 51, DEN_MAX, DEN_MAX, 63, "num = den = 2^24 at s = smax = 255: 255 * 2^24 on both sides"),
    Case("den-max-half", "100x140", None, None, 25, DEN_MAX // 2, DEN_MAX, 102, "num = den / 2 at den = 2^24"),
    Case("den-max-half-bw", "bw", None, None, 51, DEN_MAX // 2, DEN_MAX, 63, "num = den / 2 at den = 2^24, scores of 255"),
    Case("score255", "bw", 0.2, 0.1, None, None, None, 63, "every corner scores 255, the top of the uint8 plane"),
)
BY_ID = {c.id: c for c in CASES}
EMPTY = ("thr255", "thr255-bw")
QUALITY_ONE = "q1"   # exempt from FLOOR: it keeps the rows at the maximum, at least one

# aps_fast_extract refuses these (threshold, quality_num, quality_den) with APS_E_ARG
REFUSED = ((-1, 1, 10), (256, 1, 10), (51, 0, 0), (51, 1, DEN_MAX + 1), (51, 11, 10))


def is_raw(case):
    return case.mc is None


def integers(case):
    """(threshold, quality_num, quality_den) of a case: its own, or what the wrapper makes of MinContrast / MinQuality."""
    if is_raw(case):
        return case.thr, case.num, case.den
    return (int(math.floor(case.mc * 255)),) + fmir.quality_rational(case.mq)


def as_input(case):
    return {"detector": "FAST", "MinContrast": case.mc, "MinQuality": case.mq}


@functools.lru_cache(maxsize=None)
def image(name):
    img = np.ascontiguousarray(IMAGES[name]())
    img.setflags(write=False)
    return img


def extract_integers(img, tb, thr, num, den):
    """fast_mirror.extract with the gate's integers handed to fast_mirror.detect as they are."""
    gray = fmir.gray_plane(img)
    ys, xs, sc = fmir.detect(gray, thr, num, den, tb.margin)
    n = len(ys)
    if n == 0:
        return np.zeros((0, 64), np.uint8), np.zeros((0, 2), np.float64), np.zeros((0, 4), np.float32)
    I = fmir.integral(gray)
    bins = fmir.orientation(I, ys, xs, tb)
    aux = np.zeros((n, 4), np.float32)
    aux[:, 0], aux[:, 1] = sc, bins
    return fmir.describe(I, ys, xs, bins, tb), np.stack([xs + 1, ys + 1], 1).astype(np.float64), aux


@functools.lru_cache(maxsize=None)
def mirror(case_id):
    """The mirror's (desc, loc, aux) of a case, computed once, shared by the tests, read-only: fast_mirror.extract for a
    wrapper case, extract_integers for a raw one."""
    case = BY_ID[case_id]
    if is_raw(case):
        out = extract_integers(image(case.image), fc.tables(), case.thr, case.num, case.den)
    else:
        out = fmir.extract(image(case.image), fc.tables(), MinContrast=case.mc, MinQuality=case.mq)
    for a in out:
        a.setflags(write=False)
    return out
