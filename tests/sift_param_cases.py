"""The SIFT parameter matrix of test_sift_params_gpu.py (helper, not a test): the parameter sets, the arm of
aps_sift_extract's dispatch each one is there for, and the radius rule that decides which arm a set takes.

The rule is restated here from make_gauss / aps_sift_extract in csrc/sift.hip (gauss_kernel / orc_sift in
oracle/sift_oracle.c say the same): a Gaussian of sigma s has n = min(lrint(8 s + 1) | 1, 63) taps, radius n // 2; the base
blur is sqrt(max(Sigma^2 - 1, 0.01)); plane i of an octave (1 <= i <= nl + 2) is plane i - 1 blurred by
Sigma 2^((i-1)/nl) sqrt(2^(2/nl) - 1).

Dispatch on those radii (sift.hip):
  base blur    radius 3..8: the fused blur_base_kernel<R>; otherwise gray_up_kernel + launch_blur
  launch_blur  radius 1..12: blur_kernel<R>; above: blur_row_generic + blur_col_generic, which does not write the next octave's
               base, so plane nl at a radius above 12 sends every later octave through decimate_kernel
  extrema      extrema_wave_kernel<nl>, nl = 1..5
  descriptor   a square of radius rint(3 scl sqrt(2) 2.5), clamped to the octave's diagonal; above 63 the plain sweep
test_sift_param_cases.py holds every case to the arm it is named for."""
import functools
import math
from collections import namedtuple

import numpy as np

MAX_TAPS = 63        # make_gauss: n > 63 -> 63
TILE_MAX = 12        # launch_blur: blur_kernel<1..12>
BASE_FUSED = (3, 8)  # launch_base_blur: blur_base_kernel<3..8>
DESCR_QUEUED_MAX = 63  # descr_kernel: radius > 63 takes the plain sweep

SHAPES = ((120, 160), (97, 131))


def gauss_taps(sigma):
    """Tap count before the clamp (Python's round is lrint's round-half-even)."""
    return int(round(sigma * 8.0 + 1.0)) | 1


def gauss_radius(sigma):
    return min(gauss_taps(sigma), MAX_TAPS) // 2


def base_sigma(sigma):
    return math.sqrt(max(sigma * sigma - 4.0 * 0.5 * 0.5, 0.01))


def plane_sigmas(sigma, nl):
    """The incremental sigmas of planes 1 .. nl + 2."""
    kf = 2.0 ** (1.0 / nl)
    out = []
    for i in range(1, nl + 3):
        sp = kf ** (i - 1) * sigma
        st = sp * kf
        out.append(math.sqrt(st * st - sp * sp))
    return out


def radii(sigma, nl):
    """(base radius, [radius of plane 1, ..., plane nl + 2])."""
    return gauss_radius(base_sigma(sigma)), [gauss_radius(s) for s in plane_sigmas(sigma, nl)]


def descr_radius(aux):
    """Per keypoint: the descriptor's sampling radius before the diagonal clamp, from aux = [size, angle, response,
    octave + 256 layer] (size = 2 scl 2^octave / 2)."""
    octave = aux[:, 3].astype(int) % 256
    scl = aux[:, 0] / 2.0 ** octave
    return np.rint(3.0 * scl * math.sqrt(2.0) * 2.5), octave


def octave_diag(h, w, octave):
    """floor of the diagonal of octave `octave` of an h x w image (octave 0 is the 2x base)."""
    ow, oh = np.maximum(1, (2 * w) >> octave), np.maximum(1, (2 * h) >> octave)
    return np.floor(np.sqrt((ow * ow + oh * oh).astype(np.float64)))


# arms: names checked by test_sift_param_cases.arm_reached.  counts: oracle keypoints at 120 x 160 and 97 x 131 (RGB), from
# a CPU run of oracle.sift; every test asserts at least half of them, so that no case passes on a handful of keypoints.
Case = namedtuple("Case", "id sigma nl contrast edge counts arms")

CASES = (
    Case("nl1", 1.6, 1, 0.00133, 6.0, (279, 171), ("nl=1", "blur=11", "generic_after_nl", "clamp")),       # 5; 11 22 31
    Case("nl5", 1.6, 5, 0.00133, 6.0, (430, 277), ("nl=5",)),                                               # 5; 4 4 5 6 7 7 9
    Case("sigma3.2", 3.2, 3, 0.00133, 6.0, (233, 151), ("base>8", "generic_at_nl", "descr>63")),           # 12; 10 13 16 20 25
    Case("base8", 2.2, 2, 0.00133, 6.0, (258, 170), ("base=8", "nl=2", "generic_at_nl")),                   # 8; 9 13 18 25
    Case("blur1", 0.9, 4, 0.00133, 6.0, (548, 336), ("blur=1", "base<3")),                                  # 1; 3 3 4 4 5 6
    Case("base10", 2.7, 4, 0.00133, 6.0, (295, 184), ("blur=10", "base>8", "tile_at_nl", "generic_after_nl")),  # 10; 7 9 10 12 14 17
    Case("nl5_fallback", 1.05, 5, 0.00133, 6.0, (575, 379), ("nl=5", "base<3")),                           # 2; 3 3 3 4 4 5 6
    Case("thr0_edge50", 1.6, 4, 0.0, 50.0, (430, 301), ()),
    Case("thr0_edge1", 1.6, 4, 0.0, 1.0, (0, 0), ()),
    Case("edge1e6", 1.6, 4, 0.00133, 1e6, (431, 301), ()),
    Case("base3", 1.2, 4, 0.00133, 6.0, (486, 313), ("base=3",)),                                           # 3; 3 4 5 5 6 8
    Case("base6", 1.85, 3, 0.00133, 6.0, (377, 243), ("base=6",)),                                          # 6; 6 7 9 12 15
    Case("clamp", 4.0, 2, 0.00133, 6.0, (60, 21), ("clamp", "base>8", "nl=2", "generic_at_nl", "descr>63")),  # 16; 16 23 31 31
)
BY_ID = {c.id: c for c in CASES}

# the one gray case, its oracle count at 120 x 160 (channel 1 of the RGB image)
GRAY_CASE, GRAY_COUNT = "sigma3.2", 233

# section 4: large scales on images whose octaves shrink below 2 kBorder and whose diagonals fall below the descriptor radius
SMALL_CASE = "sigma3.2"
SMALL_SHAPES = {(35, 47): 12, (18, 515): 48, (37, 37): 8}  # shape -> oracle keypoints


def params(case):
    return case.sigma, case.nl, case.contrast, case.edge


def as_input(case, **more):
    return dict({"detector": "SIFT", "Sigma": case.sigma, "NumLayersInOctave": case.nl, "ContrastThreshold": case.contrast,
                 "EdgeThreshold": case.edge}, **more)


@functools.lru_cache(maxsize=None)
def image(h, w):
    """test_sift_gpu's textured image of that shape, read-only."""
    from test_sift_gpu import textured

    img = textured(np.random.default_rng(h * 7 + w), h, w)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def gray_image(h, w):
    g = np.ascontiguousarray(image(h, w)[..., 1])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def dense_image():
    """300 x 400 gray, smoothed noise stretched to 0..255: 6367 oracle features with the default parameters, more than the
    wrapper's first capacity of 4096."""
    from scipy.ndimage import gaussian_filter

    g = gaussian_filter(np.random.default_rng(11).random((300, 400)), 1.2)
    g = ((g - g.min()) / (g.max() - g.min()) * 255).astype(np.uint8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def oracle_sift(kind, h, w, prm):
    """oracle.sift of image(h, w) / gray_image(h, w) / dense_image() at prm = (sigma, nl, contrast, edge): computed once,
    shared by the tests, read-only."""
    import oracle

    img = {"rgb": image, "gray": gray_image}[kind](h, w) if kind != "dense" else dense_image()
    out = oracle.sift(img, *prm)
    for a in out:
        a.setflags(write=False)
    return out
