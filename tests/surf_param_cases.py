"""The SURF parameter matrix of test_surf_params_gpu.py (helper, not a test): the parameter sets, the arm of
aps_surf_extract each one is there for, and the mirror's keypoint count on the CPU.

What the rest of the suite runs is one set, aps_surf_params(thr, 8, 4, 0, 0) with thr 1000 or 50.  The arms that set never
enters (csrc/surf.hip):
  plan loop            `o <= params->n_octaves` decides only when NumOctaves is below what the image admits (oct1, oct2)
  surf_detect_kernel   `m = 1 .. nlv - 2`: one interior plane at NumScaleLevels 3, six at 8 (all of R[kMaxLev]); the bitmap
                       then holds nlv - 2 planes per octave and surf_emit_kernel decodes m = 1 + row / gh across them
  surf_keypoint_kernel `upright` skips the orientation block and two of its barriers (C ABI only: the wrapper sends 0)
  `v > thr`            at MetricThreshold 0 (the densest bitmap) and above every response (a plan, an all-zero bitmap)
test_surf_param_cases.py holds every case to the arm it is named for and to its count."""
import functools
from collections import namedtuple

import numpy as np

import surf_cases as sc
import surf_mirror as sm

IMAGES = {
    "pairA": lambda: sc.pair()[0],                           # 240 x 320: four octaves at four levels
    "97x131": lambda: sc.band_limited(2, 97, 131, 2.5),      # odd sizes, two octaves at four levels
    "coarse": lambda: sc.band_limited(7, 400, 520, 10.0),    # large blobs: keypoints up to the fifth octave
}
DEFAULT = dict(thr=1000.0, n_octaves=8, n_levels=4, upright=False)

# octaves: the length of the plan.  count: the mirror's keypoints (None: recorded by test_surf_param_cases.py, not fixed here).
# claim: how the case leaves the default arm - "octaves" (NumOctaves ends the plan loop, not the image), "planes" (nlv - 2
# interior planes, every one of them with a keypoint), "upright", "thr" (the threshold decides: keypoints at or below the
# default 1000, or none at all).
Case = namedtuple("Case", "id image thr n_octaves n_levels upright octaves count claims")

CASES = (
    Case("oct1", "pairA", 1000.0, 1, 4, False, 1, 479, ("octaves",)),
    Case("oct2", "pairA", 1000.0, 2, 4, False, 2, 575, ("octaves",)),
    Case("lev3", "pairA", 1000.0, 8, 3, False, 4, 460, ("planes",)),
    Case("lev3-small", "97x131", 1000.0, 8, 3, False, 3, 51, ("planes",)),
    Case("lev5", "pairA", 1000.0, 8, 5, False, 3, 640, ("planes",)),
    Case("lev6", "pairA", 1000.0, 8, 6, False, 3, 672, ("planes",)),
    Case("lev8", "pairA", 1000.0, 8, 8, False, 3, 697, ("planes",)),
    Case("lev8-small", "97x131", 1000.0, 8, 8, False, 1, 65, ("planes",)),   # one octave fits: 99 > 97
    Case("upright", "pairA", 1000.0, 8, 4, True, 4, 584, ("upright",)),
    Case("upright-small", "97x131", 1000.0, 8, 4, True, 2, 64, ("upright",)),
    Case("thr0", "pairA", 0.0, 8, 4, False, 4, 753, ("thr",)),
    Case("thr0-small", "97x131", 0.0, 8, 4, False, 2, 74, ("thr",)),
    Case("thr-huge", "pairA", 1e9, 8, 4, False, 4, 0, ("thr",)),
    Case("widest", "pairA", 0.0, 12, 8, False, 3, 1017, ("planes", "thr")),
    Case("coarse", "coarse", 10.0, 8, 4, False, 5, 252, ("thr",)),
    Case("coarse-lev6", "coarse", 10.0, 8, 6, False, 4, None, ("planes", "thr")),
)
BY_ID = {c.id: c for c in CASES}

DEFAULT_COUNTS = {"pairA": 584, "97x131": 64}   # the mirror at DEFAULT
COARSE_BINS = (24, 48, 96, 192, 384)            # filter side = scale * 9 / 1.2, binned at the octaves' doubling
COARSE_SPREAD = (20, 126, 92, 13, 1)
COARSE_LEV6_FLOOR = 50
EMPTY = ("thr-huge",)

# the ABI edges run on this image at DEFAULT
EDGE_IMAGE = "97x131"


def needs_raw_abi(case):
    """featureMatching.surf_extract forwards MetricThreshold, NumOctaves and NumScaleLevels; upright only the C ABI takes."""
    return bool(case.upright)


def as_input(case):
    return {"detector": "SURF", "MetricThreshold": case.thr, "NumOctaves": case.n_octaves, "NumScaleLevels": case.n_levels}


def filter_side(aux):
    """The interpolated filter side of each keypoint from aux's scale column (scale = 1.2 side / 9)."""
    return aux[:, 0].astype(np.float64) * 9.0 / 1.2


@functools.lru_cache(maxsize=None)
def image(name):
    img = np.ascontiguousarray(IMAGES[name]())
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def mirror(name, thr=1000.0, n_octaves=8, n_levels=4, upright=False):
    """surf_mirror.extract of image(name): (desc, loc, aux), computed once, shared by the tests, read-only."""
    out = sm.extract(image(name), MetricThreshold=thr, NumOctaves=n_octaves, NumScaleLevels=n_levels, upright=upright)
    for a in out:
        a.setflags(write=False)
    return out


def mirror_of(case):
    return mirror(case.image, case.thr, case.n_octaves, case.n_levels, case.upright)


@functools.lru_cache(maxsize=None)
def keypoints(name, thr=1000.0, n_octaves=8, n_levels=4):
    """surf_mirror.detect's (octave, level) per keypoint, in the order of mirror()'s rows."""
    k = sm.detect(sm.integral(sm.gray_plane(image(name))), thr, n_octaves, n_levels)
    o, m = k["o"].copy(), k["m"].copy()
    o.setflags(write=False)
    m.setflags(write=False)
    return o, m


def plan_of(case):
    h, w = image(case.image).shape[:2]
    return sm.plan(h, w, case.n_octaves, case.n_levels)
