"""Images and shared mirror results of the KAZE selection / Upright tests (helper, not a test).  The images are kaze_cases' (the
counts below were computed with tests/kaze_mirror.py) plus a mirror-symmetric one whose metrics tie in pairs; the stages of an
image (kaze_select_mirror.stages) and every selected result are computed once and shared read-only."""
import numpy as np

import kaze_cases as kc
import kaze_select_mirror as ksm
from kaze_cases import PAIR_H, band_limited, pair, ratio_matches, transfer_error  # noqa: F401  (the tests take them from here)

# name: rows of the unselected call at the defaults
COUNTS = {"97x131": 99, "64x64": 17, "131x97x3": 91, "pairA": 1090, "48x2100": 429, "tie": 176}
LEVELS_97x131 = [0, 5, 60, 0, 27, 2, 0, 5]   # rows per level 0..7 of "97x131" (none above); all its metrics are distinct


def tie_image():
    """120 x 160: X beside its mirror image.  The contract's arithmetic is mirror-symmetric, so the 176 rows are 88 pairs of
    bit-equal metrics: every odd N in 1..175 cuts a pair, every even N cuts none."""
    X = band_limited(9, 120, 80, 2.5)
    return np.hstack([X, X[:, ::-1]])


_IMAGES = {"tie": tie_image, "pairB": lambda: pair()[1]}
_STAGES, _RESULTS = {}, {}


def image(name):
    return _IMAGES[name]() if name in _IMAGES else kc.CASES[name][0]()


def stages(name):
    """(image, kaze_select_mirror.stages of it) of a case at the defaults."""
    if name not in _STAGES:
        img = image(name)
        assert name in _IMAGES or not kc.CASES[name][1], "the selection cases run at the default parameters"
        _STAGES[name] = (img, ksm.stages(img))
    return _STAGES[name]


def mirror(name, **keys):
    """(image, desc, loc, aux) of a case under the keys NumStrongest / NumUniform / UniformGrid / Upright."""
    at = (name, tuple(sorted(keys.items())))
    if at not in _RESULTS:
        img, st = stages(name)
        out = ksm.extract(img, st=st, **keys)
        for a in out:
            a.setflags(write=False)
        _RESULTS[at] = (img,) + out
    return _RESULTS[at]


def correct_matches(dA, locA, dB, locB, ratio=0.6, within=2.0):
    """(ratio-test matches, those within `within` px of PAIR_H) between the rows of the pair's two views."""
    m = ratio_matches(dA, dB, ratio)
    err = transfer_error(locA[m[:, 0]], locB[m[:, 1]])
    return len(m), int((err <= within).sum())
