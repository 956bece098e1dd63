"""Images, expected plans and shared mirror results of the FAST/FREAK pyramid tests (helper, not a test)."""
import functools

import numpy as np

import fast_cases as fc
import fast_mirror as fmir
import fast_pyramid_mirror as pmir

# name: (image builder, NumLevels, ScaleFactor, MinContrast, mirror keypoints per level of the plan) - what it catches
CASES = {
    "120x160": (lambda: fc.noise_rects(21, 120, 160), 4, 1.2, 0.05, [825, 420, 208, 63]),           # four levels, none a multiple of a tile
    "64x64": (lambda: fc.noise_lattice(12, 64, 64), 3, 1.2, 0.05, [81, 8]),                         # the plan drops the third level (44 < 47)
    "129x1230": (lambda: fc.noise_rects(23, 129, 1230), 3, 1.2, 0.1, [6823, 3324, 1260]),           # level 1 is 108 x 1025: crosses the 1024-px row-scan chunk
    "200x300x3": (lambda: fc.noise_rects(24, 200, 300, 3), 8, 1.2, 0.1, [1963, 634, 174, 53, 24, 10, 1, 0]),  # RGB; an empty last level inside the plan
    "150x200": (lambda: fc.noise_rects(25, 150, 200), 2, 2.0, 0.05, [1548, 143]),                   # the largest factor
    "96x131": (lambda: fc.noise_rects(26, 96, 131), 3, 1.5, 0.05, [407, 78]),                       # third level dropped at 1.5
    "planted": (lambda: fc.planted()[0], 3, 1.2, 0.2, [22, 6, 2]),
    "flat": (lambda: np.full((90, 100), 77, np.uint8), 3, 1.2, 0.2, [0, 0, 0]),
}
PLANS = {   # (h, w) per level, by hand from the contract
    "120x160": [(120, 160), (100, 133), (83, 111), (69, 93)],
    "64x64": [(64, 64), (53, 53)],
}


@functools.lru_cache(maxsize=None)
def image(name):
    img = CASES[name][0]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def mirror(name, library_tables=False):
    """(desc, loc, aux) of the mirror for a case, computed once and shared (read-only).  The tables are the contract's own
    (device-free) or, for the device comparisons, what aps_freak_pattern reports."""
    _, nl, sf, mc, _ = CASES[name]
    out = pmir.extract(image(name), fc.tables() if library_tables else contract_tables(), NumLevels=nl, ScaleFactor=sf, MinContrast=mc)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def contract_tables():
    return fmir.contract_tables()


def per_level(aux, n_levels):
    return np.bincount(aux[:, 2].astype(np.int64), minlength=n_levels).tolist()


# ---- the twin pair: B is level 2 of A, so A's level-2 keypoints are B's keypoints ------------------------------------------
TWIN_LEVELS, TWIN_SCALE, TWIN_MC = 3, 1.2, 0.05


@functools.lru_cache(maxsize=None)
def twin_images():
    A = fc.noise_rects(31, 180, 240)
    B = pmir.planes(A, TWIN_LEVELS, TWIN_SCALE, 23)[2].astype(np.uint8)
    for a in (A, B):
        a.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def twin_mirror(library_tables=False):
    """(A at three levels, A at one level, B at one level), each (desc, loc, aux) of the mirror."""
    A, B = twin_images()
    tb = fc.tables() if library_tables else contract_tables()
    out = (pmir.extract(A, tb, TWIN_LEVELS, TWIN_SCALE, TWIN_MC), pmir.extract(A, tb, 1, TWIN_SCALE, TWIN_MC),
           pmir.extract(B, tb, 1, TWIN_SCALE, TWIN_MC))
    for t in out:
        for a in t:
            a.setflags(write=False)
    return out
