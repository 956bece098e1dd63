"""Images and shared mirror results of the FAST/FREAK strongest-N tests (helper, not a test)."""
import functools

import numpy as np

import fast_cases as fc
import fast_pyramid_cases as pc
import fast_strongest_mirror as smir

# the tie cases: six copies of one 64 x 64 noise image, so the candidates away from the copies' seams come in classes of equal R
TIE_MC = 0.05
TIES = {"tiled1": (1, 100), "tiled2": (2, 202)}   # name: (NumLevels, N that cuts inside a class of level 0)


@functools.lru_cache(maxsize=None)
def tiled_image():
    img = np.ascontiguousarray(np.tile(fc.noise_rects(41, 64, 64), (2, 3)))
    img.setflags(write=False)
    return img


def spec(name):
    """(image, NumLevels, ScaleFactor, MinContrast) of a pyramid case, a tie case or a twin ("twinA", "twinB", "twinB1")."""
    if name in TIES:
        return tiled_image(), TIES[name][0], 1.2, TIE_MC
    if name in ("twinA", "twinB", "twinB1"):
        A, B = pc.twin_images()
        return (A if name == "twinA" else B), (1 if name == "twinB1" else pc.TWIN_LEVELS), pc.TWIN_SCALE, pc.TWIN_MC
    _, nl, sf, mc, _ = pc.CASES[name]
    return pc.image(name), nl, sf, mc


@functools.lru_cache(maxsize=None)
def candidates(name, library_tables=False):
    """fast_strongest_mirror.candidates of a case, computed once and shared (read-only)."""
    img, nl, sf, mc = spec(name)
    out = smir.candidates(img, fc.tables() if library_tables else pc.contract_tables(), nl, sf, mc)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def mirror(name, N, library_tables=False):
    return smir.pick(candidates(name, library_tables), N)


def per_level(aux, n_levels):
    return pc.per_level(aux, n_levels)
