"""Images, cases and shared reference results of the SIFT / SURF strongest-N tests (helper, not a test).  The unselected
references are oracle.sift and tests/surf_mirror.py, computed once per case and shared read-only; strongest_mirror.pick cuts them.
test_strongest_cases.py holds every figure quoted here, device-free."""
import functools

import numpy as np

import sift_param_cases as spc
import strongest_mirror as stm
import surf_mirror

SIFT_DEFAULT = (1.6, 4, 0.00133, 6.0)

# name: (image kind of sift_param_cases.oracle_sift or "twin", h, w, parameter set, oracle rows, second-orientation rows, [N])
SIFT_CASES = {
    "120x160": ("rgb", 120, 160, SIFT_DEFAULT, 419, 71, (1, 3, 13, 100, 418, 419, 420, 5000)),   # 1, 3, 13: inside a keypoint's tie
    "97x131": ("rgb", 97, 131, SIFT_DEFAULT, 281, 47, (4, 7, 8, 100)),                         # 4, 7, 8: inside a keypoint's tie
    "gray": ("gray", 120, 160, spc.params(spc.BY_ID[spc.GRAY_CASE]), spc.GRAY_COUNT, 50, (50,)),
    "37x37": ("rgb", 37, 37, spc.params(spc.BY_ID[spc.SMALL_CASE]), spc.SMALL_SHAPES[(37, 37)], 1, (3,)),
    "twin": ("twin", 128, 256, SIFT_DEFAULT, 138, 18, None),   # N: the first cuts inside a tie of two keypoints (twin_cuts)
}
SIFT_TIE_CUTS = {"120x160": (1, 3, 13), "97x131": (4, 7, 8)}   # the Ns that fall inside the tie of one keypoint's orientations
TWIN_DISTINCT = 60   # distinct responses among the twin image's 138 oracle rows

# name: (case of test_surf_gpu.CASES or "twin", MetricThreshold, mirror rows, [N])
SURF_CASES = {
    "97x131": ("97x131", 1000.0, 64, (1, 10, 63, 64, 65)),
    "pairA": ("pairA", 1000.0, 584, (200,)),
    "131x97x3": ("131x97x3", 1000.0, 50, (20,)),
    "600x800": ("600x800", 50.0, 5519, (1000,)),    # thousands of rows: several blocks of the sort and of the scans
    "twin": ("twin", 200.0, 24, (1, 3, 9)),          # 12 tied pairs: every odd cut falls inside a tie of two keypoints
}


@functools.lru_cache(maxsize=None)
def twin_image():
    """128 x 256 gray at level 110 with one 40 x 40 patch of smoothed noise, faded to the background over its 8-pixel rim, at
    columns 44 and 172: a period of 128 pixels, which every octave of SIFT and every sampling step of SURF divides, so the two
    copies give the same keypoints with the same response bits."""
    from scipy.ndimage import gaussian_filter

    p = gaussian_filter(np.random.default_rng(5).standard_normal((40, 40)), 1.5)
    p = p / np.abs(p).max()
    r = np.minimum(np.arange(40), 39 - np.arange(40)).astype(np.float64)
    f = np.clip((r + 0.5) / 8, 0, 1)
    img = np.full((128, 256), 110.0)
    for c in (44, 172):
        img[44:84, c:c + 40] += 100.0 * p * (f[:, None] * f[None, :])
    img = np.clip(np.round(img), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


def sift_input(name, N=None):
    sigma, nl, contrast, edge = SIFT_CASES[name][3]
    inp = {"detector": "SIFT", "Sigma": sigma, "NumLayersInOctave": nl, "ContrastThreshold": contrast, "EdgeThreshold": edge}
    return inp if N is None else {**inp, "NumStrongest": N}


def sift_image(name):
    kind, h, w = SIFT_CASES[name][:3]
    return twin_image() if kind == "twin" else {"rgb": spc.image, "gray": spc.gray_image}[kind](h, w)


@functools.lru_cache(maxsize=None)
def _twin_oracle():
    import oracle

    out = oracle.sift(twin_image(), *SIFT_DEFAULT)
    for a in out:
        a.setflags(write=False)
    return out


def sift_reference(name):
    """oracle.sift of the case, unselected: (desc, loc, aux), read-only, shared with test_sift_params_gpu.py's cache."""
    kind, h, w, prm = SIFT_CASES[name][:4]
    return _twin_oracle() if kind == "twin" else spc.oracle_sift(kind, h, w, prm)


def sift_Ns(name):
    Ns = SIFT_CASES[name][6]
    if Ns is None:   # the twin image: cuts taken from the oracle
        d, loc, aux = sift_reference(name)
        Ns = tuple(stm.tie_cuts(aux, loc, cross=True)[:4])
    return Ns


def surf_input(name, N=None):
    inp = {"detector": "SURF", "MetricThreshold": SURF_CASES[name][1]}
    return inp if N is None else {**inp, "NumStrongest": N}


@functools.lru_cache(maxsize=None)
def _twin_surf():
    out = surf_mirror.extract(twin_image(), MetricThreshold=SURF_CASES["twin"][1])
    for a in out:
        a.setflags(write=False)
    return out


def surf_reference(name):
    """(image, (desc, loc, aux)) of the SURF mirror, unselected, read-only; test_surf_gpu.mirror's cache is shared."""
    case, thr = SURF_CASES[name][:2]
    if case == "twin":
        return twin_image(), _twin_surf()
    from test_surf_gpu import mirror

    img, mthr, md, mloc, maux = mirror(case)
    assert mthr == thr
    return img, (md, mloc, maux)
