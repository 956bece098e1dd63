"""NumPy restatement of DESIGN.md "KAZE selection and Upright" -- test infrastructure, not a test.

Written from the contract, from the pieces it names: the candidates are kaze_mirror's keypoints in canonical order
(``scale_space`` / ``detect``), their strength is the metric, strongest-N is ``strongest_mirror.keep``, uniform-N is
``uniform_mirror.cell`` of the detection pixel on the H x W image and ``uniform_mirror.keep`` with one group, and the kept
candidates are described by ``kaze_mirror.orientation`` / ``descriptor`` -- with Upright by ``descriptor`` at (c, s) = (1, 0) and
an angle of +0.0.  ``stages`` holds what every combination of the four keys shares, so a test computes it once per image.
"""
import numpy as np

import kaze_mirror as km
import strongest_mirror as sm
import uniform_mirror as um

f32 = np.float32


def stages(img, Threshold=0.0001, NumOctaves=3, NumScaleLevels=4):
    """(shape, LX, LY, keypoints of kaze_mirror.detect, (c, sn, angle_deg) of every keypoint), or None for an image below level 1's
    margin."""
    img = np.asarray(img)
    lv = km.levels(NumOctaves, NumScaleLevels)
    if min(img.shape[:2]) < 2 * lv["margin"][1] + 1:
        return None
    lv, LX, LY, RR = km.scale_space(img, NumOctaves, NumScaleLevels)
    k = km.detect(lv, RR, Threshold)
    if k["px"].size:
        ori = km.orientation(LX, LY, k["m"], k["px"], k["py"], k["scale"])
    else:
        ori = (np.zeros(0, f32),) * 3
    return img.shape[:2], LX, LY, k, ori


def keep(st, NumStrongest=None, NumUniform=None, UniformGrid=um.DEFAULT_GRID):
    """Ascending indices of the candidates the keys keep."""
    if NumStrongest is not None and NumUniform is not None:
        raise ValueError("NumUniform and NumStrongest exclude each other")
    (H, W), _, _, k, _ = st
    n = k["px"].size
    for N in (NumStrongest, NumUniform):
        if N is not None and N < 1:
            raise ValueError("N must be at least 1")
    if n == 0 or (NumStrongest is None and NumUniform is None):
        return np.arange(n)
    if NumStrongest is not None:
        return sm.keep(k["metric"], NumStrongest)
    rows, cols = UniformGrid
    assert 1 <= rows <= 32 and 1 <= cols <= 32
    return um.keep(k["metric"], um.cell(k["i"], k["j"], H, W, UniformGrid), [min(NumUniform, n)], rows * cols)


def cells(st, UniformGrid=um.DEFAULT_GRID):
    """The cell of every candidate's detection pixel."""
    (H, W), _, _, k, _ = st
    return um.cell(k["i"], k["j"], H, W, UniformGrid)


def describe(st, at, Upright=False):
    """(desc, loc, aux) of the candidates `at` (ascending indices)."""
    _, LX, LY, k, (c, sn, ang) = st
    at = np.asarray(at, np.int64)
    if at.size == 0:
        return np.zeros((0, 64), f32), np.zeros((0, 2), np.float64), np.zeros((0, 4), f32)
    m, px, py, s = k["m"][at], k["px"][at], k["py"][at], k["scale"][at]
    if Upright:
        c, sn, ang = np.ones(at.size, f32), np.zeros(at.size, f32), np.zeros(at.size, f32)
    else:
        c, sn, ang = c[at], sn[at], ang[at]
    desc = km.descriptor(LX, LY, m, px, py, s, c, sn)
    loc = np.stack([px.astype(np.float64) + 1.0, py.astype(np.float64) + 1.0], 1)
    aux = np.stack([s, ang, k["metric"][at], m.astype(f32)], 1).astype(f32)
    return desc, loc, aux


def extract(img, NumStrongest=None, NumUniform=None, UniformGrid=um.DEFAULT_GRID, Upright=False, st=None, **kw):
    """What kaze_extract returns with want_aux for any combination of the four keys; kw: kaze_mirror.extract's.  st: stages(img,
    **kw) when the caller has them."""
    st = stages(img, **kw) if st is None else st
    if st is None:
        return np.zeros((0, 64), f32), np.zeros((0, 2), np.float64), np.zeros((0, 4), f32)
    return describe(st, keep(st, NumStrongest, NumUniform, UniformGrid), Upright)
