"""The FAST/FREAK scale pyramid on its NumPy restatement alone (tests/fast_pyramid_mirror.py): hand cases for the plan and the
resampling, the keypoints every test image carries per level, and the twin pair that shows what the pyramid is for.  No
library, no device: the tables are fast_mirror.contract_tables()."""
import numpy as np
import pytest

import fast_cases as fc
import fast_pyramid_cases as pc
import fast_pyramid_mirror as pmir

MARGIN = 23
S12 = pmir.scale_rational(1.2)


def test_plan_hand_cases():
    assert S12 == (1200000, 1000000)
    assert pmir.plan(120, 160, 4, *S12, MARGIN) == [(120, 160), (100, 133), (83, 111), (69, 93)]
    assert pmir.plan(64, 64, 3, *S12, MARGIN) == [(64, 64), (53, 53)]          # the third level would be 44 < 47
    assert pmir.plan(64, 64, 16, *S12, MARGIN) == [(64, 64), (53, 53)]
    assert pmir.plan(47, 49, 8, *S12, MARGIN) == [(47, 49)]                    # level 0 always exists
    assert pmir.plan(30, 30, 8, *S12, MARGIN) == [(30, 30)]
    assert pmir.plan(150, 200, 2, 2, 1, MARGIN) == [(150, 200), (75, 100)]
    assert pmir.plan(95, 95, 2, 2, 1, MARGIN) == [(95, 95), (48, 48)]          # 47.5 rounds half up
    assert pmir.plan(120, 160, 1, *S12, MARGIN) == [(120, 160)]
    for bad in ((0, *S12), (17, *S12), (2, 1000000, 1000000), (2, 2000001, 1000000), (2, 3, 0), (2, -3, -2)):
        with pytest.raises(ValueError):
            pmir.plan(120, 160, *bad, MARGIN)


def test_axis_hand_case():
    """4 -> 3: centres at 2/3, 2, 10/3 source pixels, minus the half pixel: 1/6, 3/2, 17/6."""
    x0, x1, wx = pmir.axis(4, 3)
    assert x0.tolist() == [0, 1, 2] and x1.tolist() == [1, 2, 3] and wx.tolist() == [256 // 6, 128, 256 * 5 // 6]
    x0, x1, wx = pmir.axis(5, 5)
    assert x0.tolist() == list(range(5)) and not wx.any()


def test_factor_two_is_the_rounded_mean_of_2x2():
    g = fc.noise_rects(3, 50, 62).astype(np.int64)
    want = (g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2] + 2) >> 2
    assert np.array_equal(pmir.resample(g, 25, 31), want)


def test_constant_plane_stays_constant():
    for v in (0, 77, 255):
        out = pmir.resample(np.full((61, 83), v, np.int64), 51, 69)
        assert out.shape == (51, 69) and (out == v).all()


def test_horizontal_ramp_stays_monotone():
    g = np.tile(np.arange(0, 250, 2, dtype=np.int64), (60, 1))   # 60 x 125, strictly rising along x
    out = pmir.resample(g, 50, 104)
    assert (np.diff(out, axis=1) >= 0).all() and (out == out[0]).all()
    assert out[0, 0] == 0 and out[0, -1] == 248 and out.min() >= 0 and out.max() <= 255


@pytest.mark.parametrize("name", list(pc.CASES))
def test_cases_have_keypoints_at_every_level(name):
    """Device-free: the images carry what the comparisons need - the counts per level of the issue's table."""
    _, nl, sf, mc, want = pc.CASES[name]
    img = pc.image(name)
    shapes = pmir.plan(img.shape[0], img.shape[1], nl, *pmir.scale_rational(sf), MARGIN)
    if name in pc.PLANS:
        assert shapes == pc.PLANS[name]
    lv = pmir.planes(img, nl, sf, MARGIN)
    assert [p.shape for p in lv] == shapes and all(0 <= p.min() and p.max() <= 255 for p in lv)
    d, loc, aux = pc.mirror(name)
    counts = pc.per_level(aux, len(shapes))
    assert counts == want
    # (planted is exact by construction and small, 22 + 6 + 2 as counted above, as in test_fast_gpu; every noise image carries 50)
    if name not in ("flat", "planted"):
        assert len(d) >= 50
    assert all(c > 0 for c, w in zip(counts, want) if w > 0)
    assert np.array_equal(aux[:, 2], np.sort(aux[:, 2])) and not aux[:, 3].any()   # ascending level
    # within a level ascending (row, col); level 0's locations are the integers x + 1, y + 1
    h0, w0 = shapes[0]
    for l, (hl, wl) in enumerate(shapes):
        m = aux[:, 2] == l
        xl = ((loc[m, 0] - 0.5) * (2 * wl) / w0 - 1) / 2
        yl = ((loc[m, 1] - 0.5) * (2 * hl) / h0 - 1) / 2
        assert np.allclose(xl, np.round(xl), atol=1e-9) and np.allclose(yl, np.round(yl), atol=1e-9)
        key = np.round(yl) * wl + np.round(xl)
        assert (np.diff(key) > 0).all()
        assert xl.size == 0 or (xl.min() >= MARGIN - 1e-9 and xl.max() <= wl - 1 - MARGIN + 1e-9)
    m0 = aux[:, 2] == 0
    assert np.array_equal(loc[m0], np.round(loc[m0]))


def test_one_level_is_the_single_level_mirror():
    import fast_mirror as fmir

    img = pc.image("120x160")
    one = pmir.extract(img, pc.contract_tables(), NumLevels=1, MinContrast=0.05)
    ref = fmir.extract(img, pc.contract_tables(), MinContrast=0.05)
    assert all(np.array_equal(a, b) for a, b in zip(one, ref))


def test_twin_pair():
    """B is level 2 of A.  The rows of A's pyramid at level 2 are B's rows, byte for byte, at the locations the formula gives;
    matched with the reference's binary filter (MatchThreshold 10, MaxRatio 0.6) the pyramid finds every twin at distance 0,
    while single-level A shares next to nothing with B (0 rows kept)."""
    A, B = pc.twin_images()
    assert B.shape == (125, 167)
    (d3, l3, a3), (d1, l1, a1), (db, lb, ab) = pc.twin_mirror()
    at2 = np.flatnonzero(a3[:, 2] == 2)
    assert len(at2) == 728 == len(db)
    assert np.array_equal(d3[at2], db) and np.array_equal(a3[at2, :2], ab[:, :2])
    want_loc = pmir.loc_of(lb[:, 0].astype(np.int64) - 1, lb[:, 1].astype(np.int64) - 1, B.shape, A.shape)
    assert np.array_equal(l3[at2].view(np.uint64), want_loc.view(np.uint64))
    m, d = fc.match_binary(db, d3, 0.6, 10.0)
    got = dict(zip(m[:, 0].tolist(), zip(m[:, 1].tolist(), d.tolist())))
    assert all(got.get(i + 1) == (int(at2[i]) + 1, 0.0) for i in range(len(db)))   # every twin, at distance 0
    m1, _ = fc.match_binary(db, d1, 0.6, 10.0)
    assert len(m1) < 0.05 * len(db)
