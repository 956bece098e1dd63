"""Keeps the FAST/FREAK parameter matrix honest (CPU; the pattern tables come from the built library, no device): every case
of fast_param_cases.CASES carries the mirror's keypoints it was chosen for and sits on the edge of the gate or of the
threshold that its row names.

Mirror keypoints measured on the CPU: q0 324, q0-small 131, q0.5 102, q1 1, thr0 229, thr0-large 538, thr255 0, thr255-bw 0,
boundary 93, boundary+1 77 (the 16 rows of score 46 go), den-max-one 63, den-max-half 102, den-max-half-bw 63, score255 63.
Every non-empty case carries at least 50, except q1, which keeps the one row at the maximum (88)."""
import numpy as np
import pytest

import fast_cases as fc
import fast_mirror as fmir
import fast_param_cases as pc


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_mirror_counts_of_the_matrix(case):
    d, loc, aux = pc.mirror(case.id)
    n = len(d)
    assert n == case.count
    assert (n == 0) == (case.id in pc.EMPTY)
    if case.id == pc.QUALITY_ONE:
        assert n >= 1
    elif case.id not in pc.EMPTY:
        assert n >= pc.FLOOR
    thr, num, den = pc.integers(case)
    assert 0 <= thr <= 255 and 0 <= num <= den <= pc.DEN_MAX and den > 0, "a case the ABI would refuse"
    h, w = pc.image(case.image).shape[:2]
    assert h <= 400 and w <= 520


def test_wrapper_cases_are_what_their_integers_say():
    """fast_mirror.extract(MinContrast, MinQuality) and the same case through its integers: one result."""
    for case in pc.CASES:
        if not pc.is_raw(case):
            got = pc.extract_integers(pc.image(case.image), fc.tables(), *pc.integers(case))
            assert all(np.array_equal(a, b) for a, b in zip(got, pc.mirror(case.id))), case.id


def test_quality_one_keeps_exactly_the_rows_at_the_maximum():
    everything = pc.mirror("q0")[2][:, 0]
    kept = pc.mirror("q1")
    at_max = everything == everything.max()
    assert 1 <= at_max.sum() == len(kept[0]) < len(everything)
    assert (kept[2][:, 0] == everything.max()).all()
    assert np.array_equal(kept[1], pc.mirror("q0")[1][at_max]) and np.array_equal(kept[0], pc.mirror("q0")[0][at_max])
    assert pc.integers(pc.BY_ID["q1"])[1:] == (1000000, 1000000) and pc.integers(pc.BY_ID["q0"])[1] == 0


def test_quality_zero_keeps_everything_that_survived_suppression():
    for cid in ("q0", "q0-small", "thr0", "thr0-large"):
        case = pc.BY_ID[cid]
        thr = pc.integers(case)[0]
        kept = fmir.suppress(fmir.scores(fmir.gray_plane(pc.image(case.image)), thr, fc.tables().margin))
        assert (kept > 0).sum() == case.count
    # threshold 0 is denser than anything the default parameters reach
    assert pc.BY_ID["thr0"].count > pc.BY_ID["q0-small"].count and pc.integers(pc.BY_ID["thr0"])[0] == 0


def test_the_boundary_ratio_lands_on_a_score_of_the_image():
    scores = pc.mirror("q0")[2][:, 0].astype(np.int64)   # same image and threshold as the boundary cases
    assert pc.BY_ID["boundary"].image == pc.BY_ID["q0"].image and pc.BY_ID["boundary"].thr == pc.integers(pc.BY_ID["q0"])[0]
    assert scores.max() == pc.BOUNDARY_SMAX
    assert pc.BOUNDARY_SMAX * pc.BOUNDARY_NUM == pc.BOUNDARY_SCORE * pc.BOUNDARY_DEN   # smax * num / den is the integer 46
    on_it = int((scores == pc.BOUNDARY_SCORE).sum())
    assert on_it >= 5
    keep, drop = pc.mirror("boundary")[2][:, 0], pc.mirror("boundary+1")[2][:, 0]
    assert keep.min() == pc.BOUNDARY_SCORE and (keep == pc.BOUNDARY_SCORE).sum() == on_it   # >= keeps them
    assert drop.min() > pc.BOUNDARY_SCORE and len(keep) - len(drop) == on_it                # one more in the numerator drops them
    # half the maximum is a boundary too: 44 is a score of the image
    assert (pc.mirror("q0.5")[2][:, 0] == pc.BOUNDARY_SMAX // 2).sum() >= 1 and pc.BOUNDARY_SMAX % 2 == 0


def test_the_denominator_bound():
    one, half, half_bw = pc.BY_ID["den-max-one"], pc.BY_ID["den-max-half"], pc.BY_ID["den-max-half-bw"]
    assert one.den == half.den == half_bw.den == pc.DEN_MAX == 1 << 24 and one.num == one.den and 2 * half.num == half.den
    assert (pc.mirror("den-max-one")[2][:, 0] == 255).all()   # s * den = smax * num = 255 * 2^24
    assert 255 * pc.DEN_MAX > 2 ** 31
    assert all(np.array_equal(a, b) for a, b in zip(pc.mirror("den-max-half"), pc.mirror("q0.5")))


def test_the_black_and_white_image_scores_255():
    img = pc.image("bw")
    assert set(np.unique(img)) == {0, 255}
    d, loc, aux = pc.mirror("score255")
    assert len(d) >= pc.FLOOR and (aux[:, 0] == 255).all()
    assert len(np.unique(aux[:, 1])) >= 20 and len(np.unique(d, axis=0)) == len(d)   # distinct orientations and descriptors
    # threshold 255 refuses exactly these: the plane at threshold 254 holds them, at 255 nothing
    margin = fc.tables().margin
    assert (fmir.scores(fmir.gray_plane(img), 254, margin) == 255).sum() >= len(d)
    assert not fmir.scores(fmir.gray_plane(img), 255, margin).any()
    assert pc.BY_ID["thr255-bw"].thr == 255


def test_a_score_equal_to_the_threshold_is_no_corner():
    """`s > t`: the 100x140 image has pixels that score exactly the threshold 25 of its cases, and they change the result."""
    gray = fmir.gray_plane(pc.image("100x140"))
    margin = fc.tables().margin
    assert (fmir.scores(gray, 0, margin) == 25).sum() >= 5
    assert (fmir.suppress(fmir.scores(gray, 24, margin)) > 0).sum() != pc.BY_ID["q0"].count


def test_refused_parameters_are_outside_the_abi():
    for thr, num, den in pc.REFUSED:
        assert not (0 <= thr <= 255 and 0 < den <= pc.DEN_MAX and 0 <= num <= den)
