"""CPU tests of the restated selection / Upright rules (tests/kaze_select_mirror.py) and of the facts the device cases rest on:
the counts of the cases, the tie structure of the mirror-symmetric image, what uniform-N buys over strongest-N, and what Upright
buys on the nearly level homography pair.  No device, no library."""
import numpy as np
import pytest

import kaze_mirror as km
import kaze_select_cases as ksc
import kaze_select_mirror as ksm
import surf_mirror
import uniform_mirror as um


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


@pytest.mark.parametrize("name", list(ksc.COUNTS))
def test_case_counts(name):
    _, st = ksc.stages(name)
    assert st[3]["px"].size == ksc.COUNTS[name]


def test_the_unselected_mirror_is_kaze_mirror():
    img, d, loc, aux = ksc.mirror("97x131")
    ref = km.extract(img)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((d, loc, aux), ref))
    assert np.bincount(aux[:, 3].astype(int), minlength=8).tolist() == ksc.LEVELS_97x131
    assert len(np.unique(aux[:, 2])) == len(aux), "all metrics distinct: no cut of this case falls in a tie"
    small = ksm.extract(np.full((28, 300), 9, np.uint8), NumStrongest=5, Upright=True)
    assert [a.shape for a in small] == [(0, 64), (0, 2), (0, 4)]


def test_tie_image_has_88_pairs_of_equal_metrics():
    _, st = ksc.stages("tie")
    metric = st[3]["metric"]
    order = np.argsort(-metric.astype(np.float64), kind="stable")
    srt = metric[order].view(np.uint32)
    assert len(srt) == 176 and np.array_equal(srt[0::2], srt[1::2]) and len(np.unique(srt)) == 88
    cuts = [n for n in range(1, 176) if srt[n - 1] == srt[n]]
    assert cuts == list(range(1, 176, 2)), "every odd N cuts a pair, every even N cuts none"
    for N in (51, 52):   # the earlier row of a tied pair stays
        at = ksm.keep(st, NumStrongest=N)
        assert len(at) == N and np.array_equal(at, np.sort(order[:N]))
    assert order[50] < order[51] and order[50] in ksm.keep(st, NumStrongest=51) and order[51] not in ksm.keep(st, NumStrongest=51)


def test_selected_rows_are_rows_of_the_unselected_result():
    img, d, loc, aux = ksc.mirror("97x131")
    _, st = ksc.stages("97x131")
    for keys in ({"NumStrongest": 40}, {"NumUniform": 40}, {"NumUniform": 40, "UniformGrid": (32, 32)}):
        at = ksm.keep(st, **keys)
        sd, sloc, saux = ksc.mirror("97x131", **keys)[1:]
        assert len(at) == 40 and np.array_equal(bits(sd), bits(d[at])) and np.array_equal(bits(sloc), bits(loc[at]))
        assert np.array_equal(bits(saux), bits(aux[at]))
    for keys in ({"NumStrongest": 99}, {"NumStrongest": 500}, {"NumUniform": 99}, {"NumUniform": 500}):   # N >= count: the identity
        assert np.array_equal(ksm.keep(st, **keys), np.arange(99))
    for N in (1, 40, 98):   # a (1, 1) grid is strongest-N
        assert np.array_equal(ksm.keep(st, NumUniform=N, UniformGrid=(1, 1)), ksm.keep(st, NumStrongest=N))
    with pytest.raises(ValueError):
        ksm.keep(st, NumStrongest=5, NumUniform=5)
    for keys in ({"NumStrongest": 0}, {"NumUniform": 0}):
        with pytest.raises(ValueError):
            ksm.keep(st, **keys)


def test_uniform_spreads_the_rows_and_strongest_does_not():
    """pairA, 1090 candidates, 8 x 8 grid.  Measured: N = 146 uniform 64 cells (at most 3 rows in one), strongest 45 cells (8);
    N = 58 uniform 58 cells (1), strongest 31 cells (4)."""
    _, st = ksc.stages("pairA")
    seg = ksm.cells(st)
    occ = lambda at: um.occupancy(seg, at, 64)   # noqa: E731
    u, s = occ(ksm.keep(st, NumUniform=146)), occ(ksm.keep(st, NumStrongest=146))
    print("N=146: uniform %d cells (max %d), strongest %d cells (max %d)" % ((u > 0).sum(), u.max(), (s > 0).sum(), s.max()))
    assert u.sum() == s.sum() == 146
    assert (u > 0).sum() == 64 and u.max() <= 3
    assert (s > 0).sum() < 64 and s.max() > 3
    u, s = occ(ksm.keep(st, NumUniform=58)), occ(ksm.keep(st, NumStrongest=58))
    print("N=58: uniform %d cells (max %d), strongest %d cells (max %d)" % ((u > 0).sum(), u.max(), (s > 0).sum(), s.max()))
    assert (u > 0).sum() == 58 and u.max() == 1
    assert (s > 0).sum() < 58 and s.max() > 1


def test_upright_changes_the_descriptor_and_the_angle_only():
    for name in ("97x131", "pairA"):
        _, d, loc, aux = ksc.mirror(name)
        _, ud, uloc, uaux = ksc.mirror(name, Upright=True)
        assert np.array_equal(bits(uloc), bits(loc)) and np.array_equal(bits(uaux[:, [0, 2, 3]]), bits(aux[:, [0, 2, 3]]))
        assert not uaux[:, 1].view(np.uint32).any(), "angle_deg is +0.0"
        assert ud.shape == d.shape and (ud != d).any(1).mean() > 0.9
        assert np.allclose(np.linalg.norm(ud.astype(np.float64), axis=1), 1.0, atol=1e-5)


def test_upright_gives_more_correct_matches_on_the_nearly_level_pair():
    """Ratio test at 0.6, matches within 2 px of PAIR_H (about 1.5 degrees of rotation).  Measured: KAZE 1090 / 1082 rows, oriented
    838 (836 correct), upright 1000 (998); SURF 584 / 570 rows, oriented 388 (387), upright 489 (489)."""
    A, B = ksc.pair()
    got = {}
    for up in (False, True):
        keys = {"Upright": True} if up else {}
        (_, dA, lA, _), (_, dB, lB, _) = ksc.mirror("pairA", **keys), ksc.mirror("pairB", **keys)
        got["KAZE", up] = (len(dA), len(dB)) + ksc.correct_matches(dA, lA, dB, lB)
        (dA, lA, _), (dB, lB, _) = surf_mirror.extract(A, upright=up), surf_mirror.extract(B, upright=up)
        got["SURF", up] = (len(dA), len(dB)) + ksc.correct_matches(dA, lA, dB, lB)
    for det in ("KAZE", "SURF"):
        print(det, "oriented", got[det, False], "upright", got[det, True])
        assert got[det, True][:2] == got[det, False][:2], "the same keypoints"
        assert got[det, True][3] > got[det, False][3], "more correct matches"
        assert got[det, True][3] >= 0.95 * got[det, True][2]
