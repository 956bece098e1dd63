"""The strongest-N cases of SIFT and SURF on their CPU references alone (oracle.sift, tests/surf_mirror.py, tests/strongest_mirror.py):
every figure strongest_cases.py quotes - row counts, the cuts that fall inside a tie - and the mirror's tie rule.  No device."""
import numpy as np
import pytest

import strongest_cases as sc
import strongest_mirror as stm


def test_the_mirror_keeps_the_lower_index_on_ties_and_canonical_order():
    r = np.array([1.0, 3.0, 3.0, 0.0, 3.0, 2.0, 1.0], np.float32)
    assert stm.keep(r, 1).tolist() == [1] and stm.keep(r, 2).tolist() == [1, 2] and stm.keep(r, 3).tolist() == [1, 2, 4]
    assert stm.keep(r, 4).tolist() == [1, 2, 4, 5] and stm.keep(r, 5).tolist() == [0, 1, 2, 4, 5]
    assert stm.keep(r, 7).tolist() == list(range(7)) and stm.keep(r, 100).tolist() == list(range(7))
    # f32 values compare as their u32 bit patterns when none is negative: the device's sort key
    v = np.abs(np.random.default_rng(0).standard_normal(1000)).astype(np.float32)
    v[::7] = v[3]
    v[5] = 0.0
    by_bits = np.sort(np.argsort((~v.view(np.uint32)).astype(np.uint64), kind='stable')[:300])
    assert np.array_equal(stm.keep(v, 300), by_bits)
    with pytest.raises(ValueError):
        stm.keep(r, 0)


@pytest.mark.parametrize("name", list(sc.SIFT_CASES))
def test_sift_cases_have_the_rows_and_ties_they_claim(name):
    d, loc, aux = sc.sift_reference(name)
    rows, second = sc.SIFT_CASES[name][4:6]
    assert len(d) == rows and (aux[:, 2] >= 0).all()
    assert int((np.diff(loc, axis=0) == 0).all(1).sum()) == second   # rows that repeat the keypoint before them
    within = stm.tie_cuts(aux, loc, cross=False)
    for n in sc.SIFT_TIE_CUTS.get(name, ()):
        assert n in within and n in sc.sift_Ns(name)
    assert all(1 <= n for n in sc.sift_Ns(name))
    if name == "120x160":
        assert set(sc.sift_Ns(name)) >= {rows - 1, rows, rows + 1}
    if name == "twin":
        cross = stm.tie_cuts(aux, loc, cross=True)
        assert len(np.unique(aux[:, 2])) == sc.TWIN_DISTINCT and cross[:4] == [1, 4, 7, 9] and sc.sift_Ns(name) == (1, 4, 7, 9)
        for n in sc.sift_Ns(name):   # the cut separates the twins: the copy at the lower canonical index stays
            k, k1 = stm.keep(aux[:, 2], n), stm.keep(aux[:, 2], n + 1)
            new = np.setdiff1d(k1, k)
            out = np.setdiff1d(np.arange(rows), k)
            tied = out[aux[out, 2] == aux[new[0], 2]]
            assert len(new) == 1 and new[0] == tied.min()
    else:
        assert not stm.tie_cuts(aux, loc, cross=True)
    for N in sc.sift_Ns(name):   # the kept rows are rows of the reference, in its order
        kd, kl, ka = stm.pick((d, loc, aux), N)
        assert len(kd) == min(N, rows)


@pytest.mark.parametrize("name", list(sc.SURF_CASES))
def test_surf_cases_have_the_rows_and_ties_they_claim(name):
    img, (d, loc, aux) = sc.surf_reference(name)
    rows, Ns = sc.SURF_CASES[name][2:4]
    assert len(d) == rows and (aux[:, 2] > sc.SURF_CASES[name][1]).all()
    ties = stm.tie_cuts(aux, loc, cross=True)
    if name == "twin":
        assert len(np.unique(aux[:, 2])) == rows // 2 == 12 and ties == list(range(1, rows, 2))
        assert all(n in ties for n in Ns)
    else:
        assert not ties
    if name == "97x131":
        assert set(Ns) >= {rows - 1, rows, rows + 1}
    if name == "600x800":
        assert rows > 4096 > max(Ns)
