"""FAST/FREAK strongest-N on its NumPy restatement alone (tests/fast_strongest_mirror.py): hand cases of the Harris response,
the quotas, the carry, and the figures the device tests rely on.  No library, no device: the tables are
fast_mirror.contract_tables()."""
import numpy as np
import pytest

import fast_pyramid_cases as pc
import fast_strongest_cases as sc
import fast_strongest_mirror as smir

PLAN_120x160 = pc.PLANS["120x160"]


def test_harris_hand_cases():
    at = ([10], [10])
    for v in (1, 7, 235):
        g = np.full((21, 21), 20, np.int64)
        g[10, 10] += v
        # the 8 neighbours see the pixel: Ix = (-v, 0, v | -2v, 2v), Iy alike: A = B = 12 v^2, C = 0; 25 * 144 - 576 = 3024
        assert smir.harris(g, *at).tolist() == [3024 * v ** 4]
    assert smir.harris(np.full((21, 21), 77, np.int64), *at).tolist() == [0]
    step = np.zeros((21, 21), np.int64)
    step[:, 10:] = 255   # Ix = 1020 in the two columns beside the edge, 7 rows each: A = 14 * 1020^2, B = C = 0
    assert smir.harris(step, *at).tolist() == [-(14 * 1020 ** 2) ** 2] == [-212156703360000]
    y, x = np.mgrid[0:9, 0:9]
    quad = ((y > 4) ^ (x > 4)).astype(np.int64) * 255
    assert smir.harris(quad, [4], [4]).tolist() == [2750460118560000]
    # several pixels at once, and a uint8 plane
    g = np.full((30, 40), 20, np.uint8)
    g[10, 10], g[20, 30] = 80, 120
    assert smir.harris(g, [10, 20, 15], [10, 30, 20]).tolist() == [3024 * 60 ** 4, 3024 * 100 ** 4, 0]


def test_harris_bounds():
    """The contract's extremes stay inside 57 bits after the offset of 2^54."""
    y, x = np.mgrid[0:9, 0:9]
    for g in (((y > 4) ^ (x > 4)) * 255, ((y + x) % 2) * 255, (x > 4) * 255, (y % 2) * 255):
        R = int(smir.harris(g.astype(np.int64), [4], [4])[0])
        assert -2 ** 54 < R < 2 ** 56 and 0 <= R + 2 ** 54 < 2 ** 57


def test_quotas_of_120x160():
    assert smir.quotas(PLAN_120x160, 1) == [1, 0, 0, 0]
    assert smir.quotas(PLAN_120x160, 3) == [1, 1, 1, 0]
    assert smir.quotas(PLAN_120x160, 100) == [33, 27, 22, 18]
    for N in (1, 2, 5, 99, 400, 1515, 5000, 2 ** 31 - 1):
        assert sum(smir.quotas(PLAN_120x160, N)) == N
    assert smir.quotas([(120, 160)], 17) == [17]


def test_carry():
    M = [825, 420, 208, 63]
    assert smir.kept_per_level(M, smir.quotas(PLAN_120x160, 400), 400) == [129, 108, 100, 63]
    assert smir.kept_per_level(M, smir.quotas(PLAN_120x160, 5000), 5000) == M
    assert smir.kept_per_level(M, smir.quotas(PLAN_120x160, 1516), 1516) == M
    k = smir.kept_per_level(M, smir.quotas(PLAN_120x160, 1515), 1515)
    assert sum(k) == 1515 and all(a <= b for a, b in zip(k, M))
    # lopsided: level 0 is short, what it cannot use is dropped
    assert smir.kept_per_level([2, 500], [60, 40], 100) == [2, 40]


def test_carry_with_an_empty_level():
    desc, loc, aux, R, shapes = sc.candidates("200x300x3")
    assert len(shapes) == 8 and pc.per_level(aux, 8) == pc.CASES["200x300x3"][4]
    d, l, a = sc.mirror("200x300x3", 200)
    assert pc.per_level(a, 8) == [44, 37, 31, 53, 24, 10, 1, 0] and len(d) == 200


def test_120x160_selection():
    desc, loc, aux, R, shapes = sc.candidates("120x160")
    assert shapes == PLAN_120x160 and len(desc) == 1516
    for N, want in ((1, [1, 0, 0, 0]), (3, [1, 1, 1, 0]), (100, [33, 27, 22, 18]), (400, [129, 108, 100, 63])):
        d, l, a = sc.mirror("120x160", N)
        assert pc.per_level(a, 4) == want
        # canonical order, rows are candidates' rows, aux[3] is the response
        keep = smir.select(aux[:, 2], R, shapes, N)
        assert (np.diff(keep) > 0).all() and np.array_equal(d, desc[keep]) and np.array_equal(l, loc[keep])
        assert np.array_equal(a[:, :3], aux[keep, :3]) and np.array_equal(a[:, 3], R[keep].astype(np.float32))
        # every kept row of a level is at least as strong as every dropped one
        for lv in range(4):
            m = aux[:, 2] == lv
            kept = np.isin(np.flatnonzero(m), keep)
            if kept.any() and (~kept).any():
                assert R[m][kept].min() >= R[m][~kept].max()
    for N in (1516, 5000):
        d, l, a = sc.mirror("120x160", N)
        assert np.array_equal(d, desc) and np.array_equal(l, loc) and np.array_equal(a[:, :3], aux[:, :3])
    assert len(sc.mirror("120x160", 1515)[0]) == 1515
    with pytest.raises(ValueError):
        sc.mirror("120x160", 0)


def test_one_global_cut_would_starve_the_upper_levels():
    """Why there is a quota: the 379 strongest of all 1516 candidates lie on level 0 alone."""
    desc, loc, aux, R, shapes = sc.candidates("120x160")
    top = np.argsort(-R, kind="stable")[:379]
    assert pc.per_level(aux[top], 4) == [379, 0, 0, 0]


def test_96x131_level_1_is_short_by_one():
    desc, loc, aux, R, shapes = sc.candidates("96x131")
    assert pc.per_level(aux, 2) == [407, 78]
    q = smir.quotas(shapes, 200)
    assert q[1] == 79
    assert pc.per_level(sc.mirror("96x131", 200)[2], 2) == [q[0] + 1, 78]


@pytest.mark.parametrize("name", list(sc.TIES))
def test_ties_are_cut_in_canonical_order(name):
    nl, N = sc.TIES[name]
    desc, loc, aux, R, shapes = sc.candidates(name)
    m0 = np.flatnonzero(aux[:, 2] == 0)
    assert len(m0) == 1168 and len(shapes) == nl
    classes = np.unique(R[m0], return_counts=True)[1]
    assert classes.max() == 6
    k0 = smir.kept_per_level(pc.per_level(aux, nl), smir.quotas(shapes, N), N)[0]
    order = m0[smir.rank_order(R[m0])]
    assert R[order[k0 - 1]] == R[order[k0]]   # the cut falls inside a class of equal responses: this is what makes it a tie test
    keep = smir.select(aux[:, 2], R, shapes, N)
    cls = m0[R[m0] == R[order[k0 - 1]]]       # (ascending: canonical order)
    n_in = int(np.isin(cls, keep).sum())
    assert 0 < n_in < len(cls) and np.array_equal(cls[:n_in], cls[np.isin(cls, keep)])


def test_twin_pair():
    """A with 3 levels and N = 600 keeps all of its quota at level 2; those rows are single-level B's strongest 164, byte for
    byte; the two 600-row sets match in exactly the 164 twins, at distance 0."""
    import fast_cases as fc

    da, la, aa = sc.mirror("twinA", 600)
    assert pc.per_level(aa, 3) == [238, 198, 164]
    db1, lb1, ab1 = sc.mirror("twinB1", 164)
    at2 = np.flatnonzero(aa[:, 2] == 2)
    assert np.array_equal(da[at2], db1) and np.array_equal(aa[at2][:, [0, 1, 3]], ab1[:, [0, 1, 3]])
    db, lb, ab = sc.mirror("twinB", 600)
    assert pc.per_level(ab, 3) == [238, 227, 135] and len(sc.candidates("twinB")[0]) == 1202
    m, d = fc.match_binary(da, db, 0.6, 20.0)
    assert len(m) == 164
    got = {(int(i), int(j)): float(v) for (i, j), v in zip(m, d)}
    # B's level-0 rows among its 600 that are the twins: the same pixels as single-level B's strongest 164
    rows_b = {tuple(r): i for i, r in enumerate(lb.tolist())}
    twins = [(int(at2[t]) + 1, rows_b[tuple(lb1[t].tolist())] + 1) for t in range(164)]
    assert all(got.get(t) == 0.0 for t in twins)
