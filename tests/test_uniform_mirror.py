"""Uniform-N selection on its NumPy restatement alone (tests/uniform_mirror.py): the water-filling's properties and hand cases, the
1 x 1 grid against strongest_mirror, and the occupancy figures of DESIGN.md "Uniform-N selection" on the SURF case pairA."""
import numpy as np
import pytest

import strongest_cases as sc
import strongest_mirror as stm
import uniform_mirror as um


def level_of(counts, keep):
    """The water level behind a keep vector: the smallest share among the cells that were cut (None when none was)."""
    cut = keep < counts
    return int(keep[cut].min()) if cut.any() else None


def check_waterfill(counts, Q):
    c = np.asarray(counts, np.int64)
    k = um.waterfill(c, Q)
    assert k.dtype == np.int64 and k.shape == c.shape
    assert int(k.sum()) == min(int(Q), int(c.sum())) and (k <= c).all() and (k >= 0).all()
    t = level_of(c, k)
    if t is not None:
        above = c > t
        assert int(k[above].max()) - int(k[above].min()) <= 1
        assert (k[~above] == c[~above]).all()                   # the cells at or below the level keep everything
        extra = np.flatnonzero(above & (k == t + 1))
        assert np.array_equal(extra, np.flatnonzero(above)[:len(extra)])   # the remainder goes to the first such cells
    return k


HAND = [
    ([5, 5, 5, 5], 12, [3, 3, 3, 3]),              # all counts equal
    ([5, 5, 5, 5], 14, [4, 4, 3, 3]),              # ... with a remainder: the first cells
    ([5, 5, 5, 5], 20, [5, 5, 5, 5]),
    ([3, 0, 7, 1, 0, 2], 3, [1, 0, 1, 1, 0, 0]),   # Q below the number of nonempty cells: t = 0, the first Q nonempty cells
    ([3, 0, 7, 1, 0, 2], 13, [3, 0, 7, 1, 0, 2]),  # Q = sum c
    ([3, 0, 7, 1, 0, 2], 12, [3, 0, 6, 1, 0, 2]),  # Q = sum c - 1
    ([0, 0, 9, 0], 4, [0, 0, 4, 0]),               # one cell holding everything
    ([0, 4, 0, 0, 4, 0, 4], 7, [0, 3, 0, 0, 2, 0, 2]),   # zeros between nonempty cells
    ([1, 10, 2, 10], 11, [1, 4, 2, 4]),
    ([1, 10, 2, 10], 12, [1, 5, 2, 4]),
    ([0, 0, 0], 5, [0, 0, 0]),
    ([7], 3, [3]),
]


@pytest.mark.parametrize("counts,Q,want", HAND)
def test_waterfill_hand_cases(counts, Q, want):
    assert check_waterfill(counts, Q).tolist() == want


def test_waterfill_properties_on_random_counts():
    rng = np.random.default_rng(11)
    for _ in range(300):
        m = int(rng.integers(1, 65))
        c = rng.integers(0, int(rng.choice([2, 5, 40, 1000])), m) * (rng.random(m) < rng.choice([0.3, 1.0]))
        for Q in {0, 1, int(c.sum()), max(int(c.sum()) - 1, 0), int(rng.integers(0, max(int(c.sum()), 1) + 1)), int(c.sum()) + 5}:
            check_waterfill(c.astype(np.int64), Q)


def test_cell_is_the_integer_rule():
    assert um.cell(0, 0, 97, 131, (3, 5)) == 0 and um.cell(96, 130, 97, 131, (3, 5)) == 14
    assert um.cell(32, 26, 97, 131, (3, 5)) == 0 and um.cell(33, 27, 97, 131, (3, 5)) == 1 * 5 + 1   # 33 * 3 // 97 = 1, 27 * 5 // 131 = 1
    py, px = np.mgrid[0:37, 0:41]
    c = um.cell(py, px, 37, 41, (32, 32))
    assert c.min() == 0 and c.max() == 1023 and (np.diff(c, axis=1) >= 0).all() and (np.diff(c, axis=0) >= 0).all()
    assert (um.cell(py, px, 37, 41, (1, 1)) == 0).all()


def test_grid_1x1_is_the_strongest_rule():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 20, 500).astype(np.float32)   # many ties
    for N in (1, 7, 250, 499, 500):
        assert np.array_equal(um.keep(s, np.zeros(500, np.int64), [N], 1), stm.keep(s, N))
    d, loc, aux = sc.sift_reference("120x160")
    for N in (1, 13, 100, 418, 419, 5000):
        assert np.array_equal(um.sift_keep((d, loc, aux), (120, 160), N, (1, 1)), stm.keep(aux[:, 2], N))


def test_keep_breaks_ties_to_the_lower_index_within_a_cell():
    s = np.array([5, 5, 5, 9, 5, 5], np.float32)
    seg = np.array([0, 1, 0, 1, 0, 1])
    assert um.keep(s, seg, [4], 2).tolist() == [0, 1, 2, 3]
    assert um.keep(s, seg, [3], 2).tolist() == [0, 2, 3]      # cell 0 takes the remainder
    assert um.keep(s.astype(np.int64), seg + 2, [0, 2], 2).tolist() == [0, 3]   # the second group


def _occupied(segment, at):
    return int((um.occupancy(segment, at, 64) > 0).sum())


def test_pairA_occupancy_figures():
    """SURF case pairA (240 x 320): 584 candidates in 64 of 64 cells; the strongest 146 occupy 55 cells with at most 7 rows in one,
    146 spread rows occupy 64 with at most 3; at N = 58 it is 38 cells against 58."""
    img, ref = sc.surf_reference("pairA")
    py, px, (H, W), metric = um.surf_pixels(img, sc.SURF_CASES["pairA"][1])
    seg = um.cell(py, px, H, W, (8, 8))
    assert len(metric) == 584 and _occupied(seg, np.arange(584)) == 64
    strong, spread = stm.keep(metric, 146), um.surf_keep(img, ref, 1000.0, 146)
    assert len(strong) == len(spread) == 146
    assert (_occupied(seg, strong), int(um.occupancy(seg, strong, 64).max())) == (55, 7)
    assert (_occupied(seg, spread), int(um.occupancy(seg, spread, 64).max())) == (64, 3)
    assert _occupied(seg, stm.keep(metric, 58)) == 38 and _occupied(seg, um.surf_keep(img, ref, 1000.0, 58)) == 58


def test_fast_budgets_are_the_strongest_calls_rows_per_level():
    import fast_strongest_cases as fsc
    import fast_strongest_mirror as smir

    for name, N in (("120x160", 400), ("200x300x3", 200), ("96x131", 200)):
        cand = fsc.candidates(name)
        level = cand[2][:, 2].astype(np.int64)
        at, seg = um.fast_keep(cand, N)
        strongest = smir.select(cand[2][:, 2], cand[3], cand[4], N)
        assert np.array_equal(np.bincount(level[at], minlength=len(cand[4])), np.bincount(level[strongest], minlength=len(cand[4])))
        assert np.array_equal(um.fast_keep(cand, N, (1, 1))[0], strongest)
        assert (seg // 64 == level).all()
