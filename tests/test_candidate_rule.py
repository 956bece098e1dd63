"""The top-m candidate rule (imageMatching.candidate_positions, candidate_pairs, and the >= 4 filter the callers apply) against a
loop restatement of imageMatching.m:76-100.  Device-free and exact: the rule is integer bookkeeping, and ties in the symmetric
counts - where a sort that is not stable, or a walk in the wrong order, would show - are most of the cases."""
from importlib import import_module

import numpy as np
import pytest


@pytest.fixture(scope="module")
def im(aps):
    return import_module(aps.__name__ + ".imageMatching")


def pair_order(n):
    """featureMatchingPairwise.m:48: pair (i, j), i < j, at j (j - 1) / 2 + i."""
    return [(i, j) for j in range(1, n) for i in range(j)]


def restated(sym, n, m):
    """imageMatching.m:76-100 in loops, on the full symmetric count table: the candidate pairs (i, j), i < j, in find's order."""
    symCounts = [[0 if i == j else int(sym[i][j]) for j in range(n)] for i in range(n)]      # :76-86, zero diagonal
    cand = [[False] * n for _ in range(n)]
    for i in range(n):
        idx = sorted(range(n), key=lambda j: -symCounts[i][j])                                  # :88-90, stable, descending
        for j in idx[: min(m, n - 1)]:                                                          # :91-95
            cand[i][j] = True
    out = []
    for j in range(n):                                                                          # :100, column-major
        for i in range(j):                                                                      # :99, upper triangle
            if cand[i][j] or cand[j][i]:                                                        # :96-98
                out.append((i, j))
    return out


def table(n_match, n):
    sym = np.zeros((n, n), np.int64)
    for p, (i, j) in enumerate(pair_order(n)):
        sym[i, j] = sym[j, i] = n_match[p]
    return sym


def cells(n_match, n, rng):
    """A cell array with the pair counts: matches of pair (i, j) in cell (i, j), None or empty elsewhere; a diagonal cell that is
    not empty must not count."""
    c = [[None] * n for _ in range(n)]
    for p, (i, j) in enumerate(pair_order(n)):
        c[i][j] = np.zeros((int(n_match[p]), 2))
        if rng.integers(2):
            c[j][i] = np.zeros((0, 2))
    if n:
        c[0][0] = np.zeros((50, 2))
    return c


def check(im, n_match, n, m, rng):
    n_match = np.asarray(n_match, np.int64)
    want = restated(table(n_match, n), n, m)
    order = pair_order(n)
    pos = im.candidate_positions(n_match, n, m)
    assert [order[p] for p in np.asarray(pos).tolist()] == want, (n, m, n_match.tolist())
    assert im.candidate_pairs(cells(n_match, n, rng), n, m) == want, (n, m, n_match.tolist())
    return want


def draws(rng, P):
    """Counts from 0..1, 0..5 and 0..39, all equal (every comparison a tie), and each of those with half the pairs zeroed."""
    out = [rng.integers(0, hi + 1, P) for hi in (1, 5, 39)] + [np.full(P, 7), np.zeros(P, np.int64)]
    return out + [np.where(rng.random(P) < 0.5, 0, a) for a in out[:4]]


def test_random_counts_with_heavy_ties(im):
    rng = np.random.default_rng(2024)
    cases = 0
    for n in range(1, 10):
        for m in range(1, 8):
            for n_match in draws(rng, n * (n - 1) // 2):
                check(im, n_match, n, m, rng)
                cases += 1
    assert cases == 9 * 7 * 9


def test_no_more_images_than_m(im):
    """n <= m: every image names all the others, so every pair is a candidate, whatever the counts."""
    rng = np.random.default_rng(1)
    for n, m in ((3, 3), (4, 6), (6, 6), (7, 7)):
        for n_match in (np.zeros(n * (n - 1) // 2, np.int64), rng.integers(0, 9, n * (n - 1) // 2)):
            assert check(im, n_match, n, m, rng) == pair_order(n)


def test_one_and_two_images(im):
    rng = np.random.default_rng(2)
    for m in (1, 6):
        assert check(im, [], 1, m, rng) == []
        assert check(im, [0], 2, m, rng) == [(0, 1)]
        assert check(im, [25], 2, m, rng) == [(0, 1)]


def test_an_image_without_matches_names_the_lowest_indices(im):
    """Image 3 of 5 matches nothing: its sorted row is 0, 1, 2, 3, 4, its top 2 are images 0 and 1, and for image 0 of the same
    kind the top 2 are itself and image 1 - the diagonal entry drops out with the upper triangle."""
    rng = np.random.default_rng(3)
    n, m = 5, 2
    sym = np.zeros((n, n), np.int64)
    sym[1, 2] = sym[2, 1] = 9
    sym[2, 4] = sym[4, 2] = 8
    sym[1, 4] = sym[4, 1] = 7
    n_match = [sym[i, j] for (i, j) in pair_order(n)]
    got = check(im, n_match, n, m, rng)
    # rows: 0 -> {0, 1}, 1 -> {2, 4}, 2 -> {1, 4}, 3 -> {0, 1}, 4 -> {2, 1}
    assert got == [(0, 1), (1, 2), (0, 3), (1, 3), (1, 4), (2, 4)]


def test_a_tie_for_the_last_place_goes_to_the_lower_index(im):
    """Images 2 and 3 tie for the second place of image 0 (m = 2): image 2 is named, image 3 is not - and nobody else names the
    pair (0, 3)."""
    rng = np.random.default_rng(4)
    n, m = 5, 2
    sym = np.zeros((n, n), np.int64)
    for (i, j), v in {(0, 1): 30, (0, 2): 10, (0, 3): 10, (3, 4): 50, (1, 3): 40, (2, 4): 45, (1, 2): 35}.items():
        sym[i, j] = sym[j, i] = v
    got = check(im, [sym[i, j] for (i, j) in pair_order(n)], n, m, rng)
    assert (0, 2) in got and (0, 3) not in got


def test_the_four_match_boundary(im):
    """imageMatching.m:133: a candidate pair goes to RANSAC with at least 4 putative matches - the filter expression of
    pipeline.match_and_verify and parallel._match_pass, on 3 and 4 matches."""
    n, m = 3, 6
    n_match = np.asarray([3, 4, 0], np.int64)  # pairs (0, 1), (0, 2), (1, 2)
    pw = im.candidate_positions(n_match, n, m)
    assert np.asarray(pw).tolist() == [0, 1, 2]
    work = pw[n_match[pw] >= 4].tolist()
    assert work == [1]
    assert [pair_order(n)[p] for p in work] == [(0, 2)]
