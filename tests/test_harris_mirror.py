"""The Harris mirror's own invariants (tests/harris_mirror.py on tests/harris_cases.py; CPU, the library's tables but no device):
the cases reach the risks they are there for, and every row restates the contract it came from."""
import functools

import numpy as np
import pytest

import fast_cases as fc
import fast_pyramid_mirror as pmir
import fast_strongest_mirror as smir
import harris_cases as hc
import harris_mirror as hm
import uniform_mirror as umir


@functools.lru_cache(maxsize=None)
def levels(name):
    """[(plane, dense R, ys, xs, R, candidates before the gate)] per level of the case."""
    c = hc.CASES[name]
    qn, qd = hm.quality_rational(c.quality)
    out = []
    for g in pmir.planes(hc.image(name), c.levels, c.scale, hc.MARGIN):
        out.append((g, hm.dense(g)) + hm.detect(g, qn, qd, hc.MARGIN))
    return out


@functools.lru_cache(maxsize=None)
def cand(name):
    c = hc.CASES[name]
    return hm.candidates(hc.image(name), fc.tables(), "FREAK", c.levels, c.scale, c.quality)


def test_margin_is_the_pattern_margin():
    assert fc.tables().margin == hc.MARGIN == 23 and hm.REACH == 4


@pytest.mark.parametrize("name", list(hc.CASES))
def test_rows_and_order(name):
    c = hc.CASES[name]
    desc, loc, aux, R, shapes = cand(name)
    assert len(desc) == len(loc) == len(aux) == len(R) >= c.min_rows
    if c.min_rows == 0:
        assert len(R) == 0 and all(int(d.max()) <= 0 for _, d, *_ in levels(name))   # R <= 0 everywhere: no rows, no error
        return
    assert len(shapes) == c.levels and (R > 0).all() and not aux[:, 3].any()
    assert np.array_equal(aux[:, 0], R.astype(np.float32))
    at = 0
    for l, (g, d, ys, xs, Rl, _) in enumerate(levels(name)):
        n = len(ys)
        assert (aux[at:at + n, 2] == l).all()
        key = ys * g.shape[1] + xs
        assert (np.diff(key) > 0).all()   # ascending (row, col) within the level
        h, w = g.shape
        assert ((ys >= hc.MARGIN) & (ys <= h - 1 - hc.MARGIN) & (xs >= hc.MARGIN) & (xs <= w - 1 - hc.MARGIN)).all()
        # every row's R is the per-pixel response of the strongest-N contract at that pixel
        assert np.array_equal(Rl, smir.harris(g, ys, xs)) and np.array_equal(Rl, R[at:at + n])
        assert np.array_equal(loc[at:at + n], pmir.loc_of(xs, ys, g.shape, shapes[0]))
        # strictly above the eight neighbours, which count with their own R also outside the band
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dy, dx) != (0, 0):
                    assert (Rl > d[ys + dy, xs + dx]).all()
        at += n
    assert at == len(R)


def test_dense_is_zero_where_the_window_does_not_fit():
    g = pmir.planes(hc.image("70x200"), 1, 1.2, hc.MARGIN)[0]
    d = hm.dense(g)
    inner = np.zeros(d.shape, bool)
    inner[hm.REACH:-hm.REACH, hm.REACH:-hm.REACH] = True
    assert not d[~inner].any() and (d[inner] != 0).any()
    assert not hm.dense(np.zeros((8, 30), np.int64)).any()   # no pixel has a window


def test_the_gate_drops_candidates_in_several_cases():
    dropped = [name for name in hc.CASES if any(before > len(ys) for _, _, ys, _, _, before in levels(name))]
    assert len(dropped) >= 2 and "saturated_top" in dropped, dropped
    (_, _, ys, _, R, before), = levels("saturated_top")
    assert before > 1 and len(ys) == 1   # only Rmax itself passes (2^24 - 1) / 2^24


def test_one_pixel_band_yields_its_pixel():
    (_, _, ys, xs, _, _), = levels("47x47")
    assert ys.tolist() == [23] and xs.tolist() == [23]


def test_rows_on_both_sides_of_the_seams():
    (_, _, ys, xs, _, _), = levels("70x200")    # the lattice patch: apexes past the seams
    assert 64 in xs.tolist() and {32, 40} <= set(ys.tolist())
    (_, _, ys, xs, _, _), = levels("47x129")    # apexes on 23 + 8 k: before the seams
    assert 63 in xs.tolist()
    (_, _, ys, xs, _, _), = levels("63x65")
    assert {31, 39} <= set(ys.tolist())
    (_, _, ys, xs, _, _), = levels("55x64")
    assert 31 in ys.tolist() and 23 in ys.tolist()   # the first and the last band row


def test_plateau_keeps_neither_of_a_tied_pair():
    (g, d, ys, xs, _, _), = levels("plateau")
    h, w = g.shape
    assert w % 2 == 0 and np.array_equal(d, d[:, ::-1])
    a, b = w // 2 - 1, w // 2
    rows = np.arange(hc.MARGIN, h - hc.MARGIN)
    nb = np.stack([d[rows + dy, x] for dy in (-1, 0, 1) for x in (a - 1, a, b, b + 1)])
    tied_top = (d[rows, a] > 0) & (d[rows, a] == nb.max(0))   # a pair that ties at the maximum of its neighbourhood
    assert tied_top.any()
    assert not ((xs == a) | (xs == b))[np.isin(ys, rows[tied_top])].any()
    assert len(ys) >= 1


@pytest.mark.parametrize("name", hc.SATURATED)
def test_the_gate_needs_128_bits(name):
    qn, qd = hm.quality_rational(hc.CASES[name].quality)
    (_, _, ys, _, R, before), = levels(name)
    top = int(R.max())
    assert qd <= 1 << 24 and top * qn >= 1 << 64 and top * qd >= 1 << 64   # both sides of the comparison pass 64 bits
    # and a comparison in wrapped 64-bit arithmetic would decide at least one candidate differently
    g, d, *_ = levels(name)[0]
    cy, cx = np.nonzero(hm.suppress(d, hc.MARGIN))
    Rc = [int(v) for v in d[cy, cx]]
    exact = [r * qd >= top * qn for r in Rc]
    wrapped = [(r * qd) % (1 << 64) >= (top * qn) % (1 << 64) for r in Rc]
    assert exact != wrapped and sum(exact) == len(ys)


def test_selections_are_rows_of_the_candidates():
    c = cand("pyramid")
    desc, loc, aux, R, shapes = c
    for N in (3, len(R) + 5):
        sd, sloc, saux = smir.pick(c, N)
        assert len(sd) == min(N, len(R)) and np.array_equal(saux[:, 3], saux[:, 0])
    d1, l1, a1 = umir.fast_pick(c, 7, (1, 1))
    d2, l2, a2 = smir.pick(c, 7)
    assert np.array_equal(d1, d2) and np.array_equal(l1, l2) and np.array_equal(a1, a2)
    d4, l4, a4 = umir.fast_pick(c, 7, (4, 4))
    assert len(d4) == 7


def test_orb_rows_share_everything_but_descriptor_and_bin():
    c = hc.CASES["63x65"]
    fd, floc, faux, fR, _ = cand("63x65")
    od, oloc, oaux, oR, _ = hm.candidates(hc.image("63x65"), fc.tables(), "ORB", c.levels, c.scale, c.quality)
    assert od.shape == (len(fd), 32) and np.array_equal(floc, oloc) and np.array_equal(fR, oR)
    assert np.array_equal(faux[:, [0, 2, 3]], oaux[:, [0, 2, 3]])
