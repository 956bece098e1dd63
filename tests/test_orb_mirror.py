"""CPU tests of the NumPy restatement of the FAST/ORB contract (tests/orb_mirror.py): the generated pattern and the steering tables
against the contract's check values, the bin on hand cases, the descriptor on a ramp, and quarter-turn covariance on a real view.
No device; only the last test touches the package (the scene's CPU rendering)."""
import numpy as np

import fast_cases as fc
import fast_mirror as fmir
import orb_mirror as om


def test_generated_pattern_has_the_contracts_check_values():
    tests, draws = om.generate_tests()
    assert draws == 2084 and tests.shape == (256, 4)
    assert tests[:3].tolist() == [[4, -6, 2, 6], [-12, -2, -7, 8], [-3, -8, 1, 7]] and tests[255].tolist() == [4, 11, 1, 5]
    assert len({frozenset(((xa, ya), (xb, yb))) for xa, ya, xb, yb in tests.tolist()}) == 256   # all distinct, as unordered pairs
    assert ((tests[:, 0] ** 2 + tests[:, 1] ** 2 <= 169) & (tests[:, 2] ** 2 + tests[:, 3] ** 2 <= 169)).all()
    assert ((tests[:, 0] - tests[:, 2]) ** 2 + (tests[:, 1] - tests[:, 3]) ** 2 >= 16).all()
    assert np.array_equal(om.pattern()[0], tests)


def test_steering_tables_have_the_contracts_check_values():
    tests, table, disc, cs = om.pattern()
    assert table.shape == (256, 256, 4)
    assert table[17][5].tolist() == [7, 7, 10, 4] and table[63][255].tolist() == [-11, 4, -5, 1] and table[200][0].tolist() == [-5, -5, 6, -1]
    assert int(np.abs(table).sum()) == 1467840
    assert int(np.abs(table).max()) == 13 and om.reach(table) == om.REACH == 16 <= om.MARGIN
    assert np.array_equal(table[0], tests)   # bin 0 is the pattern itself
    assert not ((table[..., 0] == table[..., 2]) & (table[..., 1] == table[..., 3])).any()   # no test collapses to one point
    for k in range(192):   # exact quarter turns (dx, dy) -> (-dy, dx)
        assert np.array_equal(table[k + 64][:, [0, 2]], -table[k][:, [1, 3]]) and np.array_equal(table[k + 64][:, [1, 3]], table[k][:, [0, 2]])
    assert np.array_equal(cs, fmir.contract_tables().cos_sin)   # FREAK's table
    assert disc.shape == (709, 2) and (disc[:, 0] ** 2 + disc[:, 1] ** 2 <= 225).all() and len({tuple(d) for d in disc.tolist()}) == 709
    assert int(np.abs(disc[:, 0]).sum()) == 4528 and 255 * 4528 < 2 ** 21


def test_bin_on_hand_cases():
    for (du, dv), want in (((5, 0), 0), ((0, 5), 64), ((-5, 0), 128), ((0, -5), 192), ((4, 4), 32)):
        g = np.full((61, 61), 90, np.int64)
        g[30 + dv, 30 + du] = 200
        m10, m01 = om.moments(g, [30], [30])
        assert (int(m10[0]), int(m01[0])) == (110 * du, 110 * dv)
        assert om.bin_of(m10, m01).tolist() == [want], (du, dv)
    flat = np.full((61, 61), 90, np.int64)
    m10, m01 = om.moments(flat, [30], [30])
    assert (int(m10[0]), int(m01[0])) == (0, 0) and om.bin_of(m10, m01).tolist() == [0]
    # a pixel outside the disc does not count: (11, 11) has 242 > 225
    flat[41, 41] = 255
    assert om.bin_of(*om.moments(flat, [30], [30])).tolist() == [0]


def test_ramp_gives_bin_zero_and_the_sign_of_the_columns():
    g = np.tile(np.arange(256, dtype=np.int64), (80, 1))   # g[y, x] = x
    ys, xs = np.array([30, 40, 49]), np.array([23, 128, 232])
    bins = om.bin_of(*om.moments(g, ys, xs))
    assert bins.tolist() == [0, 0, 0]
    d = om.describe(g, ys, xs, bins)
    tests = om.pattern()[0]
    want = np.packbits((tests[:, 0] < tests[:, 2]).astype(np.uint8).reshape(32, 8), axis=1, bitorder="little").reshape(32)
    assert d.shape == (3, 32) and d.dtype == np.uint8 and all(np.array_equal(row, want) for row in d)
    assert (om.box5(g)[2:-2, 2:-2] <= 6375).all()


def test_quarter_turn_covariance_on_a_real_view():
    """np.rot90 of view 0 of the scene: the same 227 keypoints, every bin shifted by an exact quarter turn, every descriptor
    byte-identical to its twin's (the tables of bins k and k + 64 are exact quarter turns and the box is square)."""
    views, _ = fc.scene()
    g = fmir.gray_plane(views[0])
    h, w = g.shape
    ys, xs, sc, bins, d = om.level_rows(g, 0.08, 0.1)
    assert len(ys) == 227
    r = np.rot90(g)   # r[w - 1 - x, y] = g[y, x]
    rys, rxs, rsc, rbins, rd = om.level_rows(r, 0.08, 0.1)
    assert len(rys) == 227
    twin = {(int(y), int(x)): i for i, (y, x) in enumerate(zip(rys, rxs))}
    idx = np.array([twin[(w - 1 - int(x), int(y))] for y, x in zip(ys, xs)])
    assert sorted(idx.tolist()) == list(range(227))
    assert np.array_equal(rsc[idx], sc)
    # (u, v) -> (v, -u): the moment turns by -90 degrees in image coordinates, the bin by 192
    m10, m01 = om.moments(g, ys, xs)
    rm10, rm01 = om.moments(r, rys, rxs)
    assert np.array_equal(rm10[idx], m01) and np.array_equal(rm01[idx], -m10)
    assert np.array_equal(rbins[idx], (bins + 192) % 256)
    same = int((rd[idx] == d).all(1).sum())
    print("byte-identical twins: %d of 227" % same)
    assert same == 227
