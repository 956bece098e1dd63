"""CPU pins of the FAST/FREAK contract: analytic cases on the NumPy mirror (tests/fast_mirror.py) and the properties of the
integer pattern tables the library reports through aps_freak_pattern (no device needed)."""
import math

import numpy as np

import fast_cases as fc
import fast_mirror as fm


def tb():
    return fc.tables()


def test_single_bright_dot_is_one_keypoint_with_its_contrast_as_score():
    img = np.full((80, 90), 40, np.uint8)
    img[37, 52] = 190   # every ring pixel is darker by 150: each 9-arc's minimum of centre - ring is 150
    d, loc, aux = fm.extract(img, tb())
    assert loc.tolist() == [[53.0, 38.0]] and aux[0, 0] == 150.0 and d.shape == (1, 64)
    # a pixel three away sees the dot as ONE bright ring pixel: no arc of 9, score 0
    assert fm.scores(fm.gray_plane(img), 51, tb().margin)[37, 55] == 0


def test_l_corner_score_by_hand_and_one_keypoint_after_suppression():
    """Bright quadrant 200 on 50 with its corner pixel at 220.  At the corner the ring has 5 pixels inside the quadrant
    ((3,0) (3,1) (2,2) (1,3) (0,3)) and 11 contiguous ones outside: centre - ring = 170 on an arc of 9, so s = 170.  Its
    neighbours inside the quadrant score 200 - 50 = 150 at most and are suppressed or tie with each other."""
    img = np.full((90, 90), 50, np.uint8)
    img[40:, 45:] = 200
    img[40, 45] = 220
    g = fm.gray_plane(img)
    S = fm.scores(g, 51, tb().margin)
    assert S[40, 45] == 170 and S[41, 46] == 150 and S[40, 46] == 150
    ys, xs, sc = fm.detect(g, 51, 100000, 1000000, tb().margin)
    assert list(zip(ys.tolist(), xs.tolist(), sc.tolist())) == [(40, 45, 170)]


def test_two_equal_adjacent_scores_are_both_dropped():
    img = np.full((80, 80), 10, np.uint8)
    img[40, 40] = img[40, 41] = 210   # neither lies on the other's ring: both score 200, neither is strictly greater
    g = fm.gray_plane(img)
    S = fm.scores(g, 51, tb().margin)
    assert S[40, 40] == 200 and S[40, 41] == 200
    assert len(fm.detect(g, 51, 100000, 1000000, tb().margin)[0]) == 0
    img[40, 41] = 209
    assert fm.detect(fm.gray_plane(img), 51, 100000, 1000000, tb().margin)[0].tolist() == [40]


def test_quality_gate_at_its_exact_boundary():
    img = np.full((80, 120), 0, np.uint8)
    img[40, 40], img[40, 80] = 200, 20
    t = int(math.floor(0.05 * 255))   # 12
    got = fm.extract(img, tb(), MinContrast=0.05, MinQuality=0.1)[2][:, 0].tolist()
    assert got == [200.0, 20.0]       # 20 * 10^6 >= 200 * 10^5: kept at equality
    img[40, 80] = 19
    assert fm.extract(img, tb(), MinContrast=0.05, MinQuality=0.1)[2][:, 0].tolist() == [200.0]
    assert t == 12 and fm.extract(img, tb(), MinContrast=0.05, MinQuality=0.0)[2][:, 0].tolist() == [200.0, 19.0]


def test_quarter_turned_pattern_on_quarter_turned_image_gives_the_same_bytes():
    """Tables k and k + 64 are exact quarter turns of each other, so describing the clockwise-turned image at the turned
    location with bin + 64 compares the very same box sums."""
    A = fc.noise_rects(5, 97, 113)
    B = np.ascontiguousarray(np.rot90(A, -1))   # B[x, h-1-y] = A[y, x]
    h = A.shape[0]
    IA, IB = fm.integral(fm.gray_plane(A)), fm.integral(fm.gray_plane(B))
    ys, xs = np.array([30, 48, 60, 73]), np.array([25, 56, 80, 89])
    for b in (0, 17, 63, 64, 200, 255):
        bins = np.full(4, b)
        da = fm.describe(IA, ys, xs, bins, tb())
        db = fm.describe(IB, xs, h - 1 - ys, (bins + 64) % 256, tb())
        assert np.array_equal(da, db), b
    assert len({bytes(r) for r in fm.describe(IA, ys, xs, np.zeros(4, np.int64), tb())}) == 4


def test_zero_moment_gives_bin_zero():
    """All 256 projections are 0 and tie: bin 0.  A single dot on a flat field is such a keypoint (the three outer rings'
    boxes do not reach the centre pixel), so the planted GPU case holds the device's in-lane and lane-ballot tie-breaks
    to this too."""
    img = np.full((70, 70), 77, np.uint8)
    I = fm.integral(fm.gray_plane(img))
    assert [m.tolist() for m in fm.moment(I, np.array([35]), np.array([35]), tb())] == [[0], [0]]
    assert fm.orientation(I, np.array([35]), np.array([35]), tb()).tolist() == [0]
    img, pts = fc.planted()   # its isolated dots (no other dot within the pattern's reach) are such keypoints
    ys, xs = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    mx, my = fm.moment(fm.integral(fm.gray_plane(img)), ys, xs, tb())
    zero = (mx == 0) & (my == 0)
    assert zero.sum() >= 3 and not fm.extract(img, tb())[2][zero, 1].any()


def test_a_tie_between_two_nonzero_bins_goes_to_the_lower_bin():
    """(Mx, My) = n * (s_j - s_k, c_k - c_j) is perpendicular to the chord between the table entries of the adjacent bins k
    and j = k + 1 and points outward: both project equally, and more than every other bin."""
    cs = tb().cos_sin
    for k in (0, 10, 31, 63, 64, 100, 127, 200, 254, 255):
        j = (k + 1) % 256
        mx, my = 12345 * (cs[j, 1] - cs[k, 1]), 12345 * (cs[k, 0] - cs[j, 0])
        proj = mx * cs[:, 0] + my * cs[:, 1]
        assert proj[k] == proj[j] == proj.max() > 0 and (proj == proj.max()).sum() == 2, k
        assert fm.bin_of([mx], [my], tb()).tolist() == [min(k, j)], k


# ---- the tables -------------------------------------------------------------------------------------------------------
def test_library_tables_are_the_contracts():
    want = fm.contract_tables()
    got = tb()
    for name in fm.Tables._fields:
        assert np.array_equal(getattr(got, name), getattr(want, name)), name


def test_512_distinct_pairs_with_distinct_ends_coarse_to_fine():
    p = tb().pairs
    assert p.shape == (512, 2) and len({tuple(r) for r in p.tolist()}) == 512
    assert (p[:, 0] < p[:, 1]).all() and p.min() >= 0 and p.max() <= 42
    key = [(fm.ring_of(a) + fm.ring_of(b), a, b) for a, b in p.tolist()]
    assert key == sorted(key)
    rest = [(fm.ring_of(a) + fm.ring_of(b), a, b) for a in range(43) for b in range(a + 1, 43) if (a, b) not in set(map(tuple, p.tolist()))]
    assert len(rest) == 903 - 512 and min(rest) > max(key)


def test_rotated_entries_follow_the_f64_rotation_of_orientation_zero():
    l0 = np.array(fm.layout0())   # x, y, sigma in pixels
    f = tb().fields
    for k in range(256):
        a = 2.0 * math.pi * k / 256.0
        x = l0[:, 0] * math.cos(a) - l0[:, 1] * math.sin(a)
        y = l0[:, 0] * math.sin(a) + l0[:, 1] * math.cos(a)
        assert np.abs(f[k, :, 0] - x).max() <= 1.0 and np.abs(f[k, :, 1] - y).max() <= 1.0, k
        assert np.array_equal(f[k, :, 2], f[0, :, 2]) and (f[k, :, 2] >= 0).all()
        assert np.array_equal(f[(k + 64) % 256, :, 0], -f[k, :, 1]) and np.array_equal(f[(k + 64) % 256, :, 1], f[k, :, 0])
    assert f[0, ::6, 2].tolist() == [7, 6, 4, 3, 2, 1, 1, 1] and f[:, 42, :2].max() == 0


def test_margin_orientation_pairs_and_direction_tables():
    t = tb()
    assert t.margin == int((np.maximum(np.abs(t.fields[..., 0]), np.abs(t.fields[..., 1])) + t.fields[..., 2] + 1).max()) == 23
    assert t.ori_pairs.shape == (45, 2) and len({tuple(r) for r in t.ori_pairs.tolist()}) == 45
    assert all(a // 6 == b // 6 and a // 6 < 3 and a < b for a, b in t.ori_pairs.tolist())
    n = np.hypot(t.ori_dir[:, 0], t.ori_dir[:, 1])
    assert np.abs(n - 1024.0).max() <= 1.0
    cs = t.cos_sin
    assert cs[0].tolist() == [16384, 0] and cs[64].tolist() == [0, 16384] and cs[128].tolist() == [-16384, 0]
    assert np.abs(np.hypot(cs[:, 0], cs[:, 1]) - 16384.0).max() <= 1.0


def test_nothing_overflows_for_uint8_input():
    """The contract's bound: |D| <= 255 * 225 * 225 per orientation pair, 45 pairs, directions <= 2^10, tables <= 2^14."""
    t = tb()
    area = (2 * t.fields[0][:, 2] + 1) ** 2
    assert area.max() == 225
    d_max = 255 * int(area.max()) ** 2
    m_max = 45 * d_max * 1024
    assert 2 * m_max * 16384 < 2 ** 63 and d_max < 2 ** 31
