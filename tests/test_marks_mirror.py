"""CPU tests of the mark contract's mirror (tests/marks_mirror.py) against closed forms: DESIGN.md, "Mark contract"."""
import numpy as np
import pytest

import annotate_mirror as am
import marks_mirror as mm

RED, GREEN = (255, 0, 0), (0, 255, 0)


def _rc(mask):
    return {(int(r) + 1, int(c) + 1) for r, c in zip(*np.nonzero(mask))}


def test_width_one_horizontal_segment_paints_its_row_only():
    assert _rc(mm.mark_mask(8, 9, mm.segment(2, 3, 6, 3, RED))) == {(3, c) for c in range(2, 7)}
    assert _rc(mm.mark_mask(8, 9, mm.segment(6, 3, 2, 3, RED))) == {(3, c) for c in range(2, 7)}  # direction does not matter


def test_width_one_diagonal_through_pixel_centres_is_the_bare_diagonal():
    # a neighbour of the diagonal is sqrt(1/2) px away, more than the half pixel of width 1
    assert _rc(mm.mark_mask(12, 12, mm.segment(2, 3, 9, 10, RED))) == {(k + 1, k) for k in range(2, 10)}
    assert _rc(mm.mark_mask(12, 12, mm.segment(2, 10, 9, 3, RED))) == {(12 - k, k) for k in range(2, 10)}


@pytest.mark.parametrize("p0,p1", [((2, 2), (29, 11)), ((3, 30), (17, 1)), ((1.3, 4.7), (28.4, 26.1)), ((5, 5), (6, 31))])
def test_width_one_segment_is_eight_connected_for_any_slope(p0, p1):
    """Along the major axis every column (row) the segment crosses holds a centre within half a pixel of it."""
    m = mm.mark_mask(32, 32, mm.segment(*p0, *p1, RED))
    major = 1 if abs(p1[0] - p0[0]) >= abs(p1[1] - p0[1]) else 0
    lo, hi = sorted((p0[1 - major], p1[1 - major]))
    for v in range(int(np.ceil(lo)), int(np.floor(hi)) + 1):
        assert m.take(v - 1, axis=major).any(), v
    painted = _rc(m)
    first = min(painted)
    todo, seen = [first], {first}
    while todo:  # flood fill over the 8-neighbourhood reaches every painted pixel
        r, c = todo.pop()
        for q in ((r + dr, c + dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1)):
            if q in painted and q not in seen:
                seen.add(q)
                todo.append(q)
    assert seen == painted


def test_ring_radius_three_width_one_is_the_closed_annulus_with_the_squares_symmetries():
    got = _rc(mm.mark_mask(21, 21, mm.ring(11, 11, 3, RED)))
    want = {(11 + dy, 11 + dx) for dy in range(-5, 6) for dx in range(-5, 6) if 2.5 ** 2 <= dx * dx + dy * dy <= 3.5 ** 2}
    assert got == want and len(got) == 16  # (0, 3), (1, 3), (2, 2) and their images: 4 + 8 + 4
    off = {(r - 11, c - 11) for r, c in got}
    for sym in (lambda y, x: (-y, x), lambda y, x: (y, -x), lambda y, x: (x, y)):  # generators of the eight symmetries
        assert {sym(y, x) for y, x in off} == off
    assert (11, 11) not in got and (11, 14) in got and (11, 13) not in got and (13, 13) in got  # d^2 = 9, 4, 8


def test_ring_bounds_are_closed_on_both_sides():
    # radius 2.5, width 1: 2^2 <= d^2 <= 3^2; (0, 2) and (0, 3) sit exactly on the two bounds
    got = _rc(mm.mark_mask(15, 15, mm.ring(8, 8, 2.5, RED)))
    assert (8, 10) in got and (8, 11) in got and (8, 9) not in got and (8, 12) not in got


def test_radius_zero_is_the_zero_length_segment_of_the_same_width():
    for lw in (1, 2, 5, 64):
        for x, y in ((9, 7), (9.5, 7.25), (0.4, 0.6)):
            assert np.array_equal(mm.mark_mask(40, 44, mm.ring(x, y, 0, RED, lw)), mm.mark_mask(40, 44, mm.segment(x, y, x, y, RED, lw)))
    assert _rc(mm.mark_mask(9, 9, mm.ring(5, 4, 0, RED, 2))) == {(4, 5), (3, 5), (5, 5), (4, 4), (4, 6)}
    # a radius below the half width clamps the inner bound to 0: a disc
    assert _rc(mm.mark_mask(9, 9, mm.ring(5, 4, 0.25, RED, 1))) == {(4, 5)}


def test_end_point_on_the_half_pixel_tie_paints_both_neighbours():
    # the end point is half a pixel from the centres of columns 6 and 7: the cap's comparison is closed
    assert _rc(mm.mark_mask(8, 12, mm.segment(2, 3, 6.5, 3, RED))) == {(3, c) for c in range(2, 8)}
    # a segment exactly between rows 3 and 4 is half a pixel from both
    assert {r for r, _ in _rc(mm.mark_mask(8, 12, mm.segment(2, 3.5, 6, 3.5, RED)))} == {3, 4}
    assert _rc(mm.mark_mask(8, 12, mm.segment(2, 3.5 - 1 / 16, 6, 3.5 - 1 / 16, RED))) == {(3, c) for c in range(2, 7)}


def test_segment_rule_is_the_annotation_contracts_edge_rule():
    rng = np.random.default_rng(4)
    for lw in (1, 2, 7):
        for _ in range(6):
            x0, y0, x1, y1 = rng.uniform(-5, 45, 4)
            want = am.edge_mask(40, 40, (am.quant(x0), am.quant(y0)), (am.quant(x1), am.quant(y1)), lw)
            assert np.array_equal(mm.mark_mask(40, 40, mm.segment(x0, y0, x1, y1, RED, lw)), want)


def test_grid_evaluation_equals_the_pixel_loop():
    """mark_mask's int64 grids (small operands) against its loop over Python ints, on random marks in and around a canvas,
    up to the largest operands the grids take."""
    rng = np.random.default_rng(6)
    for H, W in ((40, 44), (9, 1024)):
        for k in range(40):
            lw = int(rng.choice([1, 2, 7, 64]))
            if k % 2:
                m = mm.segment(*rng.choice([-1024, -30.5, 0.5, 7.25, W, 1024], 2), *rng.uniform(-1024, 1024, 2), RED, lw)
            else:
                m = mm.ring(rng.uniform(-60, W + 60), rng.uniform(-60, H + 60), float(rng.choice([0, 0.25, 3, 40.5, 500, 4096])), RED, lw)
            assert np.array_equal(mm.mark_mask(H, W, m), mm.mark_mask(H, W, m, python_ints=True)), m


def test_validity_order_and_count():
    base = np.full((20, 30, 3), 9, np.uint8)
    marks = [mm.segment(2, 2, 25, 15, RED, 3), mm.ring(12, 9, 5, GREEN, 2), mm.segment(2, 15, 25, 2, (0, 0, 255), 3)]
    out, n = mm.draw_marks(base, marks)
    assert n == 3 and (base == 9).all()
    top = mm.mark_mask(20, 30, marks[2])
    assert (out[top] == (0, 0, 255)).all()  # the highest index wins
    mid = mm.mark_mask(20, 30, marks[1]) & ~top
    assert mid.any() and (out[mid] == GREEN).all()
    rest = ~(top | mm.mark_mask(20, 30, marks[1]) | mm.mark_mask(20, 30, marks[0]))
    assert (out[rest] == 9).all()
    bad = [mm.segment(np.nan, 2, 5, 5, RED), mm.segment(2, 2, np.inf, 5, RED), mm.segment(2, 2, 5, 2.0 ** 20 + 1, RED),
           mm.ring(5, 5, -1, RED), mm.ring(5, 5, 4097, RED), mm.ring(5, -np.inf, 3, RED), mm.ring(5, 5, np.nan, RED)]
    out2, n2 = mm.draw_marks(base, bad + [mm.segment(500, 500, 600, 600, RED)])
    assert n2 == 1 and np.array_equal(out2, base)  # the valid one is wholly outside: it counts and paints nothing
    ok = dict(mm.ring(5, 5, 3, RED), y1=np.nan)  # y1 of a ring is not looked at
    assert mm.draw_marks(base, [ok])[1] == 1 and mm.draw_marks(base, [mm.ring(5, 5, 4096, RED), mm.segment(2.0 ** 20, 1, 1, 1, RED)])[1] == 2
    for wrong in (dict(marks[0], kind=2), dict(marks[0], kind=-1), dict(marks[0], line_width=0), dict(marks[1], line_width=65)):
        with pytest.raises(ValueError):
            mm.draw_marks(base, [marks[0], wrong])


def test_montage_padding_is_zero():
    a, b = np.full((4, 5, 3), 7, np.uint8), np.full((7, 3, 3), 200, np.uint8)
    for first, second in ((a, b), (b, a)):
        m = mm.montage_pair(first, second)
        h1, w1 = first.shape[:2]
        h2, w2 = second.shape[:2]
        assert m.shape == (7, 8, 3)
        assert np.array_equal(m[:h1, :w1], first) and np.array_equal(m[:h2, w1:], second)
        assert (m[h1:, :w1] == 0).all() and (m[h2:, w1:] == 0).all()
    assert np.array_equal(mm.montage_pair(a[:, :, 0], a[:, :, :1]), mm.montage_pair(a, a))  # a single channel is replicated


def test_match_plot_marks_order_and_dropped_rows():
    p1 = [[3, 4], [5, np.nan], [7, 8]]
    p2 = [[1, 2], [2, 2], [4, 6]]
    marks = mm.match_plot_marks(p1, p2, 50)
    assert len(marks) == 2 * 4
    assert [m["kind"] for m in marks] == [0, 0, 1, 1, 0, 0, 0, 0]
    assert [m["rgb"] for m in marks] == [(255, 255, 0)] * 2 + [(255, 0, 0)] * 2 + [(0, 255, 0)] * 4
    assert (marks[0]["x0"], marks[0]["y0"], marks[0]["x1"], marks[0]["y1"]) == (3, 4, 51, 2)
    assert (marks[3]["x0"], marks[3]["y0"], marks[3]["x1"]) == (7, 8, 3)
    assert [(m["x0"], m["y0"], m["x1"], m["y1"]) for m in marks[4:6]] == [(48, 2, 54, 2), (51, -1, 51, 5)]
    styled = mm.match_plot_marks(p1, p2, 50, markerRadius=5, lineWidth=2, colors=((1, 2, 3), (4, 5, 6), (7, 8, 9)))
    assert styled[2]["x1"] == 5 and styled[0]["line_width"] == 2 and [styled[k]["rgb"] for k in (0, 2, 4)] == [(7, 8, 9), (1, 2, 3), (4, 5, 6)]


def test_keypoint_marks():
    marks = mm.keypoint_marks([[10, 10], [20, 5]], scales=[4, 2.5], angles_deg=[0, 90])
    assert [m["kind"] for m in marks] == [1, 1, 0, 0] and marks[1]["x1"] == 2.5
    assert (marks[2]["x1"], marks[2]["y1"]) == (14, 10)
    assert abs(marks[3]["x1"] - 20) < 1e-12 and marks[3]["y1"] == 2.5  # 90 degrees points up the screen
    assert [m["x1"] for m in mm.keypoint_marks([[1, 1]], markerRadius=6)] == [6]
