"""Device tests of the mark entries: aps_draw_marks equals tests/marks_mirror.py byte for byte, with the mirror's count, on small
canvases (one pixel, one ragged tile, one full tile, ragged tiles on both axes, several tiles), and aps_montage_pair equals the
mirror's montage."""
import ctypes as C

import numpy as np
import pytest

import marks_mirror as mm

pytestmark = pytest.mark.gpu

CANVASES = [(1, 1), (37, 53), (64, 64), (65, 130), (130, 200)]
PLACES = ["host", "device", "inplace_host", "inplace_device", "host_to_device", "device_to_host"]


def _src(H, W, seed=0):
    return np.random.default_rng(seed + 1000 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _records(gpu, marks):
    """The mirror's marks as an aps_mark table (NaN in y1 of a ring where the mirror has one: it is not looked at)."""
    a = np.zeros(len(marks), gpu._capi.MARK_DTYPE)
    for k, m in enumerate(marks):
        for f in ("x0", "y0", "x1", "y1", "kind", "line_width"):
            a[f][k] = m[f]
        a["rgb"][k] = m["rgb"]
    return a


def _device(gpu, src, marks, where="host"):
    """aps_draw_marks through the raw entry.  Returns (result, count, source bytes after the call)."""
    import torch

    capi = gpu._capi
    H, W = src.shape[:2]
    s_dev = where in ("device", "inplace_device", "device_to_host")
    d_dev = where in ("device", "inplace_device", "host_to_device")
    s = torch.from_numpy(src.copy()).cuda() if s_dev else src.copy()
    if where.startswith("inplace"):
        d = s
    else:
        d = torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda") if d_dev else np.full((H, W, 3), 77, np.uint8)
    torch.cuda.synchronize()
    table = _records(gpu, marks)
    cnt = C.c_int64(-1)
    capi.check(capi.lib.aps_draw_marks(capi.ptr(s), H, W, capi.ptr(table) if len(table) else None, len(table), capi.ptr(d), C.byref(cnt)))
    capi.check(capi.lib.aps_synchronize())
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a  # noqa: E731
    return host(d), cnt.value, host(s)


def _check(gpu, src, marks, where="host"):
    want, n_want = mm.draw_marks(src, marks)
    got, n_got, src_after = _device(gpu, src, marks, where)
    assert n_got == n_want
    bad = np.argwhere((got != want).any(2))
    assert len(bad) == 0, f"{len(bad)} pixels differ from the mirror, first at (row, col) = {tuple(bad[0] + 1)}"
    if not where.startswith("inplace"):
        assert np.array_equal(src_after, src), "the source was written"
    return got


def _colour(k):
    return ((37 * k + 11) % 256, (91 * k + 200) % 256, (53 * k + 5) % 256)


def _segment_cases(H, W):
    cases = {f"width_{lw}": (0.15 * W + 1.3, 0.2 * H + 0.6, 0.85 * W + 0.2, 0.7 * H + 1.1, lw) for lw in (1, 2, 7, 64)}
    cases.update({
        "dot": (0.5 * W + 0.3, 0.5 * H + 0.7, 0.5 * W + 0.3, 0.5 * H + 0.7, 5),
        "outside": (W + 40, -30, W + 90, H + 50, 3),
        "enters_from_negative": (-0.6 * W - 9.5, -0.4 * H - 3.25, 0.6 * W, 0.7 * H, 2),
        "across_a_tile_corner": (60.2, 69.1, 69.4, 59.8, 1),
        "along_a_tile_border": (64.5, -3, 64.5, H + 3, 1),
        "half_pixel_ties": (2.5, 3.5, 0.5 * W + 0.5, 3.5, 1),
        "half_pixel_ties_wide": (1.5, 0.5 * H + 0.5, W - 0.5, 0.5 * H + 0.5, 2),
        # v = m / 16 + 1 / 32: 16 v + 0.5 is an integer exactly, the quantiser's tie
        "quantiser_ties": (2 + 1 / 32, 1 + 3 / 32, W - 5 / 32, H - 11 / 32, 1),
        "steep": (0.4 * W, -5, 0.45 * W + 1, H + 5, 1),
        "largest_coordinates": (-(2.0 ** 20), -(2.0 ** 20), 2.0 ** 20, 2.0 ** 20, 3),
    })
    return cases


SEGMENT_NAMES = sorted(_segment_cases(8, 8))


@pytest.mark.parametrize("H,W", CANVASES)
@pytest.mark.parametrize("name", SEGMENT_NAMES)
def test_one_segment_equals_mirror(gpu, H, W, name):
    x0, y0, x1, y1, lw = _segment_cases(H, W)[name]
    src = _src(H, W)
    got = _check(gpu, src, [mm.segment(x0, y0, x1, y1, (250, 10, 20), lw)])
    if name == "outside":
        assert np.array_equal(got, src)
    _check(gpu, src, [mm.segment(x1, y1, x0, y0, (250, 10, 20), lw)])  # the other direction


def _ring_cases(H, W):
    cases = {f"radius_{r}": (0.5 * W + 0.4, 0.5 * H + 0.2, r, 1) for r in (0, 0.25, 3, 40.5)}
    cases.update({
        "radius_3_wide": (0.4 * W, 0.6 * H, 3, 7),
        "radius_0_widest": (0.5 * W, 0.5 * H, 0, 64),
        "radius_4096_arc": (0.5 * W + 4096, 0.5 * H, 4096, 2),       # its leftmost arc runs through the canvas
        "radius_4096_arc_below": (0.3 * W, 0.5 * H - 4096, 4096, 1),
        "centred_outside": (-6.5, H + 4.25, 12, 2),
        "centred_on_a_tile_corner": (64.5, 64.5, 20, 3),
        "around_the_canvas": (0.5 * W, 0.5 * H, 0.75 * (H + W), 5),  # the canvas lies inside the hole
        "tie_radius": (0.5 * W + 0.5, 0.5 * H, 2.5, 1),
    })
    return cases


RING_NAMES = sorted(_ring_cases(8, 8))


@pytest.mark.parametrize("H,W", CANVASES)
@pytest.mark.parametrize("name", RING_NAMES)
def test_one_ring_equals_mirror(gpu, H, W, name):
    x, y, r, lw = _ring_cases(H, W)[name]
    _check(gpu, _src(H, W), [dict(mm.ring(x, y, r, (10, 240, 30), lw), y1=float("nan"))])  # y1 is not looked at


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 2.0 ** 20 + 1, -(2.0 ** 20) - 1])
def test_invalid_marks_are_skipped_and_not_counted(gpu, bad):
    H, W = 65, 130
    src = _src(H, W)
    good = [mm.segment(5, 5, 100, 50, _colour(0), 2), mm.ring(60, 30, 12, _colour(1), 2), mm.segment(120, 3, 8, 60, _colour(2), 1)]
    invalid = [mm.segment(bad, 5, 40, 8, _colour(3)), mm.segment(5, bad, 40, 8, _colour(4)), mm.segment(5, 5, bad, 8, _colour(5)),
               mm.segment(5, 5, 40, bad, _colour(6)), mm.ring(bad, 20, 4, _colour(7)), mm.ring(20, bad, 4, _colour(8)),
               mm.ring(20, 20, -1, _colour(9)), mm.ring(20, 20, 4097, _colour(10)), mm.ring(20, 20, np.nan, _colour(11)),
               mm.ring(20, 20, np.inf, _colour(12))]
    mixed = [good[0]] + invalid[:5] + [good[1]] + invalid[5:] + [good[2]]
    got = _check(gpu, src, mixed)
    only, n_only, _ = _device(gpu, src, good)
    assert n_only == 3 and np.array_equal(got, only)
    # the largest valid values are still drawn (and clipped)
    edge = np.sign(bad) * 2.0 ** 20 if np.isfinite(bad) else 7.0
    _check(gpu, src, [mm.segment(edge, 5, 40, 8, _colour(3), 2), mm.ring(60, 30, 4096, _colour(4)), mm.ring(edge, 20, 4, _colour(5))])


def test_three_overlapping_marks_highest_index_wins(gpu):
    H, W = 130, 200
    marks = [mm.segment(10, 10, 190, 120, (255, 0, 0), 7), mm.ring(100, 65, 40, (0, 255, 0), 7), mm.segment(10, 120, 190, 10, (0, 0, 255), 7)]
    got = _check(gpu, _src(H, W), marks)
    assert tuple(got[64, 99]) == (0, 0, 255)  # the crossing of the two segments carries the last colour
    where_ring_meets_first = mm.mark_mask(H, W, marks[0]) & mm.mark_mask(H, W, marks[1]) & ~mm.mark_mask(H, W, marks[2])
    assert where_ring_meets_first.any() and (got[where_ring_meets_first] == (0, 255, 0)).all()
    _check(gpu, _src(H, W), marks[::-1])


def test_600_segments_through_one_tile(gpu):
    """A tile's list far longer than the workgroup that walks it."""
    rng = np.random.default_rng(8)
    marks = [mm.segment(*rng.uniform(0.5, 64.5, 4), _colour(k), 1 + k % 2) for k in range(600)]
    _check(gpu, _src(64, 64), marks)
    _check(gpu, _src(65, 130), marks, where="inplace_device")  # the same list in the first of six ragged tiles


def test_a_seam_tile_holds_every_line(gpu):
    """Lines from the left half to the right half of a wide canvas, as in a montage: all of them cross the middle column."""
    rng = np.random.default_rng(9)
    H, W = 40, 400
    marks = [mm.segment(rng.uniform(1, 200), rng.uniform(1, H), rng.uniform(201, W), rng.uniform(1, H), _colour(k)) for k in range(150)]
    _check(gpu, _src(H, W), marks, where="device")


def test_no_marks_is_a_copy(gpu):
    src = _src(65, 130)
    for where in ("host", "device", "host_to_device"):
        got, n, _ = _device(gpu, src, [], where)
        assert n == 0 and np.array_equal(got, src)
    got, n, _ = _device(gpu, src, [mm.segment(500, 500, 600, 600, (1, 2, 3))])  # valid, wholly outside: counted, nothing painted
    assert n == 1 and np.array_equal(got, src)


@pytest.mark.parametrize("where", PLACES)
def test_pointer_placements(gpu, where):
    H, W = 130, 200
    marks = [mm.segment(12.3, 9.1, 180.6, 118.4, _colour(0), 2), mm.ring(64.5, 64.5, 30.25, _colour(1), 5), mm.ring(150, 20, 0, _colour(2), 9),
             mm.segment(-30, 64.5, 230, 70, _colour(3), 1), mm.segment(np.nan, 1, 2, 2, _colour(4))]
    _check(gpu, _src(H, W), marks, where=where)


def test_draw_marks_wrapper(gpu):
    """imageProcessing.draw_marks: a replicated channel, a non-contiguous view, arrays and tensors; the input is never written."""
    import torch
    from importlib import import_module

    ip = import_module(gpu.__name__ + ".imageProcessing")
    marks = [mm.segment(3, 4, 50, 30, _colour(0), 2), mm.ring(20, 18, 9, _colour(1)), mm.ring(5, 5, 5000, _colour(2))]
    table = np.concatenate([ip.mark_segments([[3, 4]], [[50, 30]], _colour(0), 2), ip.mark_rings([[20, 18], [5, 5]], [9, 5000], [_colour(1), _colour(2)])])
    src = _src(37, 53)
    want, n_want = mm.draw_marks(src, marks)
    assert n_want == 2
    for image in (src, torch.from_numpy(src), torch.from_numpy(src).cuda()):
        keep = image.clone() if hasattr(image, "clone") else image.copy()
        got, n = ip.draw_marks(image, table)
        assert n == 2 and type(got) is type(image) and getattr(got, "is_cuda", False) == getattr(image, "is_cuda", False)
        assert np.array_equal(got.cpu().numpy() if hasattr(got, "cpu") else got, want)
        assert (image == keep).all()
    gray = src[:, :, 1]
    want_gray, _ = mm.draw_marks(np.repeat(gray[:, :, None], 3, axis=2), marks)
    for image in (gray, gray[:, :, None], torch.from_numpy(np.ascontiguousarray(gray)).cuda()):
        got, _ = ip.draw_marks(image, table)
        assert np.array_equal(got.cpu().numpy() if hasattr(got, "cpu") else got, want_gray)
    big = _src(60, 80, seed=3)
    view = big[5:42, 10:63]  # non-contiguous
    got, _ = ip.draw_marks(view, table)
    assert np.array_equal(got, mm.draw_marks(view, marks)[0]) and np.array_equal(big, _src(60, 80, seed=3))
    got, _ = ip.draw_marks(torch.from_numpy(big).cuda()[5:42, 10:63], table)
    assert np.array_equal(got.cpu().numpy(), mm.draw_marks(view, marks)[0])


MONTAGES = [((40, 50), (70, 30)), ((70, 30), (40, 50)), ((33, 21), (33, 21)), ((1, 1), (1, 1)), ((1, 70), (64, 1))]


@pytest.mark.parametrize("s1,s2", MONTAGES)
@pytest.mark.parametrize("where", ["hhh", "ddd", "hdd", "dhh", "ddh", "hhd"])
def test_montage_pair_equals_mirror(gpu, s1, s2, where):
    """where: host / device for image 1, image 2, the destination."""
    import torch

    capi = gpu._capi
    a, b = _src(*s1, seed=1), _src(*s2, seed=2)
    want = mm.montage_pair(a, b)
    put = lambda x, w: torch.from_numpy(x.copy()).cuda() if w == "d" else x.copy()  # noqa: E731
    i1, i2 = put(a, where[0]), put(b, where[1])
    dst = torch.full(want.shape, 77, dtype=torch.uint8, device="cuda") if where[2] == "d" else np.full(want.shape, 77, np.uint8)
    torch.cuda.synchronize()
    capi.check(capi.lib.aps_montage_pair(capi.ptr(i1), s1[0], s1[1], capi.ptr(i2), s2[0], s2[1], capi.ptr(dst)))
    capi.check(capi.lib.aps_synchronize())
    host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else x  # noqa: E731
    assert np.array_equal(host(dst), want)
    assert np.array_equal(host(i1), a) and np.array_equal(host(i2), b)


def test_montage_pair_wrapper(gpu):
    import torch
    from importlib import import_module

    ip = import_module(gpu.__name__ + ".imageProcessing")
    a, b = _src(40, 50, seed=1), _src(70, 30, seed=2)
    want = mm.montage_pair(a, b)
    got = ip.montage_pair(a, b)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    for x, y in ((torch.from_numpy(a).cuda(), b), (a, torch.from_numpy(b).cuda()), (torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())):
        got = ip.montage_pair(x, y)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    gray = ip.montage_pair(a[:, :, 0], torch.from_numpy(b).cuda()[:, ::2])  # one channel, and a non-contiguous view
    assert np.array_equal(gray.cpu().numpy(), mm.montage_pair(a[:, :, 0], b[:, ::2]))
