"""CPU tests of the mark entries: aps_draw_marks and aps_montage_pair are declared, bound and exported; aps_mark's layout; every
refusal happens before any device work and writes nothing; without a device a valid call is APS_E_DEVICE; the host-only helpers
of the match plots."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods(aps):
    return {k: import_module(aps.__name__ + "." + k) for k in ("imageProcessing", "imageMatching", "featureMatching")}


def test_symbols_are_declared_bound_and_exported(aps):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aps.h")).read(), flags=re.S)
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    for name, nargs in (("aps_draw_marks", 7), ("aps_montage_pair", 7)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(getattr(capi.lib, name).argtypes) == nargs
    assert re.search(r"#define\s+APS_MARK_SEGMENT\s+0\b", header) and re.search(r"#define\s+APS_MARK_RING\s+1\b", header)
    assert (capi.APS_MARK_SEGMENT, capi.APS_MARK_RING) == (0, 1)


def test_aps_mark_layout(aps):
    capi = aps._capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aps.h")).read(), flags=re.S)
    body = re.search(r"typedef struct aps_mark \{(.*?)\} aps_mark;", header, re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "double x0, y0, x1, y1; int32_t kind, line_width; uint8_t rgb[3], reserved;"
    st = capi.aps_mark
    assert C.sizeof(st) == 48
    assert [n for n, _ in st._fields_] == ["x0", "y0", "x1", "y1", "kind", "line_width", "rgb", "reserved"]
    assert [getattr(st, n).offset for n, _ in st._fields_] == [0, 8, 16, 24, 32, 36, 40, 43]
    dt = capi.MARK_DTYPE
    assert dt.itemsize == 48 and list(dt.names) == [n for n, _ in st._fields_]
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 24, 32, 36, 40, 43]
    assert dt["rgb"].shape == (3,) and dt["kind"] == np.int32 and dt["x1"] == np.float64


def _marks(aps, mods, n=2):
    ip = mods["imageProcessing"]
    return np.concatenate([ip.mark_segments([[1, 1]] * (n - 1), [[3, 2]] * (n - 1), (9, 8, 7), 2), ip.mark_rings([[2, 2]], 1.5, (1, 2, 3))])


def _call(aps, src, h, w, marks, n, dst, count=True):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    cnt = C.c_int64(-7)
    st = aps.lib.aps_draw_marks(p(src), h, w, p(marks), n, p(dst), C.byref(cnt) if count else None)
    return st, cnt.value


def test_mark_constructors(aps, mods):
    ip = mods["imageProcessing"]
    m = ip.mark_segments([[1, 2], [3, 4]], [[5, 6], [7, 8]], [[1, 2, 3], [4, 5, 6]], [1, 64])
    assert m.dtype == aps._capi.MARK_DTYPE and m.shape == (2,)
    rec = lambda v: tuple(v[f].tolist() for f in v.dtype.names)  # noqa: E731
    assert rec(m[1]) == (3.0, 4.0, 7.0, 8.0, 0, 64, [4, 5, 6], 0)
    r = ip.mark_rings([[1, 2], [3, 4]], [2.5, 0], (7, 8, 9), 3)
    assert rec(r[0]) == (1.0, 2.0, 2.5, 0.0, 1, 3, [7, 8, 9], 0) and r[1]["x1"] == 0
    assert len(ip.mark_segments(np.zeros((0, 2)), np.zeros((0, 2)), (1, 1, 1))) == 0
    assert np.concatenate([m, r]).dtype == aps._capi.MARK_DTYPE
    with pytest.raises(ValueError):
        ip.mark_segments([[1, 2]], [[1, 2], [3, 4]], (0, 0, 0))
    with pytest.raises(ValueError):
        ip.draw_marks(np.zeros((4, 5, 3), np.uint8), np.zeros(2, np.float64))
    with pytest.raises(ValueError):
        ip.draw_marks(np.zeros((4, 5, 3), np.float32), m)


def test_refused_arguments_write_nothing(aps, mods):
    E = aps._capi.APS_E_ARG
    img, out = np.zeros((4, 5, 3), np.uint8), np.full((4, 5, 3), 9, np.uint8)
    marks = _marks(aps, mods)
    good = dict(src=img, h=4, w=5, marks=marks, n=2, dst=out)

    def bad_mark(field, value, at=1):
        m = marks.copy()
        m[field][at] = value
        return dict(marks=m)

    for bad in (dict(src=None), dict(dst=None), dict(marks=None), dict(h=0), dict(w=0), dict(h=-3), dict(w=2 ** 31), dict(n=-1),
                bad_mark("kind", 2), bad_mark("kind", -1), bad_mark("kind", 7, at=0), bad_mark("line_width", 0),
                bad_mark("line_width", 65), bad_mark("line_width", -2, at=0)):
        st, cnt = _call(aps, **dict(good, **bad))
        assert st == E, (bad, st)
        assert cnt == -7 and aps.lib.aps_last_error()
    # source and destination that overlap without being the same buffer
    buf = np.zeros(4 * 5 * 3 + 8, np.uint8)
    assert aps.lib.aps_draw_marks(buf.ctypes.data, 4, 5, marks.ctypes.data, 2, buf.ctypes.data + 8, None) == E
    assert aps.lib.aps_draw_marks(buf.ctypes.data + 8, 4, 5, marks.ctypes.data, 2, buf.ctypes.data, None) == E
    assert (out == 9).all() and (img == 0).all() and (buf == 0).all()  # nothing was written by a refused call


def test_tile_lists_beyond_int32_are_refused_before_any_device_work(aps, mods):
    """131072 width-1 segments along a 1 x 2^20 canvas touch 16384 tiles each: 2^31 list entries.  Counted per (mark, tile row)
    in O(1), so the refusal costs no memory and no time."""
    ip = mods["imageProcessing"]
    W, n = 2 ** 20, 2 ** 17
    img, out = np.zeros((1, W, 3), np.uint8), np.zeros((1, W, 3), np.uint8)
    marks = ip.mark_segments(np.tile([[1.0, 1.0]], (n, 1)), np.tile([[float(W), 1.0]], (n, 1)), (255, 0, 0))
    st, cnt = _call(aps, img, 1, W, marks, n, out)
    assert st == aps._capi.APS_E_ARG and cnt == -7 and b"32-bit" in aps.lib.aps_last_error()
    assert not out.any() and not img.any()


def test_valid_call_needs_a_device(aps, mods):
    """No CPU fallback: without a device a valid call is APS_E_DEVICE and writes nothing; with one it succeeds."""
    img, out = np.zeros((4, 5, 3), np.uint8), np.full((4, 5, 3), 9, np.uint8)
    st, cnt = _call(aps, img, 4, 5, _marks(aps, mods), 2, out)
    st0, _ = _call(aps, img, 4, 5, None, 0, out.copy())  # n = 0 with a NULL table is a valid call
    if aps.lib.aps_device_count() > 0:
        assert st == 0 and cnt == 2 and st0 == 0
    else:
        assert st == st0 == aps._capi.APS_E_DEVICE and cnt == -7 and (out == 9).all()


def test_montage_pair_refusals_and_device(aps):
    lib, E = aps.lib, aps._capi.APS_E_ARG
    a, b, out = np.full((4, 5, 3), 1, np.uint8), np.full((7, 3, 3), 2, np.uint8), np.full((7, 8, 3), 9, np.uint8)
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    for args in ((None, 4, 5, b, 7, 3, out), (a, 4, 5, None, 7, 3, out), (a, 4, 5, b, 7, 3, None), (a, 0, 5, b, 7, 3, out),
                 (a, 4, 0, b, 7, 3, out), (a, 4, 5, b, -1, 3, out), (a, 4, 5, b, 7, 0, out), (a, 4, 2 ** 31 - 2, b, 7, 3, out)):
        assert lib.aps_montage_pair(p(args[0]), args[1], args[2], p(args[3]), args[4], args[5], p(args[6])) == E, args[1:6]
    buf = np.full(7 * 8 * 3 + 62, 5, np.uint8)  # a destination that overlaps image 1, then image 2
    assert lib.aps_montage_pair(buf.ctypes.data + 100, 4, 5, p(b), 7, 3, buf.ctypes.data) == E
    assert lib.aps_montage_pair(p(a), 4, 5, buf.ctypes.data + 7 * 8 * 3 - 1, 7, 3, buf.ctypes.data) == E
    assert (out == 9).all() and (buf == 5).all()
    st = lib.aps_montage_pair(p(a), 4, 5, p(b), 7, 3, p(out))
    if lib.aps_device_count() > 0:
        assert st == 0 and (out[:4, :5] == 1).all() and (out[:, 5:] == 2).all() and (out[4:, :5] == 0).all()
    else:
        assert st == aps._capi.APS_E_DEVICE and (out == 9).all()


def test_match_plot_bytes(mods):
    im = mods["imageMatching"]
    # 40 x 50 beside 70 x 30: three pictures of 70 x 80 x 3 bytes
    assert im.match_plot_bytes([(40, 50, 3), (70, 30, 3)], [(0, 1)]) == 3 * 70 * 80 * 3 == 50400
    # three 4K views, two pairs, and one pair of unequal views
    sizes = [(2160, 3840), (2160, 3840), (2160, 3840), (100, 200)]
    assert im.match_plot_bytes(sizes, [(0, 1), (1, 2), (2, 3)]) == 2 * 3 * 2160 * 7680 * 3 + 3 * 2160 * 4040 * 3 == 377136000
    assert im.match_plot_bytes(sizes, []) == 0


def test_show_matched_features_serves_the_montage_only(mods):
    im = mods["imageMatching"]
    a = np.zeros((4, 5, 3), np.uint8)
    for method in ("blend", "falsecolor", "Blend"):
        with pytest.raises(ValueError, match="montage"):
            im.showMatchedFeatures(a, a, np.ones((2, 2)), np.ones((2, 2)), method=method)
    with pytest.raises(ValueError):
        im.match_plot_marks(np.ones((2, 2)), np.ones((3, 2)), 5)


def test_match_plot_and_keypoint_marks_on_the_host(aps, mods):
    """The wrappers' mark lists (host only) against the mirror's."""
    import marks_mirror as mm

    im, fm = mods["imageMatching"], mods["featureMatching"]

    def same(got, want):
        assert got.dtype == aps._capi.MARK_DTYPE and len(got) == len(want)
        for g, w in zip(got, want):
            assert all(g[f] == w[f] or (np.isnan(g[f]) and np.isnan(w[f])) for f in ("x0", "y0", "x1", "y1", "kind", "line_width"))
            assert tuple(g["rgb"]) == tuple(w["rgb"])

    rng = np.random.default_rng(2)
    p1, p2 = rng.uniform(1, 50, (9, 2)), rng.uniform(1, 30, (9, 2))
    p1[4, 1] = np.nan
    p2[7, 0] = np.inf
    same(im.match_plot_marks(p1, p2, 50), mm.match_plot_marks(p1, p2, 50))
    style = dict(markerRadius=4.5, lineWidth=3, colors=((1, 2, 3), (4, 5, 6), (7, 8, 9)))
    same(im.match_plot_marks(p1, p2, 31, **style), mm.match_plot_marks(p1, p2, 31, **style))
    pts, sc, ang = rng.uniform(1, 60, (11, 2)), rng.uniform(0.5, 9, 11), rng.uniform(-400, 400, 11)
    same(fm.keypoint_marks(pts), mm.keypoint_marks(pts))
    same(fm.keypoint_marks(pts, sc, ang, (5, 6, 7), 3, 2), mm.keypoint_marks(pts, sc, ang, (5, 6, 7), 3, 2))
    same(fm.keypoint_marks(pts, None, ang, markerRadius=5), mm.keypoint_marks(pts, None, ang, markerRadius=5))
