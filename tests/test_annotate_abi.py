"""CPU tests of the annotated panorama: the C-ABI entry's declaration and argument checks, the NumPy mirror of the annotation
contract against closed forms, the palette, warped_boxes against hand-computed values, displayPanorama's checks."""
import ctypes as C
import math
import os
import re
from importlib import import_module

import numpy as np
import pytest

import annotate_mirror as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rp(aps):
    return import_module(aps.__name__ + ".renderPanorama")


# ---- the entry ---------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_bound(aps):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aps.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+aps_annotate_panorama\s*\(", header)
    capi = aps._capi
    assert "aps_annotate_panorama" in capi.EXPORTED_SYMBOLS
    assert hasattr(C.CDLL(capi.LIB_PATH), "aps_annotate_panorama")
    assert len(capi.lib.aps_annotate_panorama.argtypes) == 10


def _call(aps, src, h, w, polys, anchors, colors, n, lw, dst, drawn=True):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    cnt = C.c_int(-7)
    st = aps.lib.aps_annotate_panorama(p(src), h, w, p(polys), p(anchors), p(colors), n, lw, p(dst), C.byref(cnt) if drawn else None)
    return st, cnt.value


def test_refused_arguments(aps):
    E = aps._capi.APS_E_ARG
    img, out = np.zeros((4, 5, 3), np.uint8), np.full((4, 5, 3), 9, np.uint8)
    polys, anchors, colors = np.ones((2, 4, 2)), np.ones((2, 2)), np.zeros((2, 3), np.uint8)
    good = dict(src=img, h=4, w=5, polys=polys, anchors=anchors, colors=colors, n=2, lw=2, dst=out)
    for bad in (dict(src=None), dict(dst=None), dict(polys=None), dict(anchors=None), dict(colors=None), dict(drawn=False),
                dict(h=0), dict(w=0), dict(h=-3), dict(n=-1), dict(lw=0), dict(lw=-2), dict(lw=65)):
        st, _ = _call(aps, **dict(good, **bad))
        assert st == E, (bad, st)
        assert aps.lib.aps_last_error()
    # source and destination that overlap without being the same buffer
    buf = np.zeros(4 * 5 * 3 + 8, np.uint8)
    st = aps.lib.aps_annotate_panorama(buf.ctypes.data, 4, 5, polys.ctypes.data, anchors.ctypes.data, colors.ctypes.data, 2, 2,
                                       buf.ctypes.data + 8, C.byref(C.c_int(0)))
    assert st == E
    assert (out == 9).all() and (img == 0).all()  # nothing was written by a refused call


def test_valid_call_needs_a_device(aps):
    """No CPU fallback: without a device a valid call is APS_E_DEVICE and writes nothing; with one it succeeds."""
    img, out = np.zeros((4, 5, 3), np.uint8), np.full((4, 5, 3), 9, np.uint8)
    st, cnt = _call(aps, img, 4, 5, np.ones((1, 4, 2)), np.ones((1, 2)), np.zeros((1, 3), np.uint8), 1, 2, out)
    if aps.lib.aps_device_count() > 0:
        assert st == 0 and cnt == 1
    else:
        assert st == aps._capi.APS_E_DEVICE and cnt == -7 and (out == 9).all()


# ---- the mirror against closed forms --------------------------------------------------------------------------------------------
def _rc(mask):
    return {(int(r) + 1, int(c) + 1) for r, c in zip(*np.nonzero(mask))}


def test_quantiser():
    assert am.quant(1.0) == 16 and am.quant(-1.0) == -16
    assert am.quant(0.5 / 16) == 1 and am.quant(-0.5 / 16) == 0 and am.quant(1.5 / 16) == 2  # ties go up (floor(v + 0.5))
    assert am.quant(3 + 7 / 16) == 55 and am.quant(2.0 ** 20) == 2 ** 24
    assert am.valid_polygon(np.full((4, 2), 2.0 ** 20)) and not am.valid_polygon(np.full((4, 2), 2.0 ** 20 + 1))
    for bad in (np.nan, np.inf, -np.inf):
        p = np.ones((4, 2))
        p[2, 1] = bad
        assert not am.valid_polygon(p)


def test_horizontal_edge_width_two_paints_three_rows_and_round_caps():
    m = am.edge_mask(20, 30, (16 * 5, 16 * 10), (16 * 20, 16 * 10), 2)
    want = {(r, c) for r in (9, 10, 11) for c in range(5, 21)} | {(10, 4), (10, 21)}
    assert _rc(m) == want
    assert _rc(am.edge_mask(20, 30, (16 * 20, 16 * 10), (16 * 5, 16 * 10), 2)) == want  # direction does not matter


def test_zero_length_edge_is_a_plus():
    m = am.edge_mask(9, 9, (16 * 5, 16 * 4), (16 * 5, 16 * 4), 2)
    assert _rc(m) == {(4, 5), (3, 5), (5, 5), (4, 4), (4, 6)}
    assert _rc(am.edge_mask(9, 9, (16 * 5, 16 * 4), (16 * 5, 16 * 4), 1)) == {(4, 5)}


def test_width_one_edge_at_a_half_pixel_offset_paints_one_row():
    """End points at x = 5.5 and 20.5 on the integer row 10, radius half a pixel: row 10 alone, from the pixel whose centre is
    exactly half a pixel before the start (the cap, distance == radius: the comparison is closed) to the one half a pixel after."""
    m = am.edge_mask(20, 30, (am.quant(5.5), 160), (am.quant(20.5), 160), 1)
    assert _rc(m) == {(10, c) for c in range(5, 22)}
    # the same closed comparison across the row direction: an edge exactly between rows 10 and 11 is half a pixel from both
    # and paints both; a sixteenth nearer to row 10 it paints row 10 only
    tie = am.edge_mask(20, 30, (80, am.quant(10.5)), (320, am.quant(10.5)), 1)
    assert {r for r, _ in _rc(tie)} == {10, 11}
    near = am.edge_mask(20, 30, (80, am.quant(10.5 - 1 / 16)), (320, am.quant(10.5 - 1 / 16)), 1)
    assert _rc(near) == {(10, c) for c in range(5, 21)}


def test_diagonal_edge_matches_float_distance_away_from_ties():
    """A slanted edge against the Euclidean distance in f64, on pixels that are not within 1e-9 of the radius."""
    p0, p1 = (37, 21), (301, 170)  # lattice
    m = am.edge_mask(16, 24, p0, p1, 3)
    d = np.array(p1, float) - p0
    for r in range(1, 17):
        for c in range(1, 25):
            a = np.array([16.0 * c, 16.0 * r]) - p0
            t = min(1.0, max(0.0, a @ d / (d @ d)))
            dist = np.hypot(*(a - t * d))
            if abs(dist - 24.0) > 1e-9:
                assert m[r - 1, c - 1] == (dist < 24.0), (r, c, dist)


def test_label_geometry_and_blend():
    img = np.full((40, 60, 3), 100, np.uint8)
    am.draw_label(img, 3, 5, 17)
    digits, bw = am.label_layout(17)
    assert digits == [1, 7] and bw == 8 + 30 + 3 and am.LABEL_H == 29
    box = img[2:2 + 29, 4:4 + bw]
    white = (box == 255).all(2)
    assert ((box[~white] == ((200 + 765 + 2) // 5, (200 + 2) // 5, (200 + 2) // 5)).all())
    # the ink of "1" then "7", each glyph pixel a 3 x 3 block
    ink = sum(row.count("#") for d in (1, 7) for row in am.GLYPHS[d]) * 9
    assert int(white.sum()) == ink
    untouched = np.ones((40, 60), bool)
    untouched[2:31, 4:4 + bw] = False
    assert (img[untouched] == 100).all()
    assert all(len(g) == 7 and all(len(r) == 5 for r in g) for g in am.GLYPHS.values()) and len(am.GLYPHS) == 10


def test_numbering_closes_up_over_invalid_polygons():
    polys = np.array([[[2, 2], [6, 2], [6, 6], [2, 6]]] * 4, np.float64)
    polys[1, 0, 0] = np.nan
    polys[2, 3, 1] = 2.0 ** 20 + 1
    out, drawn = am.annotate(np.zeros((40, 60, 3), np.uint8), polys, [[1, 1]] * 4, [[0, 255, 0]] * 4)
    assert drawn == 2
    ref, _ = am.annotate(np.zeros((40, 60, 3), np.uint8), polys[[0, 3]], [[1, 1]] * 2, [[0, 255, 0]] * 2)
    assert np.array_equal(out, ref)  # labels 1 and 2, not 1 and 4


# ---- palette -----------------------------------------------------------------------------------------------------------------
def test_palette(rp):
    for n in (0, 1, 3, 64):
        p = rp.vivid_palette(n)
        assert p.shape == (n, 3) and p.dtype == np.uint8
        assert np.array_equal(p, rp.vivid_palette(n))
        assert np.array_equal(p, rp.vivid_palette(64)[:n])
        if n:
            assert (p.max(axis=1) == 255).all() and (p.min(axis=1) == 0).all()  # full value, full saturation
        assert len({tuple(r) for r in p}) == n
    # hue 0 is red; the second hue is frac(0.6180339887...) * 6 = sector 3 + 0.708..: (0, 1 - f, 1)
    f = 6 * ((math.sqrt(5) - 1) / 2) - 3
    assert tuple(rp.vivid_palette(2)[0]) == (255, 0, 0)
    assert tuple(rp.vivid_palette(2)[1]) == (0, math.floor(255 * (1 - f) + 0.5), 255)


# ---- warped_boxes -------------------------------------------------------------------------------------------------------------
F, HI, WI = 100.0, 101, 201
K = np.array([[F, 0, 101.0], [0, F, 51.0], [0, 0, 1.0]])  # the corners are at (x - cx) / f = -+1, (y - cy) / f = -+0.5
CORNER_SIGNS = [(-1, -1), (1, -1), (1, 1), (-1, 1)]  # (1,1), (1,W), (H,W), (H,1) as (sign of x, sign of y)


def _geo(mode, o0, o1, fpan=F, Rref=np.eye(3)):
    return {"mode": mode, "H": 500, "W": 700, "fPan": fpan, "o0": o0, "o1": o1, "Rref": np.asarray(Rref, float), "refIdx": 0}


def _expect(a_of, b_of, o0, o1, fpan):
    return np.array([[(a_of(sx, sy) - o0) * fpan + 1, (b_of(sx, sy) - o1) * fpan + 1] for sx, sy in CORNER_SIGNS])


@pytest.mark.parametrize("mode", ["planar", "cylindrical", "spherical", "equirectangular", "stereographic"])
def test_warped_boxes_identity_camera(rp, mode):
    cam = {"K": K, "R": np.eye(3)}
    o0, o1, fpan = -1.25, -0.75, 80.0
    a_of, b_of = {
        "planar": (lambda sx, sy: sx * 1.0, lambda sx, sy: sy * 0.5),
        "cylindrical": (lambda sx, sy: sx * math.pi / 4, lambda sx, sy: sy * 0.5 / math.sqrt(2)),
        "spherical": (lambda sx, sy: sx * math.pi / 4, lambda sx, sy: sy * math.atan(0.5 / math.sqrt(2))),
        "equirectangular": (lambda sx, sy: sx * math.pi / 4, lambda sx, sy: sy * math.atan(0.5 / math.sqrt(2))),
        # unit ray (2/3, 1/3, 2/3) * signs: a = (2/3) / (1 + 2/3) = 0.4, b = 0.2
        "stereographic": (lambda sx, sy: sx * 0.4, lambda sx, sy: sy * 0.2),
    }[mode]
    polys, centers = rp.warped_boxes([cam], [(HI, WI, 3)], _geo(mode, o0, o1, fpan))
    want = _expect(a_of, b_of, o0, o1, fpan)
    assert polys.shape == (1, 4, 2) and centers.shape == (1, 2)
    np.testing.assert_allclose(polys[0], want, rtol=0, atol=1e-9)
    np.testing.assert_allclose(centers[0], want.mean(0), rtol=0, atol=1e-9)


def test_warped_boxes_planar_is_the_inverse_of_the_renderer_map(rp):
    """Canvas column c looks along u = o0 + (c - 1) / fPan: with fPan = f and o0 = (1 - cx) / f the canvas IS the image, and the
    corners must come back as themselves (the reference's formula, without the + 1, puts them one pixel up and to the left)."""
    cam = {"K": K, "R": np.eye(3)}
    polys, _ = rp.warped_boxes([cam], [(HI, WI, 3)], _geo("planar", (1 - 101.0) / F, (1 - 51.0) / F))
    np.testing.assert_allclose(polys[0], [[1, 1], [WI, 1], [WI, HI], [1, HI]], rtol=0, atol=1e-9)


def test_warped_boxes_spherical_yaw_90(rp):
    """World -> camera R with the optical axis along world +x: rayW = R' (xn, yn, 1) = (1, yn, -xn), theta = atan2(1, -xn)."""
    R = np.array([[0, 0, -1.0], [0, 1, 0], [1, 0, 0]])
    o0, o1, fpan = 0.1, -0.6, 120.0
    polys, centers = rp.warped_boxes([{"K": K, "R": R}], [(HI, WI, 3)], _geo("spherical", o0, o1, fpan))
    want = _expect(lambda sx, sy: math.pi / 4 if sx < 0 else 3 * math.pi / 4, lambda sx, sy: sy * math.atan(0.5 / math.sqrt(2)), o0, o1, fpan)
    np.testing.assert_allclose(polys[0], want, rtol=0, atol=1e-9)
    np.testing.assert_allclose(centers[0], [(math.pi / 2 - o0) * fpan + 1, (0 - o1) * fpan + 1], rtol=0, atol=1e-9)


def test_warped_boxes_reference_rotation_and_guard(rp):
    """Planar and stereographic go through Rref: a camera that IS the reference sees its own pinhole grid whatever its rotation;
    the stereographic denominator is clamped at 1e-6 for a ray along -z (renderPanorama.m:1269)."""
    R = np.array([[0, 0, -1.0], [0, 1, 0], [1, 0, 0]])
    polys, _ = rp.warped_boxes([{"K": K, "R": R}], [(HI, WI, 3)], _geo("planar", 0.0, 0.0, 10.0, Rref=R))
    np.testing.assert_allclose(polys[0], _expect(lambda sx, sy: sx * 1.0, lambda sx, sy: sy * 0.5, 0, 0, 10.0), rtol=0, atol=1e-9)
    back = np.diag([-1.0, 1.0, -1.0])  # looks along world -z; K with the principal point on the corner (1, 1)
    Kc = np.array([[F, 0, 1.0], [0, F, 1.0], [0, 0, 1.0]])
    polys, _ = rp.warped_boxes([{"K": Kc, "R": back}], [(HI, WI, 3)], _geo("stereographic", 0.0, 0.0, 1.0))
    assert np.isfinite(polys).all() and np.allclose(polys[0, 0], [1.0, 1.0])  # x = y = 0 over the clamped denominator


# ---- displayPanorama's argument checks ------------------------------------------------------------------------------------------
def test_display_panorama_argument_errors(rp):
    cams = [{"K": K, "R": np.eye(3)}, {"K": K, "R": np.eye(3)}]
    imgs = [np.zeros((HI, WI, 3), np.uint8)] * 2
    sizes = [(HI, WI, 3)] * 2
    inp = {"panorama2DisplaynSave": ["spherical"]}
    with pytest.raises(ValueError, match=r"displayPanorama:InvalidRefIdxsLength: finalrefIdxs must have one entry per component \(1\)\."):
        rp.displayPanorama(inp, [cams], [1, 1], imgs, sizes, [[1, 2]])
    with pytest.raises(ValueError, match=r"displayPanorama:InvalidPanoIndicesLength: panoIndices must have one cell per component \(1\)\."):
        rp.displayPanorama(inp, [cams], [1], imgs, sizes, [[1, 2], [1]])
    with pytest.raises(ValueError, match=r"displayPanorama:InvalidPanoIndexType: panoIndices\{1\} must be a numeric vector of image indices\."):
        rp.displayPanorama(inp, [cams], [1], imgs, sizes, [["a", "b"]])
    with pytest.raises(ValueError, match=r"displayPanorama:InvalidPanoIndexType: panoIndices\{2\}"):
        rp.displayPanorama(inp, [cams, cams], [1, 1], imgs, sizes, [[1, 2], np.ones((2, 2))])
    with pytest.raises(ValueError, match=r"displayPanorama:ImageIndexOutOfBounds: panoIndices\{1\} has indices outside 1\.\.2\."):
        rp.displayPanorama(inp, [cams], [1], imgs, sizes, [[1, 3]])
    with pytest.raises(ValueError, match=r"displayPanorama:ImageIndexOutOfBounds: panoIndices\{2\} has indices outside 1\.\.2\."):
        rp.displayPanorama(inp, [cams, cams], [1, 1], imgs, sizes, [[1, 2], [0, 1]])
    # an empty component is skipped (:90) and an empty non-numeric cell passes the check (:75): no render, no device
    assert rp.displayPanorama(inp, [[], None], [1, 1], imgs, sizes, [[], ()]) == [{}, {}]
