"""CPU tests of the planar-scan compositor's host half: the size function, the wrapper's argument checks, the tent
tables and the footprints (against a brute-force restatement of the kernel's validity rule)."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest


@pytest.fixture(scope="module")
def rp(aps):
    return import_module(aps.__name__ + ".renderPanorama")


@pytest.fixture(scope="module")
def ip(aps):
    return import_module(aps.__name__ + ".imageProcessing")


def _formula(shapes, canvas, blending, levels):
    """aps_planar_composite_bytes as include/aps.h writes it down."""
    n, (Hc, Wc) = len(shapes), canvas
    P = Hc * Wc
    b = sum(h * w * c for h, w, c in shapes) + 4 * sum(h + w for h, w, _ in shapes)
    b += 160 * n + 16 * n * P + P + 3 * P
    if blending == "multiband":
        L = max(1, min(levels, int(np.floor(np.log2(min(Hc, Wc))))))
        px, h, w = [P], Hc, Wc
        for _ in range(1, L):
            h, w = max(1, h // 2), max(1, w // 2)
            px.append(h * w)
        D, I = sum(px[1:]), sum(px[1:L - 1])
        b += 16 * P + 16 * n * D + (16 * min(n, 16) * P if L > 1 else 0) + 16 * (P + D) + 16 * I
    return b


@pytest.mark.parametrize("shapes,canvas,blending,levels", [
    ([(60, 90, 3)] * 3, (70, 200), "multiband", 3),
    ([(480, 640, 3)] * 12, (1300, 2100), "multiband", 5),
    ([(480, 640, 1)] * 20, (700, 900), "multiband", 1),
    ([(33, 47, 3), (60, 90, 1)], (101, 77), "linear", 3),
    ([(768, 1024, 3)] * 2, (800, 1500), "none", 3),
    ([(20, 20, 3)] * 64, (9, 300), "multiband", 7),  # levels clamp to floor(log2(9)) = 3
])
def test_composite_bytes_equals_the_header_formula(rp, shapes, canvas, blending, levels):
    assert rp.planar_composite_bytes(shapes, canvas, blending, levels) == _formula(shapes, canvas, blending, levels)


def test_composite_bytes_grows_and_rejects(aps, rp):
    base = rp.planar_composite_bytes([(480, 640, 3)] * 4, (1000, 1500), "multiband", 3)
    assert rp.planar_composite_bytes([(480, 640, 3)] * 5, (1000, 1500), "multiband", 3) > base
    assert rp.planar_composite_bytes([(480, 640, 3)] * 4, (1001, 1500), "multiband", 3) > base
    assert rp.planar_composite_bytes([(480, 640, 3)] * 4, (1000, 1500), "multiband", 4) > base
    assert rp.planar_composite_bytes([(480, 640, 3)] * 4, (1000, 1500), "linear", 3) < base
    lib = aps.lib
    one = np.array([10], np.int32)
    three = np.array([3], np.int32)

    def raw(n, h, w, c, oh, ow, mode, lv):
        return lib.aps_planar_composite_bytes(n, aps._capi.ptr(h), aps._capi.ptr(w), aps._capi.ptr(c), oh, ow, mode, lv)

    MB = aps._capi.APS_BLEND_MULTIBAND
    assert raw(1, one, one, three, 10, 10, MB, 2) > 0
    assert raw(0, one, one, three, 10, 10, MB, 2) == aps._capi.APS_E_ARG
    assert raw(1, one, one, three, 0, 10, MB, 2) == aps._capi.APS_E_DIM
    assert raw(1, one, one, three, 10, -4, MB, 2) == aps._capi.APS_E_DIM
    assert raw(1, np.array([0], np.int32), one, three, 10, 10, MB, 2) == aps._capi.APS_E_DIM
    assert raw(1, one, one, np.array([2], np.int32), 10, 10, MB, 2) == aps._capi.APS_E_DIM
    assert raw(1, one, one, three, 10, 10, MB, 0) == aps._capi.APS_E_ARG
    assert raw(1, one, one, three, 10, 10, 7, 2) == aps._capi.APS_E_ARG
    big = np.full(65, 10, np.int32)
    assert raw(65, big, big, np.full(65, 3, np.int32), 10, 10, MB, 2) == aps._capi.APS_E_DIM
    assert b"64" in lib.aps_last_error()
    with pytest.raises(ValueError):
        rp.planar_composite_bytes([(10, 10, 3)], (0, 10))


def test_wrapper_refuses_bad_arguments_before_the_library(rp, ip, monkeypatch):
    view = ip.imref2dScratch((20, 30), (0.5, 30.5), (0.5, 20.5))
    img = np.zeros((10, 12, 3), np.uint8)

    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(rp.lib, "aps_planar_composite", boom, raising=False)
    monkeypatch.setattr(rp.lib, "aps_planar_gain_stats", boom, raising=False)
    with pytest.raises(ValueError):
        rp.planar_composite([img, img], [np.eye(3)], view)
    with pytest.raises(ValueError):
        rp.planar_composite([], [], view)
    with pytest.raises(ValueError):
        rp.planar_composite([img], [np.eye(4)], view)
    with pytest.raises(ValueError):
        rp.planar_composite([img], [np.zeros((3, 2))], view)
    with pytest.raises(ValueError):
        rp.planar_composite([img.astype(np.float32)], [np.eye(3)], view)
    with pytest.raises(ValueError):
        rp.planar_composite([np.zeros((10, 12, 2), np.uint8)], [np.eye(3)], view)
    with pytest.raises(ValueError):
        rp.planar_composite([img], [np.eye(3)], view, {"blending": "feather"})
    with pytest.raises(ValueError):
        rp.planar_composite([img], [np.eye(3)], view, {"blending": "multiband", "pyrLevels": 0})
    with pytest.raises(ValueError):
        rp.planar_composite([img], [np.eye(3)], view, {"blending": "multiband", "pyrSigma": 0.0})


def test_argument_errors_of_the_entry_point_need_no_device(aps):
    """NULL, N = 0, 65 images, levels 0, sigma <= 0 and a singular homography are refused before anything touches a device."""
    cp, lib = aps._capi, aps.lib
    img = np.zeros((10, 12, 3), np.uint8)
    out = np.zeros((20, 30, 3), np.uint8)

    def call(n=1, H=np.eye(3), levels=3, sigma=1.0, images=True, pano=True, mode=cp.APS_BLEND_MULTIBAND):
        pim = (C.c_void_p * max(n, 1))(*[cp.ptr(img)] * max(n, 1))
        ih, iw, ic = (np.full(max(n, 1), v, np.int32) for v in (10, 12, 3))
        Hs = np.ascontiguousarray(np.stack([np.asarray(H, np.float64).T.reshape(9)] * max(n, 1)))
        st = lib.aps_planar_composite(C.addressof(pim) if images else None, cp.ptr(ih), cp.ptr(iw), cp.ptr(ic), n, cp.ptr(Hs), 20, 30,
                                      0.5, 0.5, 1.0, 1.0, mode, levels, sigma, 0, None, cp.ptr(out) if pano else None, None)
        return st, lib.aps_last_error()

    for kw, code in [(dict(images=False), cp.APS_E_ARG), (dict(pano=False), cp.APS_E_ARG), (dict(n=0), cp.APS_E_ARG),
                     (dict(n=65), cp.APS_E_DIM), (dict(levels=0), cp.APS_E_ARG), (dict(sigma=0.0), cp.APS_E_ARG),
                     (dict(sigma=-1.0), cp.APS_E_ARG), (dict(mode=9), cp.APS_E_ARG),
                     (dict(H=np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])), cp.APS_E_ARG),
                     (dict(H=np.array([[1.0, 0.0, 3.0], [0.0, 1.0, np.nan], [0.0, 0.0, 1.0]])), cp.APS_E_ARG)]:
        st, msg = call(**kw)
        assert st == code and len(msg) > 0, (kw, st, msg)
    assert not out.any()


def test_tent_tables_are_warpWeights(aps, rp):
    for n in (1, 2, 3, 4, 5, 7, 60, 90, 479, 480, 640, 641, 768, 1024, 2160, 3840):
        t = np.zeros(n, np.float32)
        assert aps.lib.aps_planar_tent(n, aps._capi.ptr(t)) == 0
        w = rp.warpWeights([np.zeros((n, 3), np.uint8)])[0]  # tent(n) x tent(3) = tent(n) x [0, 1, 0]
        assert np.array_equal(t.view(np.uint32), np.ascontiguousarray(w[:, 1]).view(np.uint32)), n
    for h, w_ in ((60, 90), (33, 47), (480, 640)):
        th, tw = np.zeros(h, np.float32), np.zeros(w_, np.float32)
        aps.lib.aps_planar_tent(h, aps._capi.ptr(th))
        aps.lib.aps_planar_tent(w_, aps._capi.ptr(tw))
        full = rp.warpWeights([np.zeros((h, w_), np.uint8)])[0]
        assert np.array_equal((th[:, None] * tw[None, :]).view(np.uint32), full.view(np.uint32))


# ---- footprints ------------------------------------------------------------------------------------------------------------
def _valid_mask(T, h, w, Hc, Wc, x0, y0, sx, sy):
    """The kernel's validity rule restated in f64 (image_warp_h_kernel 'bilinear': imageWarp.m:125-168): canvas pixel ->
    world -> adj(H / H33) * p / det -> divide -> 1 <= floor(src) and floor(src) + 1 <= size, in both directions."""
    Hn = np.asarray(T, np.float64)
    Hn = Hn / Hn[2, 2] if Hn[2, 2] != 0 else Hn
    A = np.linalg.det(Hn) * np.linalg.inv(Hn)
    det = np.linalg.det(Hn)
    X = x0 + np.arange(Wc, dtype=np.float64)[None, :] * sx
    Y = y0 + np.arange(Hc, dtype=np.float64)[:, None] * sy
    with np.errstate(all="ignore"):
        s0 = ((A[0, 0] * X + A[0, 1] * Y) + A[0, 2]) / det
        s1 = ((A[1, 0] * X + A[1, 1] * Y) + A[1, 2]) / det
        s2 = ((A[2, 0] * X + A[2, 1] * Y) + A[2, 2]) / det
        wv = np.where(s2 < 0, -np.maximum(np.abs(s2), 1e-12), np.where(s2 > 0, np.maximum(np.abs(s2), 1e-12), 0.0))
        fx, fy = np.floor(s0 / wv), np.floor(s1 / wv)
        return (fx >= 1) & (fx + 1 <= w) & (fy >= 1) & (fy + 1 <= h)


def _canvas_for(ip, tforms, shapes):
    lims = [ip.outputLimitsScratch(T, (1, s[1]), (1, s[0])) for T, s in zip(tforms, shapes)]
    xMin, xMax = min(l[0][0] for l in lims), max(l[0][1] for l in lims)
    yMin, yMax = min(l[1][0] for l in lims), max(l[1][1] for l in lims)
    width, height = int(np.floor(xMax - xMin + 0.5)), int(np.floor(yMax - yMin + 0.5))
    return ip.imref2dScratch((height, width), (xMin, xMax), (yMin, yMax))


def _random_homography(rng, kind, h, w):
    a = rng.uniform(-np.pi, np.pi) if kind in ("rotated", "projective") else rng.uniform(-0.05, 0.05)
    s = rng.uniform(0.6, 1.6)
    R = s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    if kind == "sheared":
        R = R @ np.array([[1.0, rng.uniform(-0.8, 0.8)], [rng.uniform(-0.3, 0.3), 1.0]])
    T = np.eye(3)
    T[:2, :2] = R
    T[:2, 2] = rng.uniform(-200, 200, 2)
    if kind == "projective":  # strong, but the denominator stays >= 0.25 over the image
        p = rng.uniform(-1, 1, 2)
        p = 0.75 * p / (abs(p[0]) * w + abs(p[1]) * h)
        T[2, :2] = p
    elif kind != "sheared":
        T[2, :2] = rng.uniform(-2e-5, 2e-5, 2)
    return T * rng.uniform(0.5, 2.0)


def test_footprints_never_lose_a_valid_pixel(rp, ip):
    rng = np.random.default_rng(2026)
    fallbacks, tight, cases = 0, 0, 0
    for kind in ("mild", "rotated", "sheared", "projective"):
        for _ in range(12):
            shapes = [(int(rng.integers(20, 70)), int(rng.integers(20, 90))) for _ in range(3)]
            tforms = [_random_homography(rng, kind, *s) for s in shapes]
            view = _canvas_for(ip, tforms, shapes)
            Hc, Wc = view["ImageSize"]
            if Hc * Wc > 4_000_000:
                continue
            rects, whole = rp.planar_footprints(shapes, tforms, view)
            for T, s, r, wh in zip(tforms, shapes, rects, whole):
                m = _valid_mask(T, s[0], s[1], Hc, Wc, view["XWorldLimits"][0], view["YWorldLimits"][0],
                                view["PixelExtentInWorldX"], view["PixelExtentInWorldY"])
                inside = np.zeros_like(m)
                inside[r[1]:r[3], r[0]:r[2]] = True
                assert not (m & ~inside).any(), (kind, T, s, r)
                assert m.any()
                cases += 1
                fallbacks += int(wh)
                tight += int((r[2] - r[0]) * (r[3] - r[1]) < Hc * Wc)
    assert cases >= 120 and fallbacks == 0  # none of these crosses the horizon: no whole-canvas fallback
    assert tight >= cases // 2              # and the rectangles do cull: most are smaller than their three-image canvas


def test_horizon_crossing_homographies_fall_back_to_the_whole_canvas(rp, ip):
    rng = np.random.default_rng(5)
    h, w = 48, 64
    taken = 0
    for i in range(8):
        T = _random_homography(rng, "mild", h, w)
        T /= T[2, 2]
        # the line d = 0 through the middle of the image: the denominator changes sign over the corners
        n = rng.uniform(-1, 1, 2)
        n /= np.abs(n).sum()
        c = np.array([w * rng.uniform(0.3, 0.7), h * rng.uniform(0.3, 0.7)])
        T[2, :2] = n / 40.0
        T[2, 2] = -(T[2, :2] @ c)
        view = ip.imref2dScratch((150, 220), (-120.5, 99.5), (-80.5, 69.5))
        rects, whole = rp.planar_footprints([(h, w)], [T], view)
        m = _valid_mask(T, h, w, 150, 220, -120.5, -80.5, 1.0, 1.0)
        inside = np.zeros_like(m)
        r = rects[0]
        inside[r[1]:r[3], r[0]:r[2]] = True
        assert not (m & ~inside).any()
        assert whole[0] and tuple(r) == (0, 0, 220, 150)
        taken += int(whole[0])
    assert taken == 8
