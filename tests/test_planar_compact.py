"""CPU tests of the footprint-compact planar compositor's host half: the size function against the formula of include/aps.h
restated here (footprints per level, contributor lists), what it accepts and refuses, and the argument checks of the entry
point, none of which needs a device."""
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


# ---- the header's formula ---------------------------------------------------------------------------------------------------
def _clip(r, w, h):
    x0, y0, x1, y1 = max(r[0], 0), max(r[1], 0), min(r[2], w), min(r[3], h)
    return (0, 0, 0, 0) if x1 <= x0 or y1 <= y0 else (x0, y0, x1, y1)


def _map_interval(a, b, in_len, out_len):
    """Output pixels of the resize in_len -> out_len that can see the input interval [a, b) (planar section)."""
    if b <= a:
        return 0, 0
    s = out_len / in_len
    half = 1.0 if s < 1.0 else s
    oa, ob = int(np.floor(a * s - half - 2.0)), int(np.ceil(b * s + half + 2.0))
    oa, ob = max(oa, 0), min(ob, out_len)
    return (0, 0) if ob <= oa else (oa, ob)


def _area(r):
    return (r[2] - r[0]) * (r[3] - r[1])


def _formula(rp, shapes, tforms, view, blending, levels):
    """aps_planar_composite_compact_bytes as include/aps.h writes it down."""
    n, (Hc, Wc) = len(shapes), view["ImageSize"]
    P = Hc * Wc
    L = max(1, min(levels, int(np.floor(np.log2(min(Hc, Wc)))))) if blending == "multiband" else 1
    hs, ws = [Hc], [Wc]
    for _ in range(1, L):
        hs.append(max(1, hs[-1] // 2))
        ws.append(max(1, ws[-1] // 2))
    rects, _ = rp.planar_footprints([s[:2] for s in shapes], tforms, view)
    G = [[_clip(tuple(int(v) for v in r), Wc, Hc) for r in rects]]
    layers, blur_max, lists = 0, 0, 0
    for l in range(L):
        B = [g if g[2] <= g[0] else _clip((g[0] - 4, g[1] - 4, g[2] + 4, g[3] + 4), ws[l], hs[l]) for g in G[l]]
        if l + 1 < L:
            nxt = []
            for g, b in zip(G[l], B):
                if g[2] <= g[0]:
                    nxt.append(g)
                    continue
                xa, xb = _map_interval(b[0], b[2], ws[l], ws[l + 1])
                ya, yb = _map_interval(b[1], b[3], hs[l], hs[l + 1])
                nxt.append((0, 0, 0, 0) if xb <= xa or yb <= ya else (xa, ya, xb, yb))
            G.append(nxt)
            blur_max = max(blur_max, sum(_area(b) for b in B))
        layers += sum(_area(g) for g in G[l])
        blocks = -(-hs[l] // 64) * -(-ws[l] // 64)
        entries = sum(((g[2] - 1) // 64 - g[0] // 64 + 1) * ((g[3] - 1) // 64 - g[1] // 64 + 1) for g in G[l] if g[2] > g[0])
        lists += blocks + 1 + entries
    b = sum(h * w * c for h, w, c in shapes) + 4 * sum(h + w for h, w, _ in shapes)
    b += 160 * n + 32 * n * (2 * L - 1) + 16 * layers + 16 * blur_max + 4 * lists + P + 3 * P
    if blending == "multiband":
        px = [h * w for h, w in zip(hs, ws)]
        D, I = sum(px[1:]), sum(px[1:L - 1])
        b += 16 * P + 16 * (P + D) + 16 * I
    return b


def _canvas_for(ip, tforms, shapes):
    lims = [ip.outputLimitsScratch(T, (1, s[1]), (1, s[0])) for T, s in zip(tforms, shapes)]
    xMin, xMax = min(l[0][0] for l in lims), max(l[0][1] for l in lims)
    yMin, yMax = min(l[1][0] for l in lims), max(l[1][1] for l in lims)
    width, height = int(np.floor(xMax - xMin + 0.5)), int(np.floor(yMax - yMin + 0.5))
    return ip.imref2dScratch((height, width), (xMin, xMax), (yMin, yMax))


def _grid_tforms(rng, rows, cols, h, w, overlap):
    Hs = []
    for r in range(rows):
        for c in range(cols):
            a = rng.uniform(-0.01, 0.01)
            T = np.array([[np.cos(a), -np.sin(a), c * w * (1 - overlap) + rng.uniform(-3, 3)],
                          [np.sin(a), np.cos(a), r * h * (1 - overlap) + rng.uniform(-3, 3)],
                          [rng.uniform(-1e-5, 1e-5), rng.uniform(-1e-5, 1e-5), 1.0]])
            Hs.append(T)
    return Hs


@pytest.mark.parametrize("rows,cols,shape,overlap,blending,levels", [
    (1, 3, (60, 90, 3), 0.4, "multiband", 3),
    (3, 4, (480, 640, 3), 0.35, "multiband", 5),
    (4, 5, (48, 64, 1), 0.5, "multiband", 1),
    (1, 2, (33, 47, 3), 0.3, "linear", 3),
    (2, 1, (768, 1024, 3), 0.2, "none", 3),
    (20, 13, (24, 32, 3), 0.5, "multiband", 7),
])
def test_compact_bytes_equals_the_header_formula(rp, ip, rows, cols, shape, overlap, blending, levels):
    rng = np.random.default_rng(rows * 100 + cols)
    shapes = [shape] * (rows * cols)
    tforms = _grid_tforms(rng, rows, cols, shape[0], shape[1], overlap)
    view = _canvas_for(ip, tforms, shapes)
    got = rp.planar_composite_compact_bytes(shapes, view["ImageSize"], tforms, view, blending, levels)
    assert got == _formula(rp, shapes, tforms, view, blending, levels)


def test_compact_bytes_of_mixed_sizes_and_a_whole_canvas_footprint(rp, ip):
    shapes = [(48, 64, 3), (33, 47, 3), (60, 90, 3)]
    T = np.array([[1.0, 0.02, 30.0], [-0.01, 1.0, 5.0], [1.0 / 40.0, 0.0, -0.8]])  # horizon across the image
    tforms = [np.eye(3), T, np.array([[1.0, 0, 20.0], [0, 1.0, -30.0], [0, 0, 1.0]])]
    view = ip.imref2dScratch((150, 220), (-120.5, 99.5), (-80.5, 69.5))
    _, whole = rp.planar_footprints([s[:2] for s in shapes], tforms, view)
    assert list(whole) == [False, True, False]
    for blending in ("multiband", "linear"):
        assert rp.planar_composite_compact_bytes(shapes, (150, 220), tforms, view, blending, 4) == _formula(rp, shapes, tforms, view, blending, 4)


def test_compact_bytes_accepts_many_images_and_rejects_what_the_composite_rejects(aps, rp, ip):
    cp, lib = aps._capi, aps.lib
    MB = cp.APS_BLEND_MULTIBAND

    def raw(n, h=10, w=10, c=3, oh=40, ow=40, mode=MB, lv=2, H=np.eye(3), null=None, sx=1.0):
        m = max(n, 1)
        ih, iw, ic = (np.full(m, v, np.int32) for v in (h, w, c))
        Hs = np.ascontiguousarray(np.stack([np.asarray(H, np.float64).T.reshape(9)] * m))
        args = [cp.ptr(ih), cp.ptr(iw), cp.ptr(ic), cp.ptr(Hs)]
        if null is not None:
            args[null] = None
        return lib.aps_planar_composite_compact_bytes(n, *args, oh, ow, 0.5, 0.5, sx, 1.0, mode, lv)

    assert raw(1) > 0
    for k in range(4):
        assert raw(1, null=k) == cp.APS_E_ARG
    assert raw(0) == cp.APS_E_ARG
    assert raw(1, oh=0) == cp.APS_E_DIM and raw(1, ow=-4) == cp.APS_E_DIM
    assert raw(1, h=0) == cp.APS_E_DIM and raw(1, c=2) == cp.APS_E_DIM
    assert raw(1, lv=0) == cp.APS_E_ARG and raw(1, mode=7) == cp.APS_E_ARG and raw(1, sx=0.0) == cp.APS_E_ARG
    assert raw(1, H=np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])) == cp.APS_E_ARG
    assert raw(1, H=np.array([[1.0, 0.0, 3.0], [0.0, 1.0, np.nan], [0.0, 0.0, 1.0]])) == cp.APS_E_ARG
    assert len(lib.aps_last_error()) > 0
    # no cap of 64: 65 and 1000 images are sizes like any other, and every image adds its own bytes only
    b64, b65, b1000 = raw(64), raw(65), raw(1000)
    assert 0 < b64 < b65 < b1000
    assert b1000 - b65 == 935 * (b65 - b64)
    with pytest.raises(ValueError):
        rp.planar_composite_compact_bytes([(10, 10, 3)], (0, 10), [np.eye(3)], {"ImageSize": (0, 10), "XWorldLimits": (0.5, 10.5), "YWorldLimits": (0.5, 0.5), "PixelExtentInWorldX": 1.0, "PixelExtentInWorldY": 1.0})
    with pytest.raises(ValueError):
        rp.planar_composite_compact_bytes([(10, 10, 3)], (40, 40), [np.eye(3)], ip.imref2dScratch((40, 40), (0.5, 40.5), (0.5, 40.5)), "feather")


@pytest.mark.parametrize("blending,levels", [("multiband", 4), ("multiband", 1), ("linear", 3)])
def test_no_term_of_the_formula_multiplies_the_image_count_by_the_canvas(rp, ip, blending, levels):
    """One more image in the interior costs the same on a canvas 16 times larger (canvas sides are multiples of
    2^(levels-1), the image sits at the same pixels of both and far from their borders, so no footprint is clipped), where the
    dense formula charges it 16 times the layers."""
    shape = (40, 60, 3)
    base = [np.array([[1.0, 0, 10.0], [0, 1.0, 12.0], [0, 0, 1.0]]), np.array([[1.0, 0, 50.0], [0, 1.0, 20.0], [0, 0, 1.0]])]
    extra = np.array([[1.01, 0.01, 200.0], [-0.01, 0.99, 180.0], [1e-5, 0, 1.0]])
    added = []
    for Hc, Wc in ((512, 768), (2048, 3072)):
        view = ip.imref2dScratch((Hc, Wc), (0.5, Wc + 0.5), (0.5, Hc + 0.5))
        two = rp.planar_composite_compact_bytes([shape] * 2, (Hc, Wc), base, view, blending, levels)
        three = rp.planar_composite_compact_bytes([shape] * 3, (Hc, Wc), base + [extra], view, blending, levels)
        added.append(three - two)
        assert three - two < rp.planar_composite_bytes([shape] * 3, (Hc, Wc), blending, levels) - rp.planar_composite_bytes([shape] * 2, (Hc, Wc), blending, levels)
    assert 0 < added[1] <= added[0]
    assert added[0] < 40 * 16 * (40 + 16) * (60 + 16)  # a few footprints' worth, against 16 * 512 * 768 per dense layer


def test_the_bench_sized_scan_fits_compact_and_not_dense(rp, ip):
    """The 8 x 8 scan of 3840 x 2160 views at 35 % overlap (host arithmetic only)."""
    rng = np.random.default_rng(88)
    shapes = [(2160, 3840, 3)] * 64
    tforms = _grid_tforms(rng, 8, 8, 2160, 3840, 0.35)
    view = _canvas_for(ip, tforms, shapes)
    assert view["ImageSize"][0] * view["ImageSize"][1] > 240e6
    assert rp.planar_composite_bytes(shapes, view["ImageSize"], "multiband", 3) > 288e9
    compact = rp.planar_composite_compact_bytes(shapes, view["ImageSize"], tforms, view, "multiband", 3)
    assert compact < 288e9 / 4 and compact == _formula(rp, shapes, tforms, view, "multiband", 3)


# ---- the entry point's argument checks ---------------------------------------------------------------------------------------
def test_argument_errors_of_the_compact_entry_point_need_no_device(aps):
    """NULL, N = 0, levels 0, sigma <= 0 and a singular homography are refused before anything touches a device; 65 images are
    NOT an argument error: the call gets past the checks and fails only for want of a device."""
    cp, lib = aps._capi, aps.lib
    img = np.zeros((10, 12, 3), np.uint8)
    out = np.zeros((20, 30, 3), np.uint8)

    def call(n=1, H=np.eye(3), levels=3, sigma=1.0, images=True, pano=True, mode=cp.APS_BLEND_MULTIBAND):
        pim = (C.c_void_p * max(n, 1))(*[cp.ptr(img)] * max(n, 1))
        ih, iw, ic = (np.full(max(n, 1), v, np.int32) for v in (10, 12, 3))
        Hs = np.ascontiguousarray(np.stack([np.asarray(H, np.float64).T.reshape(9)] * max(n, 1)))
        st = lib.aps_planar_composite_compact(C.addressof(pim) if images else None, cp.ptr(ih), cp.ptr(iw), cp.ptr(ic), n, cp.ptr(Hs),
                                              20, 30, 0.5, 0.5, 1.0, 1.0, mode, levels, sigma, 0, None, cp.ptr(out) if pano else None,
                                              None)
        return st, lib.aps_last_error()

    for kw, code in [(dict(images=False), cp.APS_E_ARG), (dict(pano=False), cp.APS_E_ARG), (dict(n=0), cp.APS_E_ARG),
                     (dict(levels=0), cp.APS_E_ARG), (dict(sigma=0.0), cp.APS_E_ARG), (dict(sigma=-1.0), cp.APS_E_ARG),
                     (dict(mode=9), cp.APS_E_ARG),
                     (dict(H=np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])), cp.APS_E_ARG),
                     (dict(H=np.array([[1.0, 0.0, 3.0], [0.0, 1.0, np.nan], [0.0, 0.0, 1.0]])), cp.APS_E_ARG)]:
        st, msg = call(**kw)
        assert st == code and len(msg) > 0, (kw, st, msg)
    assert not out.any()
    st, msg = call(n=65)
    assert st == (cp.APS_E_DEVICE if lib.aps_device_count() <= 0 else cp.APS_OK), (st, msg)
    # the statistics: same refusals, and a bound of their own on the image count
    N = np.zeros((1, 1))
    pim = (C.c_void_p * 1)(cp.ptr(img))
    one = [np.full(1, v, np.int32) for v in (10, 12, 3)]
    Hs = np.ascontiguousarray(np.eye(3).reshape(1, 9))
    st = lib.aps_planar_gain_stats_compact(C.addressof(pim), *[cp.ptr(a) for a in one], 1, cp.ptr(Hs), 20, 30, 0.5, 0.5, 1.0, 1.0, 0,
                                           cp.ptr(N), cp.ptr(N), cp.ptr(N))
    assert st == cp.APS_E_ARG
    st = lib.aps_planar_gain_stats_compact(C.addressof(pim), *[cp.ptr(a) for a in one], 1, cp.ptr(Hs), 20, 30, 0.5, 0.5, 1.0, 1.0, 4,
                                           None, cp.ptr(N), cp.ptr(N))
    assert st == cp.APS_E_ARG


def test_wrappers_refuse_bad_arguments_before_the_library(rp, ip, monkeypatch):
    view = ip.imref2dScratch((20, 30), (0.5, 30.5), (0.5, 20.5))
    img = np.zeros((10, 12, 3), np.uint8)

    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(rp.lib, "aps_planar_composite_compact", boom, raising=False)
    monkeypatch.setattr(rp.lib, "aps_planar_gain_stats_compact", boom, raising=False)
    for bad in [dict(images=[img, img], tforms=[np.eye(3)]), dict(images=[], tforms=[]), dict(images=[img], tforms=[np.eye(4)]),
                dict(images=[img.astype(np.float32)], tforms=[np.eye(3)]),
                dict(images=[img], tforms=[np.eye(3)], opts={"blending": "feather"}),
                dict(images=[img], tforms=[np.eye(3)], opts={"blending": "multiband", "pyrLevels": 0}),
                dict(images=[img], tforms=[np.eye(3)], opts={"blending": "multiband", "pyrSigma": 0.0})]:
        with pytest.raises(ValueError):
            rp.planar_composite_compact(bad["images"], bad["tforms"], view, bad.get("opts"))


def test_routing_rule_without_a_device(rp):
    """Which compositor a set is sent to (the dtype and channel rules are those of the dense path)."""
    u8 = np.zeros((10, 12, 3), np.uint8)
    assert rp._planar_device_covers([u8] * 3, {}) == "device"
    assert rp._planar_device_covers([u8] * 64, {}) == "device"
    assert rp._planar_device_covers([u8] * 65, {}) == "compact"
    assert rp._planar_device_covers([u8] * 3, {"planarCompositor": "compact"}) == "compact"
    assert rp._planar_device_covers([u8] * 70, {"planarCompositor": "host"}) is None
    assert rp._planar_device_covers([u8.astype(np.float32)] * 70, {}) is None
    assert rp._planar_device_covers([u8, u8[..., 0]], {"planarCompositor": "compact"}) is None
