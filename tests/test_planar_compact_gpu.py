"""The footprint-compact planar compositor (aps_planar_composite_compact, aps_planar_gain_stats_compact).

Up to 64 views the yardsticks are the dense compositor and the host-orchestrated path of the same commit; above 64 views,
where neither can run multiband, the oracle chain test_render_gpu.py uses for planar scans (oracle.image_warp_h on
(float32)u8 / 255 and on the clipped tent map, oracle.multiband_blend / linear_blend / first argmax, void paint,
uint8(round(255 * v)) with the product in f64).  The condition is byte identity of the uint8 panorama everywhere."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rp(gpu):
    return import_module(gpu.__name__ + ".renderPanorama")


@pytest.fixture(scope="module")
def ip(gpu):
    return import_module(gpu.__name__ + ".imageProcessing")


def _cams(Hs):
    return [{"H2refined": np.asarray(H, np.float64), "noRotation": 1} for H in Hs]


def _three_ways(rp, imgs, Hs, opts, gains=None):
    """compact, dense and host panoramas of one set (at most 64 views)."""
    sizes = [tuple(np.asarray(im).shape) for im in imgs]
    out = []
    for which in ("compact", "device", "host"):
        pano, _ = rp.renderPanorama({}, imgs, sizes, _cams(Hs), "planar", 0, dict(opts, planarCompositor=which), gains=gains)
        out.append(pano)
    return out


def _same(a, b, what=""):
    assert a.dtype == np.uint8 and a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %d bytes differ" % (what, int((a != b).sum()))


def _all_same(three):
    _same(three[0], three[1], "compact vs dense")
    _same(three[0], three[2], "compact vs host")


def _three(rng):
    imgs = [rng.integers(0, 256, (60, 90, 3), dtype=np.uint8) for _ in range(3)]
    Hs = [np.eye(3), np.array([[1.0, 0.01, 55.0], [-0.01, 1.0, 4.0], [1e-5, 0, 1.0]]),
          np.array([[0.98, 0.0, 108.5], [0.02, 1.01, -6.0], [0, 2e-5, 1.0]])]
    return imgs, Hs


def _grid_scan(rng, rows, cols, h, w, overlap=0.35):
    """rows x cols views of a translating camera with mildly projective homographies and ~`overlap` overlap."""
    imgs, Hs = [], []
    for r in range(rows):
        for c in range(cols):
            imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            a = rng.uniform(-0.01, 0.01)
            T = np.array([[np.cos(a), -np.sin(a), c * w * (1 - overlap) + rng.uniform(-3, 3)],
                          [np.sin(a), np.cos(a), r * h * (1 - overlap) + rng.uniform(-3, 3)],
                          [rng.uniform(-1e-5, 1e-5), rng.uniform(-1e-5, 1e-5), 1.0]])
            T[:2, :2] *= rng.uniform(0.98, 1.02)
            Hs.append(T)
    return imgs, Hs


def _view_of(ip, imgs, Hs):
    lims = [ip.outputLimitsScratch(np.asarray(T, np.float64), (1, int(im.shape[1])), (1, int(im.shape[0]))) for T, im in zip(Hs, imgs)]
    xMin, xMax = min(l[0][0] for l in lims), max(l[0][1] for l in lims)
    yMin, yMax = min(l[1][0] for l in lims), max(l[1][1] for l in lims)
    width, height = int(np.floor(xMax - xMin + 0.5)), int(np.floor(yMax - yMin + 0.5))
    return ip.imref2dScratch((height, width), (xMin, xMax), (yMin, yMax))


def _oracle_layers(imgs, Hs, height, width, x0, y0, sx, sy):
    Iw, Ww = [], []
    for im, H in zip(imgs, Hs):
        h, w = im.shape[:2]
        Iw.append(oracle.image_warp_h(im.astype(np.float32) / 255.0, H, height, width, x0, y0, sx, sy, 0.0))
        tent = np.outer(oracle.tent(h), oracle.tent(w)).astype(np.float32)
        Ww.append(np.clip(oracle.image_warp_h(tent, H, height, width, x0, y0, sx, sy, 0.0), 0, 1))
    return Iw, Ww


def _oracle_chain(imgs, Hs, height, width, x0, y0, sx, sy, blending, levels=3, sigma=1.0, white=False):
    Iw, Ww = _oracle_layers(imgs, Hs, height, width, x0, y0, sx, sy)
    Cc, Wc = np.stack(Iw), np.stack(Ww)
    if blending == "multiband":
        F = oracle.multiband_blend(Cc, Wc, levels, sigma)
    elif blending == "linear":
        F = oracle.linear_blend(Cc, Wc)
    else:
        F = np.take_along_axis(np.moveaxis(Cc, 0, 3), np.argmax(Wc, 0)[:, :, None, None], 3)[..., 0]
    F = np.array(F, np.float32)
    if blending == "multiband":
        F = np.clip(F, 0, 1)
    F[~(Wc > 0).any(0)] = 1.0 if white else 0.0
    return np.clip(np.floor(255.0 * F.astype(np.float64) + 0.5), 0, 255).astype(np.uint8), (Wc > 0).any(0)


# ---- compact against dense and host ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canvas", ["black", "white"])
@pytest.mark.parametrize("blending,levels,sigma", [("none", 3, 1.0), ("linear", 3, 1.0), ("multiband", 1, 1.0),
                                                   ("multiband", 3, 1.0), ("multiband", 5, 1.0), ("multiband", 3, 1.6),
                                                   ("multiband", 5, 1.6), ("multiband", 1, 1.6)])
def test_three_small_views(rp, blending, levels, sigma, canvas):
    imgs, Hs = _three(np.random.default_rng(21))
    three = _three_ways(rp, imgs, Hs, {"blending": blending, "pyrLevels": levels, "pyrSigma": sigma, "canvasColor": canvas})
    _all_same(three)
    assert (three[0] != (255 if canvas == "white" else 0)).mean() > 0.5


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_twelve_view_scan(rp, blending):
    imgs, Hs = _grid_scan(np.random.default_rng(31), 3, 4, 480, 640)
    three = _three_ways(rp, imgs, Hs, {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0})
    _all_same(three)
    assert three[0].shape[0] > 2 * 480 and three[0].shape[1] > 2.5 * 640


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_twenty_views_four_levels(rp, blending):
    imgs, Hs = _grid_scan(np.random.default_rng(32), 4, 5, 48, 64, overlap=0.5)
    assert len(imgs) == 20
    _all_same(_three_ways(rp, imgs, Hs, {"blending": blending, "pyrLevels": 4, "pyrSigma": 1.0, "canvasColor": "white"}))


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_views_of_different_sizes(rp, blending):
    rng = np.random.default_rng(33)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((60, 90), (45, 120), (77, 51))]
    Hs = [np.eye(3), np.array([[1.02, 0.03, 50.0], [-0.02, 0.97, 10.0], [2e-5, 1e-5, 1.0]]),
          np.array([[0.9, -0.1, 20.5], [0.1, 0.9, 40.25], [0, -3e-5, 1.0]])]
    _all_same(_three_ways(rp, imgs, Hs, {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0}))


@pytest.mark.parametrize("shape", [(60, 90, 1), (60, 90)])
@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_single_channel_set(rp, blending, shape):
    imgs3, Hs = _three(np.random.default_rng(34))
    imgs = [np.ascontiguousarray(im[..., :1]).reshape(shape) for im in imgs3]
    _all_same(_three_ways(rp, imgs, Hs, {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0}))


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_explicit_gains(rp, blending):
    imgs, Hs = _three(np.random.default_rng(35))
    g = np.array([[0.8, 0.9, 1.0], [1.25, 1.1, 0.95], [1.0, 0.7, 1.3]], np.float32)
    three = _three_ways(rp, imgs, Hs, {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0}, gains=g)
    _all_same(three)
    plain = _three_ways(rp, imgs, Hs, {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0})[0]
    assert not np.array_equal(three[0], plain)


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_horizon_crossing_homography(rp, ip, blending):
    """The second homography's denominator changes sign inside its image: that one layer is canvas-sized."""
    rng = np.random.default_rng(36)
    imgs = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in range(2)]
    T = np.array([[1.0, 0.02, 30.0], [-0.01, 1.0, 5.0], [1.0 / 40.0, 0.0, -0.8]])  # d = 0 at x = 32
    Hs = [np.eye(3), T]
    view = ip.imref2dScratch((150, 220), (-120.5, 99.5), (-80.5, 69.5))
    _, whole = rp.planar_footprints([(48, 64)] * 2, Hs, view)
    assert list(whole) == [False, True]
    o = {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0, "canvasColor": "black"}
    compact = rp.planar_composite_compact(imgs, Hs, view, o)
    _same(compact, rp.planar_composite(imgs, Hs, view, o), "compact vs dense")
    _same(compact, rp._planar_host(imgs, Hs, view, o), "compact vs host")
    assert compact.any()


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_whole_canvas_footprints_change_no_byte(rp, monkeypatch, blending):
    imgs, Hs = _grid_scan(np.random.default_rng(37), 2, 3, 96, 128)
    opts = {"blending": blending, "pyrLevels": 4, "pyrSigma": 1.0}
    monkeypatch.delenv("APS_PLANAR_NO_CULL", raising=False)
    culled = _three_ways(rp, imgs, Hs, opts)
    _all_same(culled)
    monkeypatch.setenv("APS_PLANAR_NO_CULL", "1")
    sizes = [im.shape for im in imgs]
    whole, _ = rp.renderPanorama({}, imgs, sizes, _cams(Hs), "planar", 0, dict(opts, planarCompositor="compact"))
    _same(whole, culled[0], "whole-canvas footprints vs culled")


@pytest.mark.parametrize("blending", ["multiband", "none"])
def test_resident_tensors_in_and_out(rp, blending):
    import torch

    imgs, Hs = _three(np.random.default_rng(39))
    opts = {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0}
    ref, _ = rp.renderPanorama({}, imgs, [(60, 90, 3)] * 3, _cams(Hs), "planar", 0, dict(opts, planarCompositor="host"))
    dimgs = [torch.from_numpy(im).cuda() for im in imgs]
    out, _ = rp.renderPanorama({}, dimgs, [(60, 90, 3)] * 3, _cams(Hs), "planar", 0, dict(opts, planarCompositor="compact"), device_out=True)
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), ref)


def _pano_and_cover(rp, entry, imgs, Hs, view, o):
    """One compositor entry point called as planar_composite calls it, with the coverage map asked for as well."""
    n, keep, pim, ih, iw, ic, Hm = rp._planar_args(imgs, Hs)
    Hc, Wc, x0, y0, sx, sy = rp._planar_view(view)
    pano, cov = np.zeros((Hc, Wc, 3), np.uint8), np.zeros((Hc, Wc), np.uint8)
    rp.check(getattr(rp.lib, entry)(C.addressof(pim), rp.ptr(ih), rp.ptr(iw), rp.ptr(ic), n, rp.ptr(Hm), Hc, Wc, x0, y0, sx, sy,
                                    rp._BLEND[o["blending"]], int(o["pyrLevels"]), float(o["pyrSigma"]), 0, None, rp.ptr(pano), rp.ptr(cov)))
    del keep
    return pano, cov


@pytest.mark.parametrize("blending", ["none", "linear", "multiband"])
@pytest.mark.parametrize("absent,xlim", [(0, (95.5, 205.5)), (2, (-4.5, 100.5))])
def test_a_view_wholly_outside_the_canvas(rp, ip, blending, absent, xlim):
    """The canvas cropped so that the first (then the last) of three views has an empty footprint, (0, 0, 0, 0), at every
    pyramid level, while the other two overlap inside it: dense, compact and host still agree on every byte, and the gain
    statistics carry zeros for the absent view."""
    imgs, Hs = _three(np.random.default_rng(41))
    view = ip.imref2dScratch((80, int(xlim[1] - xlim[0])), xlim, (-10.5, 69.5))
    rects, whole = rp.planar_footprints([(60, 90)] * 3, Hs, view)
    assert not whole.any() and [tuple(r) == (0, 0, 0, 0) for r in rects] == [k == absent for k in range(3)]
    o = {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0, "canvasColor": "black"}
    compact, dense = rp.planar_composite_compact(imgs, Hs, view, o), rp.planar_composite(imgs, Hs, view, o)
    _same(compact, dense, "compact vs dense")
    _same(compact, rp._planar_host(imgs, Hs, view, o), "compact vs host")
    cp, cc = _pano_and_cover(rp, "aps_planar_composite_compact", imgs, Hs, view, o)
    dp, dc = _pano_and_cover(rp, "aps_planar_composite", imgs, Hs, view, o)
    _same(cp, compact, "compact with coverage vs without")
    _same(dp, dense, "dense with coverage vs without")
    _same(cc, dc, "coverage, compact vs dense")
    assert 0 < cc.mean() < 1 and compact[cc > 0].any()  # the canvas is 20 rows taller than the views: some void, some cover
    N, sI, sJ = rp.planar_gain_stats_compact(imgs, Hs, view, 2)
    dN, dI, dJ = rp.planar_gain_stats(imgs, Hs, view, 2)
    assert np.array_equal(N, dN) and np.allclose(sI, dI, rtol=1e-12, atol=0) and np.allclose(sJ, dJ, rtol=1e-12, atol=0)
    a, b = [k for k in range(3) if k != absent]
    assert N[a, b] > 0 and N.sum() == N[a, b]
    for M in (N, sI, sJ, dN, dI, dJ):
        assert not M[absent].any() and not M[:, absent].any()


# ---- more than 64 views: the oracle chain ----------------------------------------------------------------------------------
@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
@pytest.mark.parametrize("rows,cols", [(10, 10), (20, 13)])
def test_scans_of_more_than_64_views_match_the_oracle_chain(rp, ip, rows, cols, blending):
    """100 and 260 views (260 crosses four 64-bit words and 255) through renderPanorama with default options.  Before the
    compact compositor the multiband cases ended in normalize_weights' "more than 64 layers in one tile"."""
    imgs, Hs = _grid_scan(np.random.default_rng(1000 + rows), rows, cols, 24, 32, overlap=0.5)
    assert len(imgs) == rows * cols > 64
    pano, _ = rp.renderPanorama({"forcePlanarScan": True}, imgs, [(24, 32, 3)] * len(imgs), [{"H2refined": H} for H in Hs], "planar", 0,
                                {"blending": blending, "pyrLevels": 3})
    view = _view_of(ip, imgs, Hs)
    height, width = view["ImageSize"]
    assert pano.shape == (height, width, 3)
    ref, cov = _oracle_chain(imgs, Hs, height, width, view["XWorldLimits"][0], view["YWorldLimits"][0], view["PixelExtentInWorldX"],
                             view["PixelExtentInWorldY"], blending, 3, 1.0)
    assert cov.mean() > 0.8
    _same(pano, ref, "compact vs oracle chain")


# ---- gain statistics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,h,w,overlap,ds", [(3, 4, 480, 640, 0.35, 4), (3, 4, 480, 640, 0.35, 3), (10, 10, 24, 32, 0.5, 1),
                                                      (10, 10, 24, 32, 0.5, 2)])
def test_gain_statistics_from_the_compact_layers(rp, ip, rows, cols, h, w, overlap, ds):
    """Counts exactly those of oracle.gain_overlap_stats_warped on the oracle-warped canvases, sums to the relative 1e-12
    the dense path is held to (f64 sums of f32 values in an unspecified order)."""
    imgs, Hs = _grid_scan(np.random.default_rng(50 + rows), rows, cols, h, w, overlap)
    view = _view_of(ip, imgs, Hs)
    height, width = view["ImageSize"]
    Iw, Ww = _oracle_layers(imgs, Hs, height, width, view["XWorldLimits"][0], view["YWorldLimits"][0], view["PixelExtentInWorldX"],
                            view["PixelExtentInWorldY"])
    oN, oI, oJ = oracle.gain_overlap_stats_warped(Iw, Ww, ds)
    N, sI, sJ = rp.planar_gain_stats_compact(imgs, Hs, view, ds)
    assert np.array_equal(N, oN) and (N > 0).sum() >= len(imgs)
    assert np.allclose(sI, oI, rtol=1e-12, atol=0) and np.allclose(sJ, oJ, rtol=1e-12, atol=0)
    if len(imgs) <= 64:
        dN, dI, dJ = rp.planar_gain_stats(imgs, Hs, view, ds)
        assert np.array_equal(N, dN) and np.allclose(sI, dI, rtol=1e-12, atol=0) and np.allclose(sJ, dJ, rtol=1e-12, atol=0)


@pytest.mark.parametrize("blending", ["multiband", "linear"])
def test_gain_compensation_through_the_compact_path(rp, blending):
    rng = np.random.default_rng(61)
    imgs, Hs = _grid_scan(rng, 3, 4, 480, 640)
    imgs = [np.clip(im.astype(np.float32) * s, 0, 255).astype(np.uint8) for im, s in zip(imgs, rng.uniform(0.7, 1.0, len(imgs)))]
    opts = {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0, "gainCompensation": 1, "sigmag": 10.0}
    sizes = [im.shape for im in imgs]
    compact, _ = rp.renderPanorama({}, imgs, sizes, _cams(Hs), "planar", 0, dict(opts, planarCompositor="compact"))
    dense, _ = rp.renderPanorama({}, imgs, sizes, _cams(Hs), "planar", 0, dict(opts, planarCompositor="device"))
    plain, _ = rp.renderPanorama({}, imgs, sizes, _cams(Hs), "planar", 0, dict(opts, planarCompositor="compact", gainCompensation=0))
    _same(compact, dense, "compact vs dense with gain compensation")
    assert not np.array_equal(compact, plain)


# ---- routing ---------------------------------------------------------------------------------------------------------------
def _count_entries(rp, monkeypatch):
    calls = {"aps_planar_composite": 0, "aps_planar_composite_compact": 0}
    for name in calls:
        real = getattr(rp.lib, name)

        def wrapped(*a, _real=real, _name=name):
            calls[_name] += 1
            return _real(*a)

        monkeypatch.setattr(rp.lib, name, wrapped, raising=False)
    return calls


def test_routing_between_the_two_entry_points(rp, monkeypatch):
    imgs, Hs = _three(np.random.default_rng(38))
    many, manyH = _grid_scan(np.random.default_rng(40), 7, 10, 24, 32, overlap=0.5)
    calls = _count_entries(rp, monkeypatch)
    opts = {"blending": "multiband", "pyrLevels": 3}
    dense, _ = rp.renderPanorama({}, imgs, [(60, 90, 3)] * 3, _cams(Hs), "planar", 0, dict(opts))
    assert calls == {"aps_planar_composite": 1, "aps_planar_composite_compact": 0}
    limited, _ = rp.renderPanorama({}, imgs, [(60, 90, 3)] * 3, _cams(Hs), "planar", 0, dict(opts, planarDenseLimitBytes=1))
    assert calls == {"aps_planar_composite": 1, "aps_planar_composite_compact": 1}
    _same(limited, dense, "routed by planarDenseLimitBytes")
    rp.renderPanorama({}, imgs, [(60, 90, 3)] * 3, _cams(Hs), "planar", 0, dict(opts, planarDenseLimitBytes=1 << 40))
    assert calls == {"aps_planar_composite": 2, "aps_planar_composite_compact": 1}
    # 70 views, the way pipeline.stitch hands a planar set over: forcePlanarScan on the input, cameras that carry H2refined only
    rp.renderPanorama({"forcePlanarScan": True}, many, [(24, 32, 3)] * 70, [{"H2refined": H} for H in manyH], "planar", 0, dict(opts))
    assert calls == {"aps_planar_composite": 2, "aps_planar_composite_compact": 2}
    rp.renderPanorama({}, imgs, [(60, 90, 3)] * 3, _cams(Hs), "planar", 0, dict(opts, planarCompositor="host"))
    assert calls == {"aps_planar_composite": 2, "aps_planar_composite_compact": 2}


# ---- one large run ---------------------------------------------------------------------------------------------------------
def test_the_8x8_scan_of_4k_views(gpu, rp, ip):
    """The bench-sized scan: the dense request exceeds the card (an argument-level APS_E_OOM, no launch), the compact one fits,
    covers the canvas and, for the pixel-local 'linear', equals the oracle chain on eight 256 x 256 windows (the chain evaluated
    on the windows as shifted views, over the images whose footprints meet them)."""
    cp, lib = gpu._capi, gpu.lib
    rng = np.random.default_rng(88)
    rows = cols = 8
    h, w = 2160, 3840
    imgs, Hs = _grid_scan(rng, rows, cols, h, w, overlap=0.35)
    n = len(imgs)
    view = _view_of(ip, imgs, Hs)
    Hc, Wc = view["ImageSize"]
    x0, y0, sx, sy = view["XWorldLimits"][0], view["YWorldLimits"][0], view["PixelExtentInWorldX"], view["PixelExtentInWorldY"]
    shapes = [(h, w, 3)] * n
    dense_bytes = rp.planar_composite_bytes(shapes, (Hc, Wc), "multiband", 3)
    compact_bytes = rp.planar_composite_compact_bytes(shapes, (Hc, Wc), Hs, view, "multiband", 3)
    print("canvas %d x %d, dense %.1f GB, compact %.1f GB" % (Wc, Hc, dense_bytes / 1e9, compact_bytes / 1e9))
    assert dense_bytes > 288e9 > compact_bytes

    pim = (C.c_void_p * n)(*[cp.ptr(im) for im in imgs])
    ih, iw, ic = (np.full(n, v, np.int32) for v in (h, w, 3))
    Hm = np.ascontiguousarray(np.stack([np.asarray(T, np.float64).T.reshape(9) for T in Hs]))
    pano = np.zeros((Hc, Wc, 3), np.uint8)
    covered = np.zeros((Hc, Wc), np.uint8)

    def call(entry, mode, cov):
        return entry(C.addressof(pim), cp.ptr(ih), cp.ptr(iw), cp.ptr(ic), n, cp.ptr(Hm), Hc, Wc, x0, y0, sx, sy, mode, 3, 1.0, 0, None,
                     cp.ptr(pano), cp.ptr(cov) if cov is not None else None)

    assert call(lib.aps_planar_composite, cp.APS_BLEND_MULTIBAND, covered) == cp.APS_E_OOM
    assert b"bytes" in lib.aps_last_error() and not pano.any() and not covered.any()
    assert call(lib.aps_planar_composite_compact, cp.APS_BLEND_MULTIBAND, covered) == cp.APS_OK, lib.aps_last_error()
    assert covered.mean() > 0.9 and pano[covered > 0].std() > 10
    assert call(lib.aps_planar_composite_compact, cp.APS_BLEND_LINEAR, None) == cp.APS_OK, lib.aps_last_error()
    rects, _ = rp.planar_footprints([(h, w)] * n, Hs, view)
    wrng = np.random.default_rng(89)
    seen = 0
    for q in range(8):
        r0, c0 = int(wrng.integers(0, Hc - 256)), int(wrng.integers(0, Wc - 256))
        if q == 0:
            r0, c0 = 0, 0
        if q == 1:
            r0, c0 = Hc - 256, Wc - 256
        meet = [k for k in range(n) if rects[k][0] < c0 + 256 and rects[k][2] > c0 and rects[k][1] < r0 + 256 and rects[k][3] > r0]
        if meet:
            ref, _ = _oracle_chain([imgs[k] for k in meet], [Hs[k] for k in meet], 256, 256, x0 + c0 * sx, y0 + r0 * sy, sx, sy, "linear")
        else:
            ref = np.zeros((256, 256, 3), np.uint8)  # a corner no view reaches: the black canvas
        seen += len(meet)
        _same(pano[r0:r0 + 256, c0:c0 + 256], ref, "window %d at (%d, %d), %d images" % (q, r0, c0, len(meet)))
    assert seen >= 8
