"""The device-resident planar-scan compositor (aps_planar_composite) against the host-orchestrated path of the same
commit (opts['planarCompositor'] = 'host': 2N imageWarp calls, numpy, the blend operators - itself tested against the
oracle in test_render_gpu.py / test_config0_gpu.py).  The condition is byte identity of the uint8 panorama."""
from importlib import import_module

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rp(gpu):
    return import_module(gpu.__name__ + ".renderPanorama")


@pytest.fixture(scope="module")
def ip(gpu):
    return import_module(gpu.__name__ + ".imageProcessing")


def _both(rp, imgs, Hs, opts, gains=None):
    cams = [{"H2refined": np.asarray(H, np.float64), "noRotation": 1} for H in Hs]
    sizes = [tuple(np.asarray(im).shape) for im in imgs]
    dev, _ = rp.renderPanorama({}, imgs, sizes, cams, "planar", 0, dict(opts), gains=gains)
    host, _ = rp.renderPanorama({}, imgs, sizes, cams, "planar", 0, dict(opts, planarCompositor="host"), gains=gains)
    return dev, host


def _same(dev, host):
    assert dev.dtype == np.uint8 and dev.shape == host.shape, (dev.shape, host.shape)
    assert np.array_equal(dev, host), "%d bytes differ" % int((dev != host).sum())


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


@pytest.mark.parametrize("canvas", ["black", "white"])
@pytest.mark.parametrize("blending,levels,sigma", [("none", 3, 1.0), ("linear", 3, 1.0), ("multiband", 1, 1.0),
                                                   ("multiband", 3, 1.0), ("multiband", 5, 1.0), ("multiband", 3, 1.6),
                                                   ("multiband", 5, 1.6), ("multiband", 1, 1.6)])
def test_three_small_views_are_byte_identical(rp, blending, levels, sigma, canvas):
    imgs, Hs = _three(np.random.default_rng(21))
    dev, host = _both(rp, imgs, Hs, {"blending": blending, "pyrLevels": levels, "pyrSigma": sigma, "canvasColor": canvas})
    _same(dev, host)
    assert (dev != (255 if canvas == "white" else 0)).mean() > 0.5


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_twelve_view_scan_is_byte_identical(rp, blending):
    imgs, Hs = _grid_scan(np.random.default_rng(31), 3, 4, 480, 640)
    dev, host = _both(rp, imgs, Hs, {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0})
    _same(dev, host)
    assert dev.shape[0] > 2 * 480 and dev.shape[1] > 2.5 * 640


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_twenty_views_take_the_many_layer_branch(rp, blending):
    imgs, Hs = _grid_scan(np.random.default_rng(32), 4, 5, 48, 64, overlap=0.5)
    assert len(imgs) == 20
    dev, host = _both(rp, imgs, Hs, {"blending": blending, "pyrLevels": 4, "pyrSigma": 1.0, "canvasColor": "white"})
    _same(dev, host)


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_views_of_different_sizes(rp, blending):
    rng = np.random.default_rng(33)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((60, 90), (45, 120), (77, 51))]
    Hs = [np.eye(3), np.array([[1.02, 0.03, 50.0], [-0.02, 0.97, 10.0], [2e-5, 1e-5, 1.0]]),
          np.array([[0.9, -0.1, 20.5], [0.1, 0.9, 40.25], [0, -3e-5, 1.0]])]
    _same(*_both(rp, imgs, Hs, {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0}))


@pytest.mark.parametrize("shape", [(60, 90, 1), (60, 90)])
@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_single_channel_set(rp, blending, shape):
    rng = np.random.default_rng(34)
    imgs3, Hs = _three(rng)
    imgs = [np.ascontiguousarray(im[..., :1]).reshape(shape) for im in imgs3]
    _same(*_both(rp, imgs, Hs, {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0}))


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_explicit_gains(rp, blending):
    imgs, Hs = _three(np.random.default_rng(35))
    g = np.array([[0.8, 0.9, 1.0], [1.25, 1.1, 0.95], [1.0, 0.7, 1.3]], np.float32)
    dev, host = _both(rp, imgs, Hs, {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0}, gains=g)
    _same(dev, host)
    plain, _ = _both(rp, imgs, Hs, {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0})
    assert not np.array_equal(dev, plain)


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_horizon_crossing_homography(rp, ip, blending):
    """The denominator of the second homography changes sign inside its image: whole-canvas footprint.  The canvas is given
    (planar_composite / _planar_host on one view), as the corner maps of such an image do not bound it."""
    rng = np.random.default_rng(36)
    imgs = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in range(2)]
    T = np.array([[1.0, 0.02, 30.0], [-0.01, 1.0, 5.0], [1.0 / 40.0, 0.0, -0.8]])  # d = 0 at x = 32
    Hs = [np.eye(3), T]
    view = ip.imref2dScratch((150, 220), (-120.5, 99.5), (-80.5, 69.5))
    _, whole = rp.planar_footprints([(48, 64)] * 2, Hs, view)
    assert list(whole) == [False, True]
    o = {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0, "canvasColor": "black"}
    dev = rp.planar_composite(imgs, Hs, view, o)
    host = rp._planar_host(imgs, Hs, view, o)
    _same(dev, host)
    assert dev.any()


@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
def test_footprint_culling_changes_no_byte(rp, monkeypatch, blending):
    imgs, Hs = _grid_scan(np.random.default_rng(37), 2, 3, 96, 128)
    opts = {"blending": blending, "pyrLevels": 4, "pyrSigma": 1.0}
    monkeypatch.delenv("APS_PLANAR_NO_CULL", raising=False)
    a, host = _both(rp, imgs, Hs, opts)
    monkeypatch.setenv("APS_PLANAR_NO_CULL", "1")
    b, _ = _both(rp, imgs, Hs, opts)
    _same(a, b)
    _same(a, host)


def test_host_switches_select_the_host_path(rp, monkeypatch):
    imgs, Hs = _three(np.random.default_rng(38))
    cams = [{"H2refined": H, "noRotation": 1} for H in Hs]
    calls = []
    real = rp.planar_composite
    monkeypatch.setattr(rp, "planar_composite", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    rp.renderPanorama({}, imgs, [(60, 90, 3)] * 3, cams, "planar", 0, {"blending": "linear"})
    assert len(calls) == 1
    rp.renderPanorama({}, imgs, [(60, 90, 3)] * 3, cams, "planar", 0, {"blending": "linear", "planarCompositor": "host"})
    monkeypatch.setenv("APS_PLANAR_HOST", "1")
    rp.renderPanorama({}, imgs, [(60, 90, 3)] * 3, cams, "planar", 0, {"blending": "linear"})
    assert len(calls) == 1


@pytest.mark.parametrize("blending", ["multiband", "none"])
def test_resident_tensors_in_and_out(rp, blending):
    import torch

    imgs, Hs = _three(np.random.default_rng(39))
    cams = [{"H2refined": H, "noRotation": 1} for H in Hs]
    opts = {"blending": blending, "pyrLevels": 3, "pyrSigma": 1.0}
    ref, _ = rp.renderPanorama({}, imgs, [(60, 90, 3)] * 3, cams, "planar", 0, dict(opts, planarCompositor="host"))
    dimgs = [torch.from_numpy(im).cuda() for im in imgs]
    out, _ = rp.renderPanorama({}, dimgs, [(60, 90, 3)] * 3, cams, "planar", 0, opts, device_out=True)
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), ref)


# ---- gains -----------------------------------------------------------------------------------------------------------------
W, H, F = 1024, 768, 1100.0


@pytest.fixture(scope="module")
def dark_pair(gpu):
    """The darkened configs[0] pair of test_config0_gpu.py: two 1024 x 768 views, the second multiplied by 0.8."""
    import torch

    synth = import_module(gpu.__name__ + ".synth")
    views, cams = synth.make_scene(2, 1, W, H, F, 0.55, seed=77, device="cuda", finest_px=4.0)
    torch.cuda.synchronize()
    imgs = [v.cpu().numpy() for v in views]
    dark = np.clip(np.floor(imgs[1].astype(np.float32) * 0.8 + 0.5), 0, 255).astype(np.uint8)
    K = cams[0]["K"]
    Ht = K @ cams[0]["R"] @ cams[1]["R"].T @ np.linalg.inv(K)
    return [imgs[0], dark], [np.eye(3), Ht / Ht[2, 2]]


def test_gain_statistics_from_the_resident_layers(gpu, rp, ip, dark_pair):
    gc = import_module(gpu.__name__ + ".gainCompensation")
    views, tforms = dark_pair
    lims = [ip.outputLimitsScratch(T, (1, W), (1, H)) for T in tforms]
    xMin, xMax = min(l[0][0] for l in lims), max(l[0][1] for l in lims)
    yMin, yMax = min(l[1][0] for l in lims), max(l[1][1] for l in lims)
    width, height = int(np.floor(xMax - xMin + 0.5)), int(np.floor(yMax - yMin + 0.5))
    view = ip.imref2dScratch((height, width), (xMin, xMax), (yMin, yMax))
    Iw, Ww, _, _, _ = rp.pureNonRotationalImagesToCanvas(views, tforms, view, rp.warpWeights(views), {})
    for ds in (4, 3, 1):
        N, sI, sJ = rp.planar_gain_stats(views, tforms, view, ds)
        hN, hI, hJ = gc.gain_overlap_stats_warped(Iw, Ww, ds)
        assert np.array_equal(N, hN) and N[0, 1] > 10000 and N.sum() == N[0, 1]
        assert np.allclose(sI, hI, rtol=1e-12, atol=0) and np.allclose(sJ, hJ, rtol=1e-12, atol=0)
    # opts['gainCompensation'] through the device path = explicit gains from gainCompensationH on the host canvases
    g = gc.gainCompensationH(Iw, Ww, {"sigmag": 10.0})
    pcams = [{"H2refined": T, "noRotation": 1} for T in tforms]
    for blending in ("linear", "multiband"):
        opts = {"blending": blending, "canvasColor": "black", "gainCompensation": 1, "sigmag": 10.0}
        auto, _ = rp.renderPanorama({}, views, [(H, W, 3)] * 2, pcams, "planar", 0, opts)
        given, _ = rp.renderPanorama({}, views, [(H, W, 3)] * 2, pcams, "planar", 0, {"blending": blending}, gains=g)
        host, _ = rp.renderPanorama({}, views, [(H, W, 3)] * 2, pcams, "planar", 0, dict(opts, planarCompositor="host"))
        none, _ = rp.renderPanorama({}, views, [(H, W, 3)] * 2, pcams, "planar", 0, {"blending": blending})
        assert np.array_equal(auto, given) and np.array_equal(auto, host) and not np.array_equal(auto, none)


def test_argument_errors_reach_no_launch(gpu, rp, ip):
    """With a device present the same refusals as on the host: status and message, and the output stays untouched."""
    import ctypes as C

    cp, lib = gpu._capi, gpu.lib
    img = np.full((10, 12, 3), 200, np.uint8)
    out = np.full((20, 30, 3), 7, np.uint8)

    def call(n=1, H=np.eye(3), levels=3, sigma=1.0, images=True):
        m = max(n, 1)
        pim = (C.c_void_p * m)(*[cp.ptr(img)] * m)
        ih, iw, ic = (np.full(m, v, np.int32) for v in (10, 12, 3))
        Hs = np.ascontiguousarray(np.stack([np.asarray(H, np.float64).T.reshape(9)] * m))
        return lib.aps_planar_composite(C.addressof(pim) if images else None, cp.ptr(ih), cp.ptr(iw), cp.ptr(ic), n, cp.ptr(Hs), 20,
                                        30, 0.5, 0.5, 1.0, 1.0, cp.APS_BLEND_MULTIBAND, levels, sigma, 0, None, cp.ptr(out), None)

    for kw, code in [(dict(images=False), cp.APS_E_ARG), (dict(n=0), cp.APS_E_ARG), (dict(n=65), cp.APS_E_DIM),
                     (dict(levels=0), cp.APS_E_ARG), (dict(sigma=0.0), cp.APS_E_ARG),
                     (dict(H=np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])), cp.APS_E_ARG)]:
        assert call(**kw) == code and len(lib.aps_last_error()) > 0, kw
        assert (out == 7).all()
    assert call() == 0 and (out != 7).any()
