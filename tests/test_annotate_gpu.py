"""Device tests of the annotated panorama: aps_annotate_panorama equals tests/annotate_mirror.py byte for byte on small canvases
(one tile, ragged tiles, several tiles), and the operators that produce rgbAnnotation (renderPanorama in the five modes, the
three planar compositors, displayPanorama + cropNsavePanorama, pipeline.stitch) return the mirror's drawing of warped_boxes on
an unchanged panorama."""
import ctypes as C
import os
from importlib import import_module

import numpy as np
import pytest

import annotate_mirror as am

pytestmark = pytest.mark.gpu

CANVASES = [(1, 1), (5, 7), (64, 64), (65, 63), (130, 200)]


def _src(H, W, seed=0):
    return np.random.default_rng(seed + 1000 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _device(gpu, src, polys, anchors, colors, lw=2, where="host"):
    """aps_annotate_panorama through the raw entry.  where: 'host' (both host), 'device' (both resident), 'inplace_host',
    'inplace_device', 'host_to_device', 'device_to_host'.  Returns (result, count, source bytes after the call)."""
    import torch

    capi = gpu._capi
    polys = np.ascontiguousarray(np.asarray(polys, np.float64).reshape(-1, 4, 2))
    anchors = np.ascontiguousarray(np.asarray(anchors, np.float64).reshape(-1, 2))
    colors = np.ascontiguousarray(np.asarray(colors, np.uint8).reshape(-1, 3))
    H, W = src.shape[:2]
    s_dev = where in ("device", "inplace_device", "device_to_host")
    d_dev = where in ("device", "inplace_device", "host_to_device")
    s = torch.from_numpy(src.copy()).cuda() if s_dev else src.copy()
    if where.startswith("inplace"):
        d = s
    else:
        d = torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda") if d_dev else np.full((H, W, 3), 77, np.uint8)
    torch.cuda.synchronize()
    cnt = C.c_int(-1)
    capi.check(capi.lib.aps_annotate_panorama(capi.ptr(s), H, W, capi.ptr(polys), capi.ptr(anchors), capi.ptr(colors), len(polys),
                                              int(lw), capi.ptr(d), C.byref(cnt)))
    capi.check(capi.lib.aps_synchronize())
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a  # noqa: E731
    return host(d), cnt.value, host(s)


def _check(gpu, src, polys, anchors, colors=None, lw=2, where="host"):
    polys = np.asarray(polys, np.float64).reshape(-1, 4, 2)
    if colors is None:
        colors = [[(37 * k + 11) % 256, (91 * k + 200) % 256, (53 * k + 5) % 256] for k in range(len(polys))]
    want, n_want = am.annotate(src, polys, anchors, colors, lw)
    got, n_got, src_after = _device(gpu, src, polys, anchors, colors, lw, where)
    assert n_got == n_want
    bad = np.argwhere((got != want).any(2))
    assert len(bad) == 0, f"{len(bad)} pixels differ from the mirror, first at (row, col) = {tuple(bad[0] + 1)}"
    if not where.startswith("inplace"):
        assert np.array_equal(src_after, src), "the source was written"
    return got


FAR = [[5000, 5000], [5010, 5000], [5010, 5010], [5000, 5010]]  # a valid polygon nowhere near any test canvas


def _polygon_cases(H, W):
    """name -> (polys, anchors); anchors far outside unless the case is about them."""
    off = [[-4000.0, -4000.0]]
    q = lambda *pts: [[list(map(float, p)) for p in pts]]  # noqa: E731
    cases = {
        "inside": q((0.2 * W + 1, 0.2 * H + 1), (0.8 * W, 0.25 * H + 1), (0.75 * W, 0.8 * H), (0.15 * W + 1, 0.7 * H)),
        "straddles_left_top": q((-0.3 * W - 2, -0.2 * H - 1), (0.5 * W, -0.1 * H - 3), (0.6 * W, 0.5 * H), (-0.2 * W - 5, 0.6 * H)),
        "straddles_right_bottom": q((0.5 * W, 0.4 * H), (1.4 * W + 3, 0.5 * H), (1.3 * W + 2, 1.5 * H + 4), (0.4 * W, 1.3 * H + 2)),
        "around_the_canvas": q((-20, -30), (W + 25, -10), (W + 40, H + 33), (-15, H + 12)),
        "all_corners_equal": q(*[(0.5 * W + 0.3, 0.5 * H + 0.7)] * 4),
        "one_zero_length_edge": q((0.3 * W, 0.3 * H), (0.3 * W, 0.3 * H), (0.9 * W, 0.6 * H), (0.2 * W, 0.9 * H)),
        "edge_on_tile_boundary": q((64.5, -3), (64.5, H + 3), (W + 9, 64.5), (-7, 64.5)),
        "edge_on_tile_boundary_integer": q((64, 1), (64, H), (65, H), (65, 1)),
        "odd_sixteenths": q((1 + 3 / 16, 2 + 5 / 16), (W - 7 / 16, 1 + 9 / 16), (W - 1 - 11 / 16, H - 13 / 16), (2 + 15 / 16, H - 1 / 16)),
        # v = m / 16 + 1 / 32: 16 v + 0.5 is the integer m + 1 exactly, the quantiser's tie
        "quantiser_ties": q((2 + 1 / 32, 1 + 3 / 32), (W - 5 / 32, 2 + 7 / 32), (W - 1 - 9 / 32, H - 11 / 32), (1 + 13 / 32, H - 1 - 15 / 32)),
    }
    return {k: (v, off) for k, v in cases.items()}


CASE_NAMES = sorted(_polygon_cases(8, 8))


@pytest.mark.parametrize("H,W", CANVASES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_one_polygon_equals_mirror(gpu, H, W, name):
    polys, anchors = _polygon_cases(H, W)[name]
    _check(gpu, _src(H, W), polys, anchors)


@pytest.mark.parametrize("H,W", CANVASES)
def test_polygon_outside_leaves_the_canvas_alone(gpu, H, W):
    src = _src(H, W)
    for poly in (FAR, [[W + 3, 1], [W + 40, 1], [W + 40, H], [W + 3, H]], [[-50, -50], [-2, -50], [-2, -2], [-50, -2]]):
        got = _check(gpu, src, [poly], [[-4000, -4000]])
        assert np.array_equal(got, src)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 2.0 ** 20 + 1, -(2.0 ** 20) - 1])
def test_invalid_polygons_are_skipped_and_the_numbering_closes_up(gpu, bad):
    H, W = 65, 63
    src = _src(H, W)
    polys = np.array([[[5, 5], [40, 8], [38, 30], [6, 28]], [[10, 20], [50, 22], [48, 60], [12, 58]],
                      [[20, 3], [60, 5], [58, 40], [22, 38]]], np.float64)
    polys[1, 2, 1] = bad
    anchors = [[2, 2], [30, 30], [20, 34]]
    got = _check(gpu, src, polys, anchors)
    two, n_two, _ = _device(gpu, src, polys[[0, 2]], [anchors[0], anchors[2]], [[11, 200, 5], [85, 126, 111]])
    assert n_two == 2 and np.array_equal(got, two)  # polygon 3 carries label 2 and its own colour
    # the largest valid coordinate is still drawn (and clipped)
    polys[1, 2, 1] = np.sign(bad) * 2.0 ** 20 if np.isfinite(bad) else 7.0
    _check(gpu, src, polys, anchors)


def test_three_overlapping_polygons_highest_index_wins(gpu):
    H, W = 130, 200
    polys = [[[10, 10], [150, 10], [150, 100], [10, 100]], [[10, 10], [150, 10], [120, 120], [30, 90]],
             [[10, 10], [150, 10], [190, 60], [5, 125]]]
    colors = [[255, 0, 0], [0, 255, 0], [0, 0, 255]]
    got = _check(gpu, _src(H, W), polys, [[-4000, -4000]] * 3, colors)
    assert (got[9, 20:140] == (0, 0, 255)).all()  # the shared top edge carries the last colour


def test_120_tiny_polygons_have_one_two_and_three_digit_labels(gpu):
    H, W = 130, 200
    rng = np.random.default_rng(5)
    polys, anchors = [], []
    for k in range(120):
        x, y = 4 + 16 * (k % 12) + rng.uniform(0, 1), 3 + 12.5 * (k // 12) + rng.uniform(0, 1)
        polys.append([[x, y], [x + 6.3, y + 0.4], [x + 5.9, y + 5.2], [x - 0.2, y + 4.8]])
        anchors.append([x - 2.6, y + 1.4])
    _check(gpu, _src(H, W), polys, anchors)


@pytest.mark.parametrize("H,W", CANVASES)
def test_labels_clipped_at_every_border_and_overlapping(gpu, H, W):
    src = _src(H, W)
    for ax, ay in ((-6.4, 0.4 * H), (W - 9.5, 0.3 * H), (0.3 * W, -11.5), (0.4 * W, H - 7.49), (W + 0.49, 1), (1, H + 0.5),
                   (-40.2, -30.2), (1, 1), (0.51, 0.5)):
        _check(gpu, src, [FAR], [[ax, ay]])
    # two labels that overlap blend in label order (1 under 2), and twelve give two-digit boxes over one-digit ones
    _check(gpu, src, [FAR] * 2, [[0.2 * W, 0.2 * H], [0.2 * W + 7, 0.2 * H + 9]])
    _check(gpu, src, [FAR] * 12, [[0.1 * W + 3 * k, 0.1 * H + 2 * k] for k in range(12)])
    # a label whose anchor is not a valid coordinate is not drawn; its polygon still counts
    got = _check(gpu, src, [FAR] * 2, [[np.nan, 3], [2, np.inf]])
    assert np.array_equal(got, src)


@pytest.mark.parametrize("where", ["host", "device", "inplace_host", "inplace_device", "host_to_device", "device_to_host"])
@pytest.mark.parametrize("lw", [1, 2, 5])
def test_pointers_and_line_widths(gpu, where, lw):
    H, W = 130, 200
    polys = [[[12.3, 9.1], [180.6, 20.2], [170.9, 118.4], [25.5, 101.7]], [[-30, 64.5], [90, -12], [230, 70], [100, 150]]]
    _check(gpu, _src(H, W), polys, [[60, 40], [71, 52]], lw=lw, where=where)


def test_no_polygons_is_a_copy(gpu):
    src = _src(65, 63)
    got, n, _ = _device(gpu, src, np.zeros((0, 4, 2)), np.zeros((0, 2)), np.zeros((0, 3), np.uint8))
    assert n == 0 and np.array_equal(got, src)


def test_widest_line(gpu):
    _check(gpu, _src(130, 200), [[[40, 40], [160, 50], [150, 100], [45, 95]]], [[-4000, -4000]], lw=64)


# ---- through the operators ---------------------------------------------------------------------------------------------------
VH, VW, VF = 96, 128, 150.0


@pytest.fixture(scope="module")
def mods(gpu):
    return {k: import_module(gpu.__name__ + "." + k) for k in ("renderPanorama", "synth", "pipeline", "imageProcessing")}


@pytest.fixture(scope="module")
def views(mods):
    import torch

    synth = mods["synth"]
    K = np.array([[VF, 0, (VW + 1) / 2], [0, VF, (VH + 1) / 2], [0, 0, 1.0]])
    cams = [{"K": K, "R": synth.rot_yaw_pitch(y, p, r)} for y, p, r in ((-0.35, 0.03, 0.02), (0.0, -0.04, -0.03), (0.33, 0.05, 0.04))]
    imgs = [synth.render_view(c, VH, VW, 7, "cuda").cpu().numpy() for c in cams]
    torch.cuda.synchronize()
    return imgs, cams


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


FLAGS = {"showPanoramaImgsNums": True, "showCropBoundingBox": True}


@pytest.mark.parametrize("device_out", [False, True])
@pytest.mark.parametrize("mode", ["planar", "cylindrical", "spherical", "equirectangular", "stereographic"])
def test_render_panorama_annotation(mods, views, mode, device_out):
    rp = mods["renderPanorama"]
    imgs, cams = views
    sizes = [(VH, VW, 3)] * 3
    opts = {"anglePower": 2, "blending": "linear", "tile": (64, 64), "cropBorder": True}
    plain, none = rp.renderPanorama({}, imgs, sizes, cams, mode, 1, opts, device_out=device_out)
    assert none is None
    pano, ann, _, geo = rp.renderPanorama({}, imgs, sizes, cams, mode, 1, dict(opts, **FLAGS), device_out=device_out,
                                          return_covered=True)
    assert ann is not None and hasattr(ann, "is_cuda") == device_out and (not device_out or ann.is_cuda)
    plain, pano, ann = _np(plain), _np(pano), _np(ann)
    assert np.array_equal(plain, pano), "the panorama changed with the flags"
    assert ann.shape == pano.shape and ann.dtype == np.uint8
    # the boxes: warped_boxes on the uncropped canvas, shifted by the crop origin (renderPanorama.m:434-455)
    full, _ = rp.renderPanorama({}, imgs, sizes, cams, mode, 1, dict(opts, cropBorder=False))
    _, rect, _ = rp.cropNonzeroBbox(full, "black")
    polys, centers = rp.warped_boxes(cams, sizes, geo)
    shift = np.array([rect[2] - 1, rect[0] - 1], np.float64)
    polys, centers = polys - shift, centers - shift
    want, n = am.annotate(pano, polys, centers, rp.vivid_palette(3), 2)
    assert n == 3 and np.array_equal(ann, want)
    changed = (ann != pano).any(2)
    assert changed.any() and not (changed & ~am.allowed_change_mask(pano.shape[0], pano.shape[1], polys, centers, 2)).any()
    # an image corner lands on the canvas pixel that samples it: the outline hugs the covered region of the panorama
    outline = np.zeros(changed.shape, bool)
    for p in polys:
        for e in range(4):
            outline |= am.edge_mask(pano.shape[0], pano.shape[1], *[(am.quant(x), am.quant(y)) for x, y in (p[e], p[(e + 1) % 4])], 2)
    covered = (pano > 0).any(2)
    grown = np.zeros_like(covered)
    for dy in (-3, 0, 3):
        for dx in (-3, 0, 3):
            grown |= np.roll(np.roll(covered, dy, 0), dx, 1)
    assert (outline & grown).sum() >= 0.9 * outline.sum()
    # the caller's colours
    mine = np.array([[1, 2, 3], [250, 251, 252], [9, 99, 199]], np.uint8)
    _, ann2 = rp.renderPanorama({}, imgs, sizes, cams, mode, 1, dict(opts, annotationColors=mine, **FLAGS))
    assert np.array_equal(_np(ann2), am.annotate(pano, polys, centers, mine, 2)[0])


def _scan(mods):
    synth = mods["synth"]
    K = np.array([[400.0, 0, 64.5], [0, 400.0, 48.5], [0, 0, 1.0]])
    base = synth.render_view({"K": K, "R": np.eye(3)}, 96, 128, 3, "cuda").cpu().numpy()
    imgs = [base, np.ascontiguousarray(base[:, ::-1]), np.ascontiguousarray(base[::-1])]
    Hs = [np.eye(3), np.array([[1.02, 0.03, 70.3], [-0.02, 0.99, 11.6], [1e-5, -2e-5, 1.0]]),
          np.array([[0.97, -0.05, 31.2], [0.04, 1.01, 60.9], [-1e-5, 1e-5, 1.0]])]
    return imgs, [{"H2refined": H, "noRotation": 1} for H in Hs]


@pytest.mark.parametrize("device_out", [False, True])
@pytest.mark.parametrize("compositor", ["device", "compact", "host"])
def test_planar_scan_annotation(mods, compositor, device_out):
    rp, ip = mods["renderPanorama"], mods["imageProcessing"]
    imgs, cams = _scan(mods)
    sizes = [im.shape for im in imgs]
    opts = {"blending": "linear", "planarCompositor": compositor}
    plain, none = rp.renderPanorama({}, imgs, sizes, cams, "planar", 0, opts, device_out=device_out)
    pano, ann = rp.renderPanorama({}, imgs, sizes, cams, "planar", 0, dict(opts, **FLAGS), device_out=device_out)
    assert none is None and ann is not None and hasattr(ann, "is_cuda") == device_out
    plain, pano, ann = _np(plain), _np(pano), _np(ann)
    assert np.array_equal(plain, pano)
    # renderPanorama.m:738-742: corners through transformPointsForwardScratch, minus the world limits of the canvas
    tforms = [c["H2refined"] for c in cams]
    lims = [ip.outputLimitsScratch(T, (1, 128), (1, 96)) for T in tforms]
    x0, y0 = min(l[0][0] for l in lims), min(l[1][0] for l in lims)
    polys, centers = [], []
    for T in tforms:
        q = np.asarray(ip.transformPointsForwardScratch(T, np.array([[1, 1], [128, 1], [128, 96], [1, 96], [1, 1]], np.float64))) - [x0, y0]
        polys.append(q[:4])
        centers.append(q.mean(0))
    want, n = am.annotate(pano, polys, centers, rp.vivid_palette(3), 2)
    assert n == 3 and np.array_equal(ann, want)
    changed = (ann != pano).any(2)
    assert changed.any() and not (changed & ~am.allowed_change_mask(pano.shape[0], pano.shape[1], polys, centers, 2)).any()


def test_display_then_crop_n_save_writes_the_annotated_files(mods, views, tmp_path):
    from PIL import Image

    rp, ip = mods["renderPanorama"], mods["imageProcessing"]
    imgs, cams = views
    # the set's images sit at positions 2, 4, 5 of a longer list (1-based panoIndices), the reference image is the 2nd member
    all_imgs = [imgs[0] * 0, imgs[0], imgs[1] * 0, imgs[1], imgs[2]]
    all_sizes = np.array([[VH, VW, 3]] * 5)
    inp = {"panorama2DisplaynSave": ["spherical", "planar"], "canvasColor": "black", "gainCompensation": 0, "sigmaN": 10.0,
           "sigmag": 0.1, "bands": 2, "blending": "linear", "MBBsigma": 1.0, "tile": (64, 64), "transformationType": "projective",
           "imageWrite": True, "imageSaveFolder": str(tmp_path / "out"), "cropPanorama": 0, **FLAGS}
    store = rp.displayPanorama(inp, [cams, []], [2, 1], all_imgs, all_sizes, [[2, 4, 5], []], device_out=True)
    assert len(store) == 2 and sorted(store[0]) == ["planar", "spherical"] and store[1] == {}
    for proj in ("spherical", "planar"):
        pano, ann = store[0][proj]
        assert pano.is_cuda and ann.is_cuda and pano.shape == ann.shape
        direct, _ = rp.renderPanorama(inp, imgs, [(VH, VW, 3)] * 3, cams, proj, 1,
                                      {"anglePower": 2, "blending": "linear", "tile": (64, 64), "cropBorder": True})
        assert np.array_equal(_np(pano), _np(direct))
    one = rp.displayPanorama(dict(inp, panorama2DisplaynSave="spherical"), [cams], [2], imgs, all_sizes[:3], [[1, 2, 3]])
    assert sorted(one[0]) == ["spherical"] and np.array_equal(one[0]["spherical"][1], _np(store[0]["spherical"][1]))
    ip.cropNsavePanorama(inp, store, 1, ["scene"])
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == sorted(f"{p}{tag}_projective_1_1_scene.png" for p in ("planar", "spherical") for tag in ("", "_annotated"))
    for proj in ("spherical", "planar"):
        for tag, slot in (("", 0), ("_annotated", 1)):
            px = np.asarray(Image.open(tmp_path / "out" / f"{proj}{tag}_projective_1_1_scene.png"))
            assert np.array_equal(px, _np(store[0][proj][slot]))
    # without the flags: slot 1 is None and no annotated file is written
    off = dict(inp, showCropBoundingBox=False, imageSaveFolder=str(tmp_path / "off"))
    store_off = rp.displayPanorama(off, [cams], [2], imgs, all_sizes[:3], [[1, 2, 3]])
    assert store_off[0]["planar"][1] is None and np.array_equal(store_off[0]["planar"][0], _np(store[0]["planar"][0]))
    ip.cropNsavePanorama(off, store_off, 1, ["scene"])
    assert sorted(os.listdir(tmp_path / "off")) == ["planar_projective_1_1_scene.png", "spherical_projective_1_1_scene.png"]


def test_stitch_fills_info_annotated(mods):
    import torch

    synth, pl, rp = mods["synth"], mods["pipeline"], mods["renderPanorama"]
    w, h, f = 480, 360, 700.0
    cams = synth.grid_cameras(2, 1, w, h, f, 2 * np.arctan(w / (2 * f)) * 0.5, 0.0, 1.0, 11)
    imgs = [synth.render_view(c, h, w, 11, "cuda", finest_px=1.5) for c in cams]
    torch.cuda.synchronize()
    inp = pl.default_input(bands=2, resizeImage=0)
    panos, info = pl.stitch(inp, imgs, Ks=[c["K"] for c in cams], tile=(256, 256))
    assert "annotated" not in info and len(panos) == 1
    panos2, info2 = pl.stitch(dict(inp, **FLAGS), imgs, Ks=[c["K"] for c in cams], tile=(256, 256))
    assert len(info2["annotated"]) == len(panos2) == 1
    pano, ann = _np(panos2[0]), _np(info2["annotated"][0])
    assert np.array_equal(pano, _np(panos[0])) and ann.shape == pano.shape
    changed = (ann != pano).any(2)
    assert 0 < changed.mean() < 0.2
    # two outlines in the palette's colours, two labels
    pal = rp.vivid_palette(2)
    assert all(((ann == c).all(2) & changed).sum() > 200 for c in pal)
    assert ((ann == 255).all(2) & changed).sum() > 20
