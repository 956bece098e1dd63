"""Device tests of the match and keypoint plots: showMatchedFeatures, showKeypoints, matchPlots and pipeline.stitch under
input.showKeypointsPlot return the pictures tests/marks_mirror.py draws, byte for byte."""
from importlib import import_module

import numpy as np
import pytest

import marks_mirror as mm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(gpu):
    return {k: import_module(gpu.__name__ + "." + k) for k in ("imageMatching", "featureMatching", "imageProcessing", "synth", "pipeline")}


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same(got, want):
    got = _np(got)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere((got != want).any(2))
    assert len(bad) == 0, f"{len(bad)} pixels differ from the mirror, first at (row, col) = {tuple(bad[0] + 1)}"


@pytest.fixture(scope="module")
def pair():
    """A 40 x 50 and a 70 x 30 image with 25 matches: points on every border, one row with a NaN."""
    rng = np.random.default_rng(12)
    I1, I2 = _img(40, 50, 1), _img(70, 30, 2)
    p1 = np.stack([rng.uniform(1, 50, 25), rng.uniform(1, 40, 25)], axis=1)
    p2 = np.stack([rng.uniform(1, 30, 25), rng.uniform(1, 70, 25)], axis=1)
    p1[:4] = [[1, 1], [50, 40], [1, 40], [50, 1]]       # the corners of image 1
    p2[:4] = [[30, 70], [1, 1], [30, 1], [1, 70]]       # and of image 2
    p1[4:6] = [[25.5, 1], [50, 20.5]]                   # on the top and right borders, on half-pixel ties
    p2[4:6] = [[1, 35.5], [15.5, 70]]
    p1[9, 1] = np.nan
    return I1, I2, p1, p2


@pytest.mark.parametrize("kind", ["numpy", "cuda", "mixed"])
def test_show_matched_features_equals_mirror(mods, pair, kind):
    import torch

    im = mods["imageMatching"]
    I1, I2, p1, p2 = pair
    want = mm.match_plot(I1, I2, p1, p2)
    assert (want != mm.montage_pair(I1, I2)).any()
    a = torch.from_numpy(I1).cuda() if kind != "numpy" else I1
    b = torch.from_numpy(I2).cuda() if kind == "cuda" else I2
    got = im.showMatchedFeatures(a, b, p1, p2)
    assert (kind == "numpy") == isinstance(got, np.ndarray) and (kind == "numpy" or got.is_cuda)
    _same(got, want)
    assert np.array_equal(_np(a), I1) and np.array_equal(_np(b), I2)


def test_show_matched_features_styles_and_edge_cases(mods, pair):
    im = mods["imageMatching"]
    I1, I2, p1, p2 = pair
    style = dict(markerRadius=5.5, lineWidth=2, colors=((0, 0, 255), (255, 0, 255), (255, 255, 255)))
    _same(im.showMatchedFeatures(I1, I2, p1, p2, "montage", **style), mm.match_plot(I1, I2, p1, p2, **style))
    _same(im.showMatchedFeatures(I2, I1, p2, p1, method="Montage"), mm.match_plot(I2, I1, p2, p1))  # the taller image first
    _same(im.showMatchedFeatures(I1, I2, np.zeros((0, 2)), np.zeros((0, 2))), mm.montage_pair(I1, I2))  # no matches: the montage
    _same(im.showMatchedFeatures(I1[:, :, 0], I2[:, :, :1], p1, p2), mm.match_plot(I1[:, :, 0], I2[:, :, :1], p1, p2))
    with pytest.raises(ValueError):
        im.showMatchedFeatures(I1, I2, p1, p2, method="falsecolor")


def test_show_keypoints_equals_mirror(mods):
    import torch

    fm = mods["featureMatching"]
    rng = np.random.default_rng(21)
    img = _img(65, 130, 5)
    pts = np.stack([rng.uniform(-3, 134, 30), rng.uniform(-3, 69, 30)], axis=1)
    scales = rng.uniform(0.3, 25, 30)
    scales[3], scales[4] = 5000.0, 0.0  # above 4096: skipped; 0: a dot
    angles = rng.uniform(-200, 400, 30)
    angles[:4] = [0, 90, 180, 270]
    for args, kw in (((pts,), {}), ((pts, scales), {}), ((pts, None, angles), dict(markerRadius=6)),
                     ((pts, scales, angles), dict(color=(255, 128, 0), lineWidth=2))):
        want, _ = mm.draw_marks(img, mm.keypoint_marks(*args, **kw))
        _same(fm.showKeypoints(img, *args, **kw), want)
    got = fm.showKeypoints(torch.from_numpy(img).cuda(), torch.from_numpy(pts).cuda(), torch.from_numpy(scales), angles)
    assert got.is_cuda
    _same(got, mm.draw_marks(img, mm.keypoint_marks(pts, scales, angles))[0])
    # the ring of 5000 px is skipped by the contract; its 5000 px long orientation segment is a valid mark
    table = fm.keypoint_marks(pts, scales, angles)
    assert mods["imageProcessing"].draw_marks(img, table)[1] == mm.draw_marks(img, mm.keypoint_marks(pts, scales, angles))[1] == 2 * 30 - 1
    assert np.array_equal(_np(fm.showKeypoints(img, np.zeros((0, 2)))), img)


def _lists(rng, n_i, n_j, k):
    return np.stack([rng.integers(1, n_i + 1, k), rng.integers(1, n_j + 1, k)], axis=1)


@pytest.mark.parametrize("resident", [False, True])
def test_match_plots_on_three_small_images(mods, resident):
    import torch

    im = mods["imageMatching"]
    rng = np.random.default_rng(31)
    imgs = [_img(40, 50, 1), _img(70, 30, 2), _img(33, 64, 3)]
    kps = [np.stack([rng.uniform(1, im_.shape[1], 20), rng.uniform(1, im_.shape[0], 20)], axis=1) for im_ in imgs]
    pairs = [(0, 1), (0, 2), (1, 2)]
    putative = {p: _lists(rng, 20, 20, 12) for p in pairs}
    inliers = {p: putative[p][::3] for p in pairs}
    inliers[(0, 2)] = np.zeros((0, 2), np.int64)  # a pair whose model was not found: no inlier marks
    given = [torch.from_numpy(a).cuda() for a in imgs] if resident else imgs
    plots = im.matchPlots(given, kps, putative, inliers, pairs)
    assert list(plots) == pairs
    for (i, j) in pairs:
        plot = plots[(i, j)]
        assert sorted(plot) == ["inliers", "original", "putative"]
        assert all((hasattr(v, "is_cuda") and v.is_cuda) == resident for v in plot.values())
        _same(plot["original"], mm.montage_pair(imgs[i], imgs[j]))
        for name, lists in (("putative", putative), ("inliers", inliers)):
            mt = lists[(i, j)]
            _same(plot[name], mm.match_plot(imgs[i], imgs[j], kps[i][mt[:, 0] - 1], kps[j][mt[:, 1] - 1]))
    _same(plots[(0, 2)]["inliers"], mm.montage_pair(imgs[0], imgs[2]))
    # lists given in the order of the pairs, a subset of the pairs, a style
    sub = im.matchPlots(imgs, kps, [putative[(1, 2)]], [inliers[(1, 2)]], [(1, 2)], markerRadius=4, lineWidth=2)
    mt = putative[(1, 2)]
    _same(sub[(1, 2)]["putative"], mm.match_plot(imgs[1], imgs[2], kps[1][mt[:, 0] - 1], kps[2][mt[:, 1] - 1], markerRadius=4, lineWidth=2))
    with pytest.raises(ValueError, match="Match indices exceed"):
        im.matchPlots(imgs, kps, [np.array([[21, 1]])], [np.zeros((0, 2))], [(0, 1)])


# ---- through pipeline.stitch: the scene test_stitch_fills_info_annotated of tests/test_annotate_gpu.py builds -----------------
@pytest.fixture(scope="module")
def scene(mods):
    import torch

    synth, pl = mods["synth"], mods["pipeline"]
    w, h, f = 480, 360, 700.0
    cams = synth.grid_cameras(2, 1, w, h, f, 2 * np.arctan(w / (2 * f)) * 0.5, 0.0, 1.0, 11)
    imgs = [synth.render_view(c, h, w, 11, "cuda", finest_px=1.5) for c in cams]
    torch.cuda.synchronize()
    inp = pl.default_input(bands=2, resizeImage=0)
    kw = dict(Ks=[c["K"] for c in cams], tile=(256, 256))
    panos, info = pl.stitch(inp, imgs, **kw)
    panos_f, info_f = pl.stitch(dict(inp, showKeypointsPlot=1), imgs, **kw)
    return imgs, inp, kw, panos, info, panos_f, info_f


def _check_stitch_plots(info, resident):
    host_imgs = [_np(a) for a in info["images_processed"]]
    kps = [_np(k)[:, :2] for k in info["keypoints"]]
    for (i, j), plot in info["match_plots"].items():
        lists = info["match_plot_lists"][(i, j)]
        assert sorted(plot) == ["inliers", "original", "putative"]
        assert all((hasattr(v, "is_cuda") and v.is_cuda) == resident and (resident or isinstance(v, np.ndarray)) for v in plot.values())
        _same(plot["original"], mm.montage_pair(host_imgs[i], host_imgs[j]))
        for name in ("putative", "inliers"):
            mt = np.asarray(lists[name], np.int64)
            _same(plot[name], mm.match_plot(host_imgs[i], host_imgs[j], kps[i][mt[:, 0] - 1], kps[j][mt[:, 1] - 1]))


def test_stitch_fills_match_plots(mods, scene):
    imgs, inp, kw, panos, info, panos_f, info_f = scene
    assert "match_plots" not in info and "match_plot_lists" not in info and "keypoints" not in info
    assert "match_plots" not in mods["pipeline"].DEFAULT_INPUT and "showKeypointsPlot" not in mods["pipeline"].DEFAULT_INPUT
    # the panoramas and every other entry of info are the same with and without the flag
    assert len(panos) == len(panos_f) == 1 and np.array_equal(_np(panos[0]), _np(panos_f[0]))
    assert sorted(set(info_f) - set(info)) == ["keypoints", "match_plot_lists", "match_plots"] and set(info) <= set(info_f)
    assert np.array_equal(info["putative"], info_f["putative"]) and info["n_features"] == info_f["n_features"]
    assert info["result"]["pairs"] == info_f["result"]["pairs"] and sorted(info["result"]) == sorted(info_f["result"])
    for a, b in zip(info["result"]["inliers"] + info["result"]["models"], info_f["result"]["inliers"] + info_f["result"]["models"]):
        assert np.array_equal(a, b)
    # one entry per pair RANSAC saw: the candidate pairs (all pairs, for two images) with at least 4 putative matches
    put = info_f["putative"]
    seen = [(i, j) for j in range(len(imgs)) for i in range(j) if put[i, j] >= 4]
    assert seen == [(0, 1)] and list(info_f["match_plots"]) == seen == list(info_f["match_plot_lists"])
    lists = info_f["match_plot_lists"][(0, 1)]
    assert len(lists["putative"]) == put[0, 1] and 0 < len(lists["inliers"]) <= len(lists["putative"])
    assert info_f["result"]["pairs"] == [(0, 1)] and np.array_equal(lists["inliers"], info_f["result"]["inliers"][0])  # the verified pair's list
    assert {tuple(r) for r in lists["inliers"].tolist()} <= {tuple(r) for r in lists["putative"].tolist()}
    _check_stitch_plots(info_f, resident=True)
    changed = (_np(info_f["match_plots"][(0, 1)]["putative"]) != _np(info_f["match_plots"][(0, 1)]["original"])).any(2)
    assert changed.sum() > len(lists["putative"])  # something was drawn


def test_stitch_match_plots_on_the_host_and_for_asked_pairs(mods, scene):
    pl = mods["pipeline"]
    imgs, inp, kw, _, _, panos_f, info_f = scene
    panos_h, info_h = pl.stitch(dict(inp, showKeypointsPlot=True), imgs, device_out=False, **kw)
    _check_stitch_plots(info_h, resident=False)
    for name in ("original", "putative", "inliers"):  # the same bytes as the resident pictures
        assert np.array_equal(info_h["match_plots"][(0, 1)][name], _np(info_f["match_plots"][(0, 1)][name]))
    asked = dict(inp, showKeypointsPlot=1, keypointsPlotPairs=[(0, 1)])
    _, info_a = pl.stitch(asked, imgs, **kw)
    assert list(info_a["match_plots"]) == [(0, 1)]
    assert np.array_equal(_np(info_a["match_plots"][(0, 1)]["inliers"]), _np(info_f["match_plots"][(0, 1)]["inliers"]))
    _, info_none = pl.stitch(dict(asked, keypointsPlotPairs=[]), imgs, **kw)
    assert info_none["match_plots"] == {} and info_none["match_plot_lists"] == {}
    for never in ([(1, 0)], [(0, 1), (0, 2)]):  # pairs RANSAC never saw
        with pytest.raises(ValueError, match="keypointsPlotPairs"):
            pl.stitch(dict(asked, keypointsPlotPairs=never), imgs, **kw)
    with pytest.raises(ValueError, match="keypointsPlotPairs"):
        pl.stitch(dict(inp, showKeypointsPlot=1, keypointsPlotLimitBytes=1), imgs, **kw)
    need = mods["imageMatching"].match_plot_bytes([(360, 480)] * 2, [(0, 1)])
    _, info_fit = pl.stitch(dict(inp, showKeypointsPlot=1, keypointsPlotLimitBytes=need), imgs, **kw)  # exactly at the limit
    assert list(info_fit["match_plots"]) == [(0, 1)]
    # a flag that is present and false is no flag
    _, info_off = pl.stitch(dict(inp, showKeypointsPlot=0, keypointsPlotLimitBytes=1), imgs, **kw)
    assert "match_plots" not in info_off
