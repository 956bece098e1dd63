"""The 'miller', 'fisheye' and 'panini' canvases on the device.  The C oracle does not know them: the yardstick is the numpy
mirror of the projection contract (tests/projection_mirror.py; its sampling half is pinned by the oracle in
tests/test_projections.py), the per-tile path for the batched one, and the mirror's independently written forward maps for the
geometry.  Shapes and bounds are those of the tests of the four older modes in tests/test_render_gpu.py."""
import math
from importlib import import_module

import numpy as np
import pytest

import projection_mirror as pm
from test_render_oracle import cam

pytestmark = pytest.mark.gpu

ATOL_F32 = 2e-4  # tests/test_render_gpu.py: anything behind the ray generator
MODES = pm.MODES
SWITCHES = ("APS_RENDER_LEGACY", "APS_WARP_EXACT", "APS_RENDER_NO_CULL", "APS_RENDER_CHECK_RECTS", "APS_RENDER_DEVICE_COVER")


@pytest.fixture(scope="module")
def rp(gpu):
    return import_module(gpu.__name__ + ".renderPanorama")


def _scene(rng, n=3, W=160, H=120, f=220.0):
    """tests/test_render_gpu.py::_scene (smooth): 8 x 8 blocks of constant colour, cameras 0.35 rad apart."""
    imgs, cams = [], []
    for i in range(n):
        base = rng.random((H // 8 + 2, W // 8 + 2, 3))
        imgs.append((np.kron(base, np.ones((8, 8, 1)))[:H, :W] * 255).astype(np.uint8))
        cams.append(cam(f, W, H, yaw=(i - (n - 1) / 2) * 0.35, pitch=0.03 * (-1) ** i))
    return imgs, cams


def _render(rp, monkeypatch, switches, *args, **kw):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s in switches:
        monkeypatch.setenv(s, "1")
    out = rp.renderPanorama(*args, **kw)
    for s in switches:
        monkeypatch.delenv(s)
    return out


# ---- 1. warp_tile against the mirror ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_warp_tile_within_tolerance_of_the_mirror(rp, mode):
    """The geometry and the bounds of test_render_gpu.py::test_warp_tile_within_tolerance.  The mirror's float32 rays are within
    1.5e-7 of the float64 ones on this canvas (3e-5 px at f = 200), the class of the older modes against the oracle."""
    rng = np.random.default_rng(3)
    W, H, f = 160, 120, 200.0
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    c = cam(f, W, H, yaw=0.07, pitch=-0.05)
    Rref = cam(f, W, H, yaw=0.02)["R"]
    geo = {"mode": mode, "H": 150, "W": 220, "fPan": f, "o0": -0.5, "o1": -0.4, "Rref": Rref}
    S, M, Wa, Wf = rp.warp_tile(img, c, geo, 10, 20, 128, 190, 2.0, gain=(1.1, 0.9, 1.0))
    oS, oM, oWa, oWf = pm.warp_tile(img, c, geo, 10, 20, 128, 190, 2.0, gain=(1.1, 0.9, 1.0))
    both = M & oM
    dS = np.abs(S[both] - oS[both])
    print(mode, "mask", oM.sum(), "flips", (M != oM).mean(), "Wang", np.abs(Wa[both] - oWa[both]).max(), "Wf",
          np.abs(Wf[both] - oWf[both]).max(), "colour max", dS.max(), "mean", dS.mean())
    assert oM.sum() > 3000
    assert (M != oM).mean() <= 1e-3
    np.testing.assert_allclose(Wa[both], oWa[both], atol=ATOL_F32)
    np.testing.assert_allclose(Wf[both], oWf[both], atol=ATOL_F32)
    assert dS.max() <= 5e-3
    assert dS.mean() <= ATOL_F32
    assert np.all(S[~M] == 0) and np.all(Wa[~M] == 0) and np.all(Wf[~M] == 0)


# ---- 2. the fisheye's void --------------------------------------------------------------------------------------------------------
def test_fisheye_sees_nothing_beyond_pi(rp):
    """A hand-made canvas whose tile straddles the circle r = pi (fPan = 40, origin at -3.5: the circle crosses row 50 at column
    14.3) under a camera that looks backwards, so that the image lies around the canvas' rim: nothing is sampled outside the
    circle, and inside the device's mask is the mirror's."""
    rng = np.random.default_rng(8)
    W, H = 160, 120
    img = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
    c = {"K": np.array([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1.0]]), "R": np.diag([-1.0, 1.0, -1.0])}
    geo = {"mode": "fisheye", "H": 100, "W": 120, "fPan": 40.0, "o0": -3.5, "o1": -1.25, "Rref": np.eye(3)}
    S, M, Wa, Wf = rp.warp_tile(img, c, geo, 0, 0, 100, 120, 2.0)
    oS, oM, oWa, oWf = pm.warp_tile(img, c, geo, 0, 0, 100, 120, 2.0)
    yp, xp = np.mgrid[0:100, 0:120]
    r_px = np.hypot(geo["o0"] + xp / 40.0, geo["o1"] + yp / 40.0) * 40.0
    outside, ring = r_px > math.pi * 40.0, np.abs(r_px - math.pi * 40.0) <= 1.0
    assert outside.sum() > 300 and (~outside).sum() > 300
    assert not oM[outside].any() and oM[~outside].sum() > 1000  # the mirror: empty beyond pi, not empty inside
    assert not M[outside & ~ring].any() and np.all(S[outside & ~ring] == 0)
    assert ((M != oM) & ~ring).mean() <= 1e-3
    both = M & oM
    np.testing.assert_allclose(Wa[both], oWa[both], atol=ATOL_F32)
    # the whole-canvas render paints nothing there either, on either path
    opts = {"anglePower": 2, "blending": "none", "tile": (64, 96), "cropBorder": False}
    g = dict(geo, refIdx=0)
    pano, _, cov, _ = rp.renderPanorama({}, [img], [(H, W, 3)], [c], "fisheye", 0, opts, return_covered=True, geo=g)
    assert not cov[outside & ~ring].any() and not pano[outside & ~ring].any()
    assert ((cov.astype(bool) != oM) & ~ring).mean() <= 1e-3


# ---- 3. the batched path is the per-tile path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("blending", ["multiband", "linear", "none"])
@pytest.mark.parametrize("mode", MODES)
def test_batched_path_equals_per_tile_path(rp, monkeypatch, mode, blending):
    """APS_WARP_EXACT=1 (the batched pipeline with the per-tile arithmetic in the warp) against APS_RENDER_LEGACY=1 in every
    byte of panorama and coverage; the default batched render within the bound of
    test_render_gpu.py::test_batched_multiband_equals_per_tile_path (max 2, >= 99.95 % within 1); APS_RENDER_NO_CULL=1 changes
    no byte."""
    imgs, cams = _scene(np.random.default_rng(4))
    sizes = [(120, 160, 3)] * 3
    opts = {"anglePower": 2, "blending": blending, "pyrLevels": 3, "pyrSigma": 1.0, "tile": (64, 96), "cropBorder": False}
    args = ({}, imgs, sizes, cams, mode, 1, opts)
    fast, _, fcov, _ = _render(rp, monkeypatch, (), *args, return_covered=True)
    exact, _, ecov, _ = _render(rp, monkeypatch, ("APS_WARP_EXACT",), *args, return_covered=True)
    ref, _, rcov, _ = _render(rp, monkeypatch, ("APS_RENDER_LEGACY",), *args, return_covered=True)
    nocull, _, ncov, _ = _render(rp, monkeypatch, ("APS_RENDER_NO_CULL",), *args, return_covered=True)
    dcover, _, dcov, _ = _render(rp, monkeypatch, ("APS_RENDER_DEVICE_COVER",), *args, return_covered=True)
    assert rcov.sum() > 10000 and (rcov == 0).sum() > 100
    assert np.array_equal(ecov, rcov) and np.array_equal(exact, ref)
    assert np.array_equal(ncov, fcov) and np.array_equal(nocull, fast)
    assert np.array_equal(dcov, fcov) and np.array_equal(dcover, fast)
    assert np.array_equal(fcov, rcov)
    dd = np.abs(fast.astype(int) - exact.astype(int))[(fcov == 1) & (ecov == 1)]
    print(mode, blending, "default against exact: max", dd.max(), "within 1:", (dd <= 1).mean())
    assert dd.max() <= 2 and (dd <= 1).mean() >= 0.9995, (dd.max(), (dd <= 1).mean())
    assert np.all(fast[fcov == 0] == 0)


def test_miller_analytic_footprints_contain_the_exact_ones_for_tilted_wide_and_near_pole_cameras(rp, monkeypatch):
    """The camera set of test_render_gpu.py::test_analytic_footprints_contain_the_exact_ones... (rolled and pitched cameras, a
    wide field of view, views close to a pole, one across the theta = +-pi seam) on the Miller canvas: the check inside the
    library raises if an exact footprint leaves its analytic rectangle; the panorama must equal the device-cover one."""
    rng = np.random.default_rng(41)
    W, H = 200, 150

    def rot(yaw, pitch, roll):
        cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
        Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1.0]])
        return (Ry @ Rx @ Rz).T

    poses = [(0.0, 0.0, 0.0, 260.0), (0.5, 0.3, 0.4, 260.0), (-0.6, -0.5, -0.7, 180.0), (1.2, 0.9, 0.2, 300.0),
             (-1.4, -1.0, 1.0, 240.0), (2.2, 0.1, -0.3, 120.0)]
    for seam in (False, True):
        ps = poses + [(3.1, 0.2, 0.1, 260.0)] if seam else poses  # straddles the seam: the analytic path declines
        imgs, cams = [], []
        for (yaw, pitch, roll, f) in ps:
            base = rng.random((H // 8 + 2, W // 8 + 2, 3))
            imgs.append((np.kron(base, np.ones((8, 8, 1)))[:H, :W] * 255).astype(np.uint8))
            cams.append({"K": np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]]), "R": rot(yaw, pitch, roll)})
        sizes = [(H, W, 3)] * len(imgs)
        opts = {"anglePower": 2, "blending": "multiband", "pyrLevels": 4, "pyrSigma": 1.0, "tile": (96, 128), "cropBorder": False}
        args = ({}, imgs, sizes, cams, "miller", 0, opts)
        pano, _, cov, geo = _render(rp, monkeypatch, ("APS_RENDER_CHECK_RECTS",), *args, return_covered=True)
        ref, _, rcov, _ = _render(rp, monkeypatch, ("APS_RENDER_DEVICE_COVER",), *args, return_covered=True)
        assert cov.sum() > 20000 and np.array_equal(cov, rcov) and np.array_equal(pano, ref)
        assert geo["H"] < 2 * pm.MILLER_POLE * geo["fPan"] * 1.03  # the poles are at a finite height


# ---- 4. geometry, independent of the mirror's inverse ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_block_centres_land_where_the_forward_map_says(rp, mode):
    """One wide image (+-45 degrees) whose camera is the reference, blending 'none', anglePower 1, gains 1: the image consists of
    8 x 8 blocks of constant colour, and the canvas pixel nearest to the forward image of a block's centre must hold exactly that
    block's colour.  (Rounding to the canvas pixel moves the ray by at most half a canvas pixel, at most 1.4 image pixels at the
    rim of this view; a block centre is 3.5 pixels from the nearest pixel whose bilinear taps leave the block.)"""
    rng = np.random.default_rng(12)
    W, H, f = 160, 120, 80.0
    base = rng.integers(1, 256, (H // 8, W // 8, 3)).astype(np.uint8)
    img = np.kron(base, np.ones((8, 8, 1), np.uint8))
    c = cam(f, W, H, yaw=0.2, pitch=-0.1)
    opts = {"anglePower": 1, "blending": "none", "tile": (64, 96), "cropBorder": False, "fPan": f, "autoRef": False}
    pano, _, cov, geo = rp.renderPanorama({}, [img], [(H, W, 3)], [c], mode, 0, opts, return_covered=True)
    by, bx = np.mgrid[0:H // 8, 0:W // 8]
    u, v = 8.0 * bx + 4.5, 8.0 * by + 4.5  # block centres, 1-based pixel coordinates: >= 3 px from every block edge
    rays = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(np.asarray(c["K"])).T @ np.asarray(c["R"])  # R' K^-1 [u v 1]'
    _, _, xp, yp = pm.forward(mode, geo, rays)
    xi, yi = np.rint(xp).astype(int), np.rint(yp).astype(int)
    assert xi.min() >= 0 and yi.min() >= 0 and xi.max() < geo["W"] and yi.max() < geo["H"]
    assert len({(a, b) for a, b in zip(xi.ravel(), yi.ravel())}) == xi.size  # distinct canvas pixels
    assert cov[yi, xi].all()
    assert np.array_equal(pano[yi, xi], base)


# ---- 5. tile ranges compose -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fisheye", "miller"])
def test_contiguous_tile_ranges_compose_to_the_full_render(gpu, rp, mode):
    """test_render_gpu.py::test_contiguous_tile_ranges_compose_to_the_full_render at world = 3, host and resident."""
    import torch

    par = import_module(gpu.__name__ + ".parallel")
    rng = np.random.default_rng(33)
    imgs, cams = _scene(rng, n=5, W=200, H=130, f=280.0)
    sizes = [(130, 200, 3)] * 5
    opts = {"anglePower": 2, "blending": "multiband", "pyrLevels": 4, "pyrSigma": 1.0, "tile": (64, 80), "cropBorder": False}
    full, _, cov, geo = rp.renderPanorama({}, imgs, sizes, cams, mode, 2, opts, return_covered=True)
    ranges = par.tile_ranges(int(geo["H"]), int(geo["W"]), (64, 80), 3)
    acc, acc_t = np.zeros_like(full), None
    dimgs = [torch.from_numpy(i).cuda() for i in imgs]
    torch.cuda.synchronize()
    for r in range(3):
        part, _ = rp.renderPanorama({}, imgs, sizes, cams, mode, 2, opts, tile_subset=("range",) + ranges[r])
        assert not (acc.astype(bool) & part.astype(bool)).any()  # disjoint
        acc = np.maximum(acc, part)
        pt, _ = rp.renderPanorama({}, dimgs, sizes, cams, mode, 2, opts, tile_subset=("range",) + ranges[r], device_out=True)
        acc_t = pt if acc_t is None else torch.maximum(acc_t, pt)
    assert cov.sum() > 10000 and np.array_equal(acc, full)
    assert np.array_equal(acc_t.cpu().numpy(), full)


# ---- 6. gain compensation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_gain_compensation_recovers_planted_gains(gpu, rp, mode):
    """test_render_gpu.py::test_gain_compensation_recovers_planted_gains, its scene and its acceptance numbers."""
    gc = import_module(gpu.__name__ + ".gainCompensation")
    rng = np.random.default_rng(43)
    imgs, cams = _scene(rng, n=4, W=200, H=140, f=300.0)
    smooth = [np.clip(60 + 0.5 * im.astype(np.float32), 0, 255) for im in imgs]
    planted = np.array([1.0, 0.7, 1.3, 0.85])
    imgs2 = [np.clip(s * p, 0, 255).astype(np.uint8) for s, p in zip(smooth, planted)]
    sizes = [(140, 200, 3)] * 4
    o = rp.default_opts({"anglePower": 2}, cams, 1)
    geo = rp.canvas_geometry(cams, sizes, mode, 1, o)
    Nij, _, _ = gc.gain_overlap_stats(imgs2, cams, geo, 2)
    assert np.count_nonzero(Nij >= 30) >= 3  # the three neighbouring pairs overlap
    g = gc.gainCompensationRKf(imgs2, cams, mode, 1, {"overlapStride": 2, "minOverlapSamples": 30}, geo)
    prod = g[:, 0] * planted
    print(mode, "gains", g[:, 0], "std / mean", prod.std() / prod.mean())
    assert prod.std() / prod.mean() < 0.08  # g_i * planted_i is (nearly) one constant
    assert np.allclose(g[:, 0], g[:, 1], rtol=0.05)
    # the mode's spelling is canvas_geometry's: case does not matter
    assert np.array_equal(gc.gainCompensationRKf(imgs2, cams, mode.upper(), 1, {"overlapStride": 2, "minOverlapSamples": 30}, geo), g)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------
FLAGS = {"showPanoramaImgsNums": True, "showCropBoundingBox": True}


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _crop_share(mask):
    """The covered share of a panorama after cropNonzeroBbox: the bounding box of the mask, padded by 6 px inside the canvas."""
    rows, cols = np.flatnonzero(mask.any(1)), np.flatnonzero(mask.any(0))
    r1, r2 = max(rows[0] - 6, 0), min(rows[-1] + 6, mask.shape[0] - 1)
    c1, c2 = max(cols[0] - 6, 0), min(cols[-1] + 6, mask.shape[1] - 1)
    return mask[r1:r2 + 1, c1:c2 + 1].mean(), (r2 - r1 + 1, c2 - c1 + 1)


@pytest.fixture(scope="module")
def stitched(gpu, rp):
    """The two-view scene of tests/test_annotate_gpu.py::test_stitch_fills_info_annotated, stitched in 'spherical' mode."""
    import torch

    synth, pl = import_module(gpu.__name__ + ".synth"), import_module(gpu.__name__ + ".pipeline")
    w, h, f = 480, 360, 700.0
    cams = synth.grid_cameras(2, 1, w, h, f, 2 * np.arctan(w / (2 * f)) * 0.5, 0.0, 1.0, 11)
    imgs = [synth.render_view(c, h, w, 11, "cuda", finest_px=1.5) for c in cams]
    torch.cuda.synchronize()
    Ks = [c["K"] for c in cams]
    panos, info = pl.stitch(pl.default_input(bands=2, resizeImage=0), imgs, Ks=Ks, tile=(256, 256))
    assert len(panos) == 1
    return pl, imgs, Ks, _np(panos[0]), info


@pytest.mark.parametrize("mode", MODES)
def test_stitch_end_to_end(rp, stitched, mode):
    """pipeline.stitch in the new mode: a non-empty panorama whose covered share is within 10 % of the share predicted from the
    spherical panorama - every covered spherical pixel (four sub-samples) sent along its ray through the mirror's forward map
    onto the new mode's canvas; and with the two annotation flags an annotated picture of the same size."""
    pl, imgs, Ks, pano_s, info_s = stitched
    comp = info_s["components"][0]
    cams, ref = comp["cameras"], comp["ref"]
    sizes = [(360, 480, 3)] * 2
    inp = pl.default_input(bands=2, resizeImage=0, panorama2DisplaynSave=mode)
    panos, info = pl.stitch(inp, imgs, Ks=Ks, tile=(256, 256))
    assert len(panos) == 1 and "annotated" not in info
    pano = _np(panos[0])
    covered = (pano > 0).any(2)
    assert pano.ndim == 3 and pano.shape[2] == 3 and covered.sum() > 100000
    # the spherical panorama, uncropped, with its canvas: its crop is what stitch returned
    opts = {"anglePower": 2, "blending": inp["blending"], "pyrLevels": inp["bands"], "pyrSigma": inp["MBBsigma"],
            "canvasColor": inp["canvasColor"], "tile": (256, 256), "cropBorder": False}
    full_s, _, _, geo_s = rp.renderPanorama(inp, imgs, sizes, cams, "spherical", ref, opts, return_covered=True, device_out=True)
    full_s = _np(full_s)
    cropped, _, _ = rp.cropNonzeroBbox(full_s, "black")
    assert np.array_equal(cropped, pano_s)
    ys, xs = np.nonzero((full_s > 0).any(2))
    geo_m = rp.canvas_geometry(cams, sizes, mode, ref, rp.default_opts(opts, cams, ref))
    pred = np.zeros((geo_m["H"], geo_m["W"]), bool)
    for dy in (-0.25, 0.25):
        for dx in (-0.25, 0.25):
            th, ph = geo_s["o0"] + (xs + dx) / geo_s["fPan"], geo_s["o1"] + (ys + dy) / geo_s["fPan"]
            rays = np.stack([np.cos(ph) * np.sin(th), np.sin(ph), np.cos(ph) * np.cos(th)], -1)
            _, _, xp, yp = pm.forward(mode, geo_m, rays)
            xi, yi = np.rint(xp).astype(int), np.rint(yp).astype(int)
            ok = (xi >= 0) & (xi < geo_m["W"]) & (yi >= 0) & (yi < geo_m["H"])
            pred[yi[ok], xi[ok]] = True
    share_pred, shape_pred = _crop_share(pred)
    share = covered.mean()
    print(mode, "covered share", share, "predicted", share_pred, "shape", pano.shape[:2], "predicted", shape_pred)
    assert abs(share - share_pred) <= 0.10 * share_pred
    assert abs(pano.shape[0] - shape_pred[0]) <= 4 and abs(pano.shape[1] - shape_pred[1]) <= 4
    # annotated
    panos2, info2 = pl.stitch(dict(inp, **FLAGS), imgs, Ks=Ks, tile=(256, 256))
    ann = _np(info2["annotated"][0])
    assert np.array_equal(_np(panos2[0]), pano) and ann.shape == pano.shape and ann.dtype == np.uint8
    changed = (ann != pano).any(2)
    assert 0 < changed.mean() < 0.2
    pal = rp.vivid_palette(2)
    assert all(((ann == c).all(2) & changed).sum() > 200 for c in pal)  # two outlines in the palette's colours


def test_display_panorama_in_all_eight_projections(gpu, rp):
    ip = import_module(gpu.__name__ + ".imageProcessing")
    imgs, cams = _scene(np.random.default_rng(6))
    names = ["planar", "cylindrical", "spherical", "equirectangular", "stereographic", "miller", "fisheye", "panini"]
    inp = {"panorama2DisplaynSave": names, "canvasColor": "black", "gainCompensation": 0, "sigmaN": 10.0, "sigmag": 0.1,
           "bands": 2, "blending": "linear", "MBBsigma": 1.0, "tile": (64, 64), "transformationType": "projective",
           "cropPanorama": 0, **FLAGS}
    sizes = np.array([[120, 160, 3]] * 3)
    store = rp.displayPanorama(inp, [cams, cams[:2]], [2, 1], imgs, sizes, [[1, 2, 3], [1, 2]])
    assert len(store) == 2
    for rec in store:
        assert sorted(rec) == sorted(names)
        for p in names:
            pano, ann = rec[p]
            assert pano.any() and ann is not None and ann.shape == pano.shape and (ann != pano).any()
    assert np.array_equal(store[0]["spherical"][0], store[0]["equirectangular"][0])
    files = [n for n, *_ in ip.panorama_file_names(inp, store, 1, ["scene"])]
    assert len(files) == 2 * 2 * 8 and "panini_annotated_projective_1_2_scene.png" in files
