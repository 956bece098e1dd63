"""The 'miller', 'fisheye' and 'panini' canvases on the host (no GPU): the numpy mirror of the projection contract
(tests/projection_mirror.py) is checked against itself (forward after inverse) and, for its sampling half, against the C oracle
in 'spherical' mode; canvas_geometry, warped_boxes, the enum and the file names are checked against the mirror and the issue's
stated properties."""
import math
from importlib import import_module

import numpy as np
import pytest

import oracle
import projection_mirror as pm
from test_render_oracle import cam


@pytest.fixture(scope="module")
def rp(aps):
    return import_module(aps.__name__ + ".renderPanorama")


def _scene(rng, n=3, W=160, H=120, f=220.0):
    """tests/test_render_gpu.py::_scene (smooth): 8 x 8 blocks of constant colour, cameras 0.35 rad apart."""
    imgs, cams = [], []
    for i in range(n):
        base = rng.random((H // 8 + 2, W // 8 + 2, 3))
        imgs.append((np.kron(base, np.ones((8, 8, 1)))[:H, :W] * 255).astype(np.uint8))
        cams.append(cam(f, W, H, yaw=(i - (n - 1) / 2) * 0.35, pitch=0.03 * (-1) ** i))
    return imgs, cams


GEO_I = {"fPan": 1.0, "o0": 0.0, "o1": 0.0, "Rref": np.eye(3)}


@pytest.mark.parametrize("mode", pm.MODES)
def test_forward_after_inverse_is_the_identity(mode):
    """10^4 random directions inside the map's domain, f64: direction -> (a, b) by the forward map -> ray by the contract's
    inverse -> the direction again; and (a, b) -> ray -> (a, b).  Measured (direction): 1.5e-15 (Miller), 8e-16 (fisheye),
    4.4e-16 (Panini)."""
    d = pm.random_directions(mode, 10000, np.random.default_rng(7))
    a, b, _, _ = pm.forward(mode, GEO_I, d)
    r = pm.inverse_f64(mode, a, b)
    r /= np.sqrt((r ** 2).sum(1, keepdims=True))
    err = np.abs(r - d).max()
    a2, b2, _, _ = pm.forward(mode, GEO_I, r)
    err_ab = max(np.abs(a2 - a).max(), np.abs(b2 - b).max())
    print(mode, "direction round trip", err, "coordinate round trip", err_ab)
    assert err <= 1e-12
    assert err_ab <= 1e-9  # (the coordinates amplify a direction error by the map's local magnification, up to ~4e2 here)


@pytest.mark.parametrize("mode", pm.MODES)
def test_f32_inverse_agrees_with_f64(mode):
    """The float32 inverse in the device's operation order against the float64 one on the canvas of the warp_tile tests: the ray
    error is that of float32 (measured <= 1.5e-7), i.e. ~3e-5 px at f = 200 - the class of the four older modes."""
    geo = {"mode": mode, "H": 150, "W": 220, "fPan": 200.0, "o0": -0.5, "o1": -0.4, "Rref": cam(200.0, 160, 120, yaw=0.02)["R"]}
    yp, xp = np.mgrid[0:150, 0:220]
    d32 = pm.inverse(mode, geo, xp, yp)
    a, b = geo["o0"] + xp / geo["fPan"], geo["o1"] + yp / geo["fPan"]
    r = pm.inverse_f64(mode, a, b)
    if mode != "miller":
        r = r @ np.asarray(geo["Rref"], np.float64)  # world = Rref' * r
    r /= np.sqrt((r ** 2).sum(-1, keepdims=True))
    assert np.abs(d32.astype(np.float64) - r).max() <= 5e-7
    # and forward(inverse(pixel)) is the pixel
    _, _, fx, fy = pm.forward(mode, geo, d32)
    assert np.abs(fx - xp).max() <= 1e-3 and np.abs(fy - yp).max() <= 1e-3


def test_mirror_sampling_half_is_the_oracles():
    """project + sample_one as the mirror restates them, pinned ONCE by the C oracle: 'spherical' mode, the geometry of
    test_render_gpu.py::test_warp_tile_within_tolerance.  Both sides are CPU float32; they differ through numpy's and glibc's
    sinf / cosf only, so the bounds are that test's own."""
    rng = np.random.default_rng(3)
    W, H, f = 160, 120, 200.0
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    c = cam(f, W, H, yaw=0.07, pitch=-0.05)
    geo = {"mode": "spherical", "H": 150, "W": 220, "fPan": f, "o0": -0.5, "o1": -0.4, "Rref": cam(f, W, H, yaw=0.02)["R"]}
    S, M, Wa, Wf = pm.warp_tile(img, c, geo, 10, 20, 128, 190, 2.0, gain=(1.1, 0.9, 1.0))
    oS, oM, oWa, oWf = oracle.warp_tile(img, c, geo, 10, 20, 128, 190, 2.0, gain=(1.1, 0.9, 1.0))
    assert oM.sum() > 3000 and (M != oM).mean() <= 1e-3
    both = M & oM
    np.testing.assert_allclose(Wa[both], oWa[both], atol=2e-4)
    np.testing.assert_allclose(Wf[both], oWf[both], atol=2e-4)
    assert np.abs(S[both] - oS[both]).max() <= 5e-3 and np.abs(S[both] - oS[both]).mean() <= 2e-4
    assert np.all(S[~M] == 0) and np.all(Wa[~M] == 0) and np.all(Wf[~M] == 0)
    for n in (1, 2, 5, 8, 120, 161):
        assert np.array_equal(pm.tent(n), oracle.tent(n))


def test_fisheye_void_rule_of_the_mirror():
    geo = {"mode": "fisheye", "H": 64, "W": 64, "fPan": 40.0, "o0": -3.5, "o1": -0.8, "Rref": np.eye(3)}
    yp, xp = np.mgrid[0:64, 0:64]
    d = pm.inverse("fisheye", geo, xp, yp)
    a, b = pm.ab_of_pixel(geo, xp, yp)
    r = np.hypot(a.astype(np.float64), b.astype(np.float64))
    void = (d == 0).all(-1)
    assert void.any() and (~void).any()
    assert np.array_equal(void[np.abs(r - np.pi) > 1e-5], (r > np.pi)[np.abs(r - np.pi) > 1e-5])
    assert np.allclose(np.sqrt((d[~void].astype(np.float64) ** 2).sum(-1)), 1.0, atol=1e-6)


def test_canvas_geometry_of_the_new_modes(rp):
    imgs, cams = _scene(np.random.default_rng(6))
    sizes = [(120, 160, 3)] * 3
    o = rp.default_opts({"anglePower": 2}, cams, 1)
    sph = rp.canvas_geometry(cams, sizes, "spherical", 1, o)
    geos = {m: rp.canvas_geometry(cams, sizes, m, 1, o) for m in pm.MODES}
    for m, g in geos.items():
        assert g["mode"] == m and g["H"] > 0 and g["W"] > 0 and math.isfinite(g["o0"]) and math.isfinite(g["o1"])
        assert g["H"] * g["W"] < 4 * sph["H"] * sph["W"]  # a 1.4 rad fan: every map is within a small factor of the sphere's
    assert geos["fisheye"]["H"] == geos["fisheye"]["W"] and geos["fisheye"]["o0"] == geos["fisheye"]["o1"]
    assert geos["miller"]["W"] == sph["W"] and geos["miller"]["o0"] == sph["o0"]
    assert geos["miller"]["H"] >= sph["H"]  # |1.25 asinh(tan(0.8 ph))| >= |ph|
    # the bounds functions against the mirror's forward maps on the cameras' own corner and border rays
    t0, t1, p0, p1 = rp.sphericalBounds(cams, sizes)
    m0, m1, y0, y1 = rp.millerBounds(cams, sizes)
    assert (m0, m1) == (t0, t1) and abs(y0 - 1.25 * math.asinh(math.tan(0.8 * p0))) < 1e-15 and abs(y1 - 1.25 * math.asinh(math.tan(0.8 * p1))) < 1e-15
    Rref = cams[1]["R"]
    g = {"fPan": 1.0, "o0": 0.0, "o1": 0.0, "Rref": Rref}
    rays = np.concatenate([r.T for r in rp._all_grid_rays(cams, sizes, border=512)])
    for mode, got in (("fisheye", rp.fisheyeBounds(cams, sizes, Rref, (0, 100))),
                      ("panini", rp.paniniBounds(cams, sizes, Rref, (0, 100), 8.0))):
        a, b, _, _ = pm.forward(mode, g, rays)
        np.testing.assert_allclose(got, (a.min(), a.max(), b.min(), b.max()), rtol=0, atol=1e-12)
    # the megapixel cap and the reference choice apply to both R_ref-family modes
    for m in ("fisheye", "panini"):
        capped = rp.canvas_geometry(cams, sizes, m, 1, dict(o, maxMegapixel=0.05))
        assert capped["H"] * capped["W"] <= 0.05e6 * 1.05 and capped["H"] < geos[m]["H"]
        assert rp.canvas_geometry(cams, sizes, m, 0, dict(o, autoRef=True))["refIdx"] == 1  # the middle camera: smallest canvas
        assert rp.canvas_geometry(cams, sizes, m, 0, dict(o, autoRef=False))["refIdx"] == 0


def test_miller_canvas_stops_at_the_poles(rp):
    """A view that contains the zenith: the elevation bound is the pole, and the margin must not add rows beyond it (there the
    elevation 1.25 atan(sinh(0.8 b)) passes 90 degrees and the ray wraps to the opposite azimuth)."""
    cams = [cam(220.0, 160, 120, pitch=0.0), cam(220.0, 160, 120, pitch=1.45), cam(220.0, 160, 120, pitch=-1.45)]
    sizes = [(120, 160, 3)] * 3
    o = rp.default_opts({"anglePower": 2, "margin": 0.05}, cams, 0)
    g = rp.canvas_geometry(cams, sizes, "miller", 0, o)
    f = g["fPan"]
    assert -pm.MILLER_POLE <= g["o1"] and g["o1"] + (g["H"] - 1) / f <= pm.MILLER_POLE
    assert g["H"] >= 0.95 * 2 * pm.MILLER_POLE * f  # and it does reach them
    assert abs(rp.MILLER_POLE - pm.MILLER_POLE) < 1e-15
    d = pm.inverse("miller", g, np.zeros(g["H"]), np.arange(g["H"]))
    assert (d[:, 2] * math.cos(g["o0"]) >= -1e-6).all()  # column 0 looks along azimuth o0 in every row: none wraps over a pole


def test_mercator_is_still_an_unknown_mode(rp):
    imgs, cams = _scene(np.random.default_rng(6))
    o = rp.default_opts({"anglePower": 2}, cams, 1)
    for name in ("mercator", "Mercator", "transverse", "miller2"):
        with pytest.raises(ValueError, match="mode must be cylindrical, spherical, or planar/perspective"):
            rp.canvas_geometry(cams, [(120, 160, 3)] * 3, name, 1, o)


def test_enum_values_are_exported(aps):
    capi = aps._capi
    assert (capi.APS_PROJ_MILLER, capi.APS_PROJ_FISHEYE, capi.APS_PROJ_PANINI) == (4, 5, 6)
    assert (capi.APS_PROJ_CYLINDRICAL, capi.APS_PROJ_SPHERICAL, capi.APS_PROJ_PLANAR, capi.APS_PROJ_STEREOGRAPHIC) == (0, 1, 2, 3)
    rp = import_module(aps.__name__ + ".renderPanorama")
    assert {m: rp._MODES[m] for m in pm.MODES} == {"miller": 4, "fisheye": 5, "panini": 6}
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aps.h")).read()
    for name, value in (("MILLER", 4), ("FISHEYE", 5), ("PANINI", 6)):
        assert re.search(rf"APS_PROJ_{name}\s*=\s*{value}\b", header)


@pytest.mark.parametrize("mode", pm.MODES)
def test_warped_boxes_agree_with_the_forward_map(rp, mode):
    imgs, cams = _scene(np.random.default_rng(6))
    sizes = [(120, 160, 3)] * 3
    geo = rp.canvas_geometry(cams, sizes, mode, 1, rp.default_opts({"anglePower": 2}, cams, 1))
    polys, centers = rp.warped_boxes(cams, sizes, geo)
    assert polys.shape == (3, 4, 2)
    for i, c in enumerate(cams):
        corners = np.array([[1.0, 1.0, 1.0], [160.0, 1.0, 1.0], [160.0, 120.0, 1.0], [1.0, 120.0, 1.0]])  # (x, y, 1)
        rays = (np.asarray(c["R"]).T @ np.linalg.solve(np.asarray(c["K"]), corners.T)).T
        _, _, xp, yp = pm.forward(mode, geo, rays)
        np.testing.assert_allclose(polys[i], np.stack([xp + 1.0, yp + 1.0], 1), rtol=0, atol=1e-9)  # 1-based
    np.testing.assert_allclose(centers, polys.mean(1), rtol=0, atol=1e-12)
    assert (polys[:, :, 0] > 0).all() and (polys[:, :, 0] < geo["W"] + 1).all()
    assert (polys[:, :, 1] > 0).all() and (polys[:, :, 1] < geo["H"] + 1).all()


def test_panorama_file_names_carry_the_new_prefixes(aps):
    ip = import_module(aps.__name__ + ".imageProcessing")
    assert ip.PANO_PROJECTIONS == ("planar", "cylindrical", "spherical", "equirectangular", "stereographic", "miller", "fisheye",
                                   "panini")
    store = [{"panini": [1, 2, 3], "spherical": [1, 2, 3], "miller": [1, 2, 3]}, {"fisheye": [1, 2, 3], "cylindrical": []}]
    inp = {"transformationType": "projective", "cropPanorama": 1, "showPanoramaImgsNums": True, "showCropBoundingBox": True}
    names = [n for n, *_ in ip.panorama_file_names(inp, store, 2, ["a", "Grand Canyon"])]
    assert names == [f"{p}{tag}_projective_2_{ii}_Grand Canyon.png"
                     for ii, have in ((1, ("spherical", "miller", "panini")), (2, ("fisheye",)))
                     for tag in ("", "_cropped", "_annotated") for p in have]
