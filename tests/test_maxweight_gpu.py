"""GPU tests of multiband blending over max-weight seams ("Max-weight multiband contract"):
opts['multibandWeights'] = 'maxweight', APS_BLEND_MULTIBAND_MAXWEIGHT, aps_maxweight_weights.

The expected pictures are built from pieces that are pinned elsewhere: renderPanorama.warp_tile (the per-tile path's sampler),
the NumPy partition of tests/maxweight_mirror.py, oracle.multiband_blend and the renderer's paint rule."""
import os
from importlib import import_module

import numpy as np
import pytest

import maxweight_cases as mc
import maxweight_mirror as mm
import oracle
import render_space_cases as rc
from test_render_gpu import ATOL_F32, _scene

pytestmark = pytest.mark.gpu

SWITCHES = ("APS_RENDER_LEGACY", "APS_WARP_EXACT", "APS_RENDER_DEVICE_COVER", "APS_RENDER_NO_CULL", "APS_RENDER_CHECK_RECTS",
            "APS_PLANAR_HOST", "APS_PLANAR_NO_CULL")


@pytest.fixture(scope="module")
def rp(gpu):
    return import_module(gpu.__name__ + ".renderPanorama")


@pytest.fixture(scope="module")
def bl(gpu):
    return import_module(gpu.__name__ + ".blending")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Switches:
    """The environment switches of one render: all of SWITCHES cleared, the given ones set, the old state put back."""

    def __init__(self, *on):
        self.on = on

    def __enter__(self):
        self.old = {s: os.environ.pop(s, None) for s in SWITCHES}
        for s in self.on:
            os.environ[s] = "1"

    def __exit__(self, *exc):
        for s in SWITCHES:
            os.environ.pop(s, None)
            if self.old[s] is not None:
                os.environ[s] = self.old[s]


# ---- 1. the stand-alone operator ---------------------------------------------------------------------------------------------------
def engineered(K, h, w):
    """Exact ties, zeros, negatives and one NaN."""
    rng = np.random.default_rng(100 * K + h)
    W = rng.random((K, h, w), dtype=np.float32)
    W[:, : h // 4, : w // 3] = 0
    W[K - 1, h // 2:, :] = -W[K - 1, h // 2:, :]
    if K > 1:
        W[K // 2, :, w // 2:] = W[0, :, w // 2:]
    W[rng.integers(K), h - 1, w - 1] = np.nan
    return W


@pytest.mark.parametrize("h,w", [(1, 1), (33, 47), (64, 96)])
@pytest.mark.parametrize("K", [1, 2, 7, 17, 65])
def test_maxweight_weights_equals_the_mirror_bit_for_bit(gpu, bl, K, h, w):
    import torch

    capi = gpu._capi
    W = engineered(K, h, w)
    want = mm.partition(W)
    with np.errstate(invalid="ignore"):
        assert h * w == 1 or (0 < (W > 0).any(0).mean() < 1 and want.sum(0).max() == 1)
    # host pointers, out of place and in place
    out = np.full_like(W, 7)
    capi.check(capi.lib.aps_maxweight_weights(capi.ptr(W), K, h, w, capi.ptr(out)))
    assert np.array_equal(bits(out), bits(want))
    inplace = W.copy()
    capi.check(capi.lib.aps_maxweight_weights(capi.ptr(inplace), K, h, w, capi.ptr(inplace)))
    assert np.array_equal(bits(inplace), bits(want))
    # resident pointers, out of place and in place
    d = torch.from_numpy(W).cuda()
    do = torch.full_like(d, 7)
    torch.cuda.synchronize()
    capi.check(capi.lib.aps_maxweight_weights(capi.ptr(d), K, h, w, capi.ptr(do)))
    assert np.array_equal(bits(do.cpu().numpy()), bits(want)) and np.array_equal(bits(d.cpu().numpy()), bits(W))
    capi.check(capi.lib.aps_maxweight_weights(capi.ptr(d), K, h, w, capi.ptr(d)))
    assert np.array_equal(bits(d.cpu().numpy()), bits(want))
    # the public wrappers: numpy in, numpy out; resident in, resident out
    assert np.array_equal(bits(bl.maxWeightPartition(W)), bits(want))
    assert np.array_equal(bits(bl.maxWeightPartition(list(W))), bits(want))
    r = bl.maxWeightPartition(torch.from_numpy(W).cuda())
    assert r.is_cuda and np.array_equal(bits(r.cpu().numpy()), bits(want))


def test_multiBandBlending_with_maxweight_is_the_blend_of_the_partition(bl):
    rng = np.random.default_rng(3)
    K, h, w = 5, 33, 47
    C = rng.random((K, h, w, 3), dtype=np.float32)
    W = np.nan_to_num(engineered(K, h, w))
    for levels in (1, 3):
        F = bl.multiBandBlending(list(C), list(W), levels, True, 1.0, Weights="maxweight")
        assert np.array_equal(bits(F), bits(oracle.multiband_blend(C, mm.partition(W), levels, 1.0)))
    assert np.array_equal(bits(bl.multiBandBlending(list(C), list(W), 1, True, 1.0, Weights="maxweight")),
                          bits(np.clip(mm.owner_colour(C, W), 0, 1)))
    assert np.array_equal(bits(bl.multiBandBlending(list(C), list(W), 3, True, 1.0, Weights="tent")),
                          bits(bl.multiBandBlending(list(C), list(W), 3, True, 1.0)))


# ---- 2. planar scans ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planar_setup(gpu):
    """The three-image set-up of test_render_gpu.test_planar_scan_compositing_matches_oracle_pieces and its warped pieces."""
    ip = import_module(gpu.__name__ + ".imageProcessing")
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 256, (60, 90, 3), dtype=np.uint8) for _ in range(3)]
    Hs = [np.eye(3), np.array([[1.0, 0.01, 55.0], [-0.01, 1.0, 4.0], [1e-5, 0, 1.0]]),
          np.array([[0.98, 0.0, 108.5], [0.02, 1.01, -6.0], [0, 2e-5, 1.0]])]
    lims = [ip.outputLimitsScratch(H, (1, 90), (1, 60)) for H in Hs]
    xMin, xMax = min(l[0][0] for l in lims), max(l[0][1] for l in lims)
    yMin, yMax = min(l[1][0] for l in lims), max(l[1][1] for l in lims)
    width, height = int(np.floor(xMax - xMin + 0.5)), int(np.floor(yMax - yMin + 0.5))
    sx, sy = (xMax - xMin) / width, (yMax - yMin) / height
    tent = np.outer(oracle.tent(60), oracle.tent(90)).astype(np.float32)
    C = np.stack([oracle.image_warp_h(im.astype(np.float32) / 255.0, H, height, width, xMin, yMin, sx, sy, 0.0) for im, H in zip(imgs, Hs)])
    W = np.stack([np.clip(oracle.image_warp_h(tent, H, height, width, xMin, yMin, sx, sy, 0.0), 0, 1) for H in Hs])
    return imgs, Hs, C, W


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("compositor", ["device", "compact", "host"])
def test_planar_scans_are_bit_exact_against_oracle_pieces(rp, planar_setup, compositor, levels):
    imgs, Hs, C, W = planar_setup
    cams = [{"H2refined": H, "noRotation": 1} for H in Hs]
    opts = {"blending": "multiband", "multibandWeights": "maxweight", "pyrLevels": levels, "pyrSigma": 1.0, "canvasColor": "white",
            "planarCompositor": compositor}
    with Switches():
        pano, ann = rp.renderPanorama({"forcePlanarScan": True}, imgs, [(60, 90, 3)] * 3, cams, "planar", 0, opts)
        none, _ = rp.renderPanorama({"forcePlanarScan": True}, imgs, [(60, 90, 3)] * 3, cams, "planar", 0, dict(opts, blending="none"))
    F = np.array(oracle.multiband_blend(C, mm.partition(W), levels, 1.0), np.float32)
    F[~(W > 0).any(0)] = 1.0
    ref = np.clip(np.floor(255.0 * F.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)   # that test's paint
    assert pano.shape == ref.shape and ann is None and 0.5 < (W > 0).any(0).mean() < 1
    assert (mm.partition(W).sum(0) > 0).sum() == (W > 0).any(0).sum() and ((W > 0).sum(0) > 1).mean() > 0.1
    assert np.array_equal(pano, ref)
    if levels == 1:
        assert np.array_equal(pano, none)   # one level: the owner's colour, which is what 'none' paints


# ---- 3, 4, 6. ray canvases: the per-tile path against the pieces, the batched path against the per-tile path -----------------------
_SCENE6 = {}


def scene6():
    if not _SCENE6:
        imgs, cams = _scene(np.random.default_rng(21), n=6, W=220, H=140, f=300.0)
        _SCENE6.update(imgs=imgs, cams=cams, sizes=[(140, 220, 3)] * 6)
    return _SCENE6


_RENDERS = {}


def render6(rp, case, weights, *switches):
    """One render of the six-view scene, computed once per (case, weights, switches) and shared by the tests below."""
    key = (case, weights, switches)
    if key not in _RENDERS:
        sc = scene6()
        with Switches(*switches):
            pano, _, cov, geo = rp.renderPanorama({}, sc["imgs"], sc["sizes"], sc["cams"], case.mode, 2, mc.ray_opts(case, weights),
                                                  gains=mc.GAINS6 if case.gains else None, return_covered=True)
        for a in (pano, cov):
            a.setflags(write=False)
        _RENDERS[key] = (pano, cov, geo)
    return _RENDERS[key]


ray_cases = pytest.mark.parametrize("case", mc.RAY_CASES, ids=mc.ray_id)


@ray_cases
def test_per_tile_path_equals_the_contract_from_pieces(rp, case):
    """APS_RENDER_LEGACY=1: per tile rp.warp_tile per image -> mirror partition of Wang * Wf -> oracle.multiband_blend -> the
    renderer's paint rule; panorama and coverage byte for byte."""
    pano, cov, geo = render6(rp, case, "maxweight", "APS_RENDER_LEGACY")
    sc = scene6()
    gains = mc.GAINS6 if case.gains else [(1.0, 1.0, 1.0)] * 6
    pieces = [rp.warp_tile(im, c, geo, 0, 0, geo["H"], geo["W"], 2.0, g) for im, c, g in zip(sc["imgs"], sc["cams"], gains)]
    want, wcov = mc.expected_maxweight(pieces, case.tile, case.levels, mc.SIGMA, case.white)
    assert wcov.sum() > 20000 and (wcov == 0).sum() > 100 and (mc.raw_weights(pieces) > 0).sum(0).max() >= 2
    assert np.array_equal(cov, wcov)
    assert np.array_equal(pano, want)


@ray_cases
def test_batched_path_with_per_tile_arithmetic_equals_the_per_tile_path(rp, case):
    ref, rcov, _ = render6(rp, case, "maxweight", "APS_RENDER_LEGACY")
    for switches in (("APS_WARP_EXACT",), ("APS_WARP_EXACT", "APS_RENDER_NO_CULL"), ("APS_WARP_EXACT", "APS_RENDER_DEVICE_COVER")):
        pano, cov, _ = render6(rp, case, "maxweight", *switches)
        assert np.array_equal(cov, rcov), switches
        assert np.array_equal(pano, ref), switches


@pytest.mark.parametrize("name,mode,power", [("fan12", "spherical", 2.0), ("fan12", "planar", 3.0), ("crowd40", "spherical", 2.0),
                                             ("crowd", "planar", 2.0), ("slivers", "spherical", 2.0)])
def test_deep_stacks_and_tiny_images_batched_equals_per_tile(rp, name, mode, power):
    """More than kWF = 8 layers on a block (the walking form), more than kWL = 6 (re-sampled layers), more than kMaxK = 16 and
    more than 64 layers in a tile (the per-tile partition without footprints; it has no cap), images under 4 px (the exact
    sampler inside the fast warp), and a power that sends every block through the walking form."""
    sc, st = rc.scene(name), rc.STATS[(name, mode)]
    assert {"fan12": st.max_block > rc.KWF, "crowd40": rc.KMAXK < st.max_tile <= rc.LEGACY_MB_MAX, "crowd": st.max_tile > rc.LEGACY_MB_MAX,
            "slivers": min(min(s[:2]) for s in sc.sizes) < 4}[name]

    def run(*switches):
        with Switches(*switches):
            pano, _, cov, _ = rp.renderPanorama({}, list(sc.images), list(sc.sizes), list(sc.cameras), mode, sc.ref_idx,
                                                rc.render_opts(sc, "multiband", power, multibandWeights="maxweight"),
                                                gains=list(sc.gains), return_covered=True, geo=rc.geometry(name, mode))
        return pano, cov

    ref, rcov = run("APS_RENDER_LEGACY")
    exact, ecov = run("APS_WARP_EXACT")
    assert rcov.sum() > 5000 and np.array_equal(ecov, rcov) and np.array_equal(exact, ref)
    nocull, ncov = run("APS_WARP_EXACT", "APS_RENDER_NO_CULL")
    assert np.array_equal(ncov, rcov) and np.array_equal(nocull, ref)
    fast, fcov = run()
    assert np.array_equal(fcov, rcov)
    with Switches():
        tent, _, tcov, _ = rp.renderPanorama({}, list(sc.images), list(sc.sizes), list(sc.cameras), mode, sc.ref_idx,
                                             rc.render_opts(sc, "multiband", power), gains=list(sc.gains), return_covered=True,
                                             geo=rc.geometry(name, mode))
    assert np.array_equal(tcov, rcov) and not np.array_equal(tent, fast)


@ray_cases
def test_coverage_is_the_tent_coverage_and_tent_mode_is_untouched(rp, case):
    for switches in ((), ("APS_RENDER_LEGACY",)):
        tent, tcov, _ = render6(rp, case, None, *switches)
        named, ncov, _ = render6(rp, case, "tent", *switches)
        mw, mcov, _ = render6(rp, case, "maxweight", *switches)
        assert np.array_equal(mcov, tcov), switches
        assert np.array_equal(named, tent) and np.array_equal(ncov, tcov), switches
        assert not np.array_equal(mw, tent), switches   # the key is not ignored


# ---- 5. the default (fast) warp against the exact one ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_world(gpu, rp):
    synth = import_module(gpu.__name__ + ".synth")
    views, cams = mc.one_world_views(synth, "cuda")
    sizes = [(mc.ONE_H, mc.ONE_W, 3)] * 3
    return views, cams, sizes


def test_fast_warp_against_the_exact_warp_away_from_near_ties(rp, one_world):
    """Three views of ONE synthetic world, 800 x 560, spherical, three levels, tiles of 256 x 320 (canvas 612 x 1706).
    T: the pixels whose two largest raw weights differ by at most ATOL_F32 = 2e-4 (there the fast and the exact warp may
    disagree about the owner), grown by the reach of the pure mask.  Outside it the bounds of
    test_batched_multiband_equals_per_tile_path hold unchanged.  Measured on the CPU with oracle.warp_tile before the scene was
    settled: T is 0.17 % of the covered pixels, its dilation 11.8 % (bound: under 15 %)."""
    views, cams, sizes = one_world
    with Switches():
        fast, _, fcov, geo = rp.renderPanorama({}, views, sizes, cams, "spherical", 1, mc.one_world_opts("maxweight"), return_covered=True)
    with Switches("APS_WARP_EXACT"):
        exact, _, ecov, _ = rp.renderPanorama({}, views, sizes, cams, "spherical", 1, mc.one_world_opts("maxweight"), return_covered=True)
    assert np.array_equal(fcov, ecov) and ecov.sum() > 500000
    pieces = [rp.warp_tile(v, c, geo, 0, 0, geo["H"], geo["W"], 2.0) for v, c in zip(views, cams)]
    W = mc.raw_weights(pieces)
    excluded = mc.reach_dilate(mc.near_ties(W, ATOL_F32), mc.ONE_TILE, mc.ONE_LEVELS, mc.SIGMA)
    covered = ecov == 1
    share = (excluded & covered).sum() / covered.sum()
    dd = np.abs(fast.astype(int) - exact.astype(int)).max(2)[covered & ~excluded]
    print(f"excluded share of the covered pixels {share:.4f}; outside: max {int(dd.max())}, within 1: {(dd <= 1).mean():.5f}, "
          f"equal: {(dd == 0).mean():.5f}")
    assert share < 0.15, share
    assert dd.max() <= 2 and (dd <= 1).mean() >= 0.9995, (int(dd.max()), (dd <= 1).mean())
    assert (dd == 0).mean() >= 0.97, (dd == 0).mean()


# ---- 7. what the feature is for ----------------------------------------------------------------------------------------------------
def test_a_disc_seen_by_one_view_is_kept_whole_and_tent_mode_ghosts_it(rp, one_world):
    """A white 15-px disc painted into view A only, inside its overlap with view B.  On the pure pixels the maxweight panorama
    is the owner's own sample within one grey level (float rounding of the telescoping sum); the tent panorama differs from
    both A's and B's sample on the disc by more than 20 grey levels (CPU oracle: at least 43 from A, 154 from B)."""
    views, cams, sizes = one_world
    views = [mc.paint_disc(views[0]), views[1], views[2]]
    with Switches("APS_WARP_EXACT"):   # the sampler of warp_tile, so that one grey level is rounding only
        mw, _, cov, geo = rp.renderPanorama({}, views, sizes, cams, "spherical", 1, mc.one_world_opts("maxweight"), return_covered=True)
    with Switches():
        tent, _, tcov, _ = rp.renderPanorama({}, views, sizes, cams, "spherical", 1, mc.one_world_opts(), return_covered=True)
    pieces = [rp.warp_tile(v, c, geo, 0, 0, geo["H"], geo["W"], 2.0) for v, c in zip(views, cams)]
    W = mc.raw_weights(pieces)
    covered = cov == 1
    assert np.array_equal(covered, (W > 0).any(0)) and np.array_equal(tcov, cov)
    pure = mc.pure_canvas(W, mc.ONE_TILE, mc.ONE_LEVELS, mc.SIGMA) & covered
    own = mm.paint(mm.owner_colour(np.stack([p[0] for p in pieces]), W), covered)
    assert 0.7 < pure.sum() / covered.sum() < 0.97
    assert np.abs(mw.astype(int) - own.astype(int)).max(2)[pure].max() <= 1
    SA, SB = mm.paint(pieces[0][0], covered), mm.paint(pieces[1][0], covered)
    disc = (SA.min(2) >= 250) & pieces[0][1] & pieces[1][1]
    assert disc.sum() >= 100 and pure[disc].all() and (mm.owner(W)[disc] == 0).all()
    assert np.abs(mw.astype(int) - SA.astype(int)).max(2)[disc].max() <= 1          # the disc is whole
    dA = np.abs(tent.astype(int) - SA.astype(int)).max(2)[disc]
    dB = np.abs(tent.astype(int) - SB.astype(int)).max(2)[disc]
    assert dA.min() > 20 and dB.min() > 20, (int(dA.min()), int(dB.min()))           # the ghost


# ---- 8. pipelines ------------------------------------------------------------------------------------------------------------------
def test_stitch_and_stitch_distributed_pass_the_key_on(gpu, rp):
    import torch

    synth = import_module(gpu.__name__ + ".synth")
    pl = import_module(gpu.__name__ + ".pipeline")
    par = import_module(gpu.__name__ + ".parallel")
    nx, ny, w, h, f = 3, 2, 640, 480, 900.0   # the scene of test_pipeline_gpu.py
    cams = synth.grid_cameras(nx, ny, w, h, f, 2 * np.arctan(w / (2 * f)) * 0.6, 2 * np.arctan(h / (2 * f)) * 0.6, 1.0, 7)
    views = [synth.render_view(cams[i], h, w, 7, "cuda", finest_px=6.0) for i in range(nx * ny)]
    torch.cuda.synchronize()
    Ks = [c["K"] for c in cams]
    inp = pl.default_input(bands=3, multibandWeights="maxweight")
    with Switches():
        panos, info = pl.stitch(inp, views, Ks, tile=(512, 512))
        assert info["n_components"] == 1 and len(panos) == 1
        c = info["components"][0]
        members = c["members"]
        opts = {"anglePower": 2, "blending": inp["blending"], "pyrLevels": inp["bands"], "pyrSigma": inp["MBBsigma"],
                "canvasColor": inp["canvasColor"], "tile": (512, 512), "cropBorder": True}
        sizes = [tuple(int(v) for v in views[k].shape) for k in members]
        direct = {wt: rp.renderPanorama(inp, [views[k] for k in members], sizes, c["cameras"], inp["panorama2DisplaynSave"], c["ref"],
                                        dict(opts, multibandWeights=wt))[0] for wt in ("maxweight", "tent")}
        got = panos[0].cpu().numpy()
        assert got.shape == direct["maxweight"].shape and np.array_equal(got, direct["maxweight"])
        assert not np.array_equal(got, direct["tent"])
        dpano, dinfo = par.stitch_distributed(inp, dict(enumerate(views)), nx * ny, Ks, (512, 512), 0, None, pano_root=0)
        torch.cuda.synchronize()
        assert dinfo["n_components"] == 1
        dc = dinfo["components"][0]
        dsizes = [tuple(int(v) for v in views[k].shape) for k in dc["members"]]
        ddirect = {wt: rp.renderPanorama(inp, [views[k] for k in dc["members"]], dsizes, dc["cameras"], inp["panorama2DisplaynSave"],
                                         dc["ref"], dict(opts, multibandWeights=wt))[0] for wt in ("maxweight", "tent")}
        assert np.array_equal(dpano.cpu().numpy(), ddirect["maxweight"]) and not np.array_equal(dpano.cpu().numpy(), ddirect["tent"])


def test_tile_subsets_compose_to_the_full_render(rp):
    imgs, cams = _scene(np.random.default_rng(22), n=5, W=220, H=140, f=300.0)
    sizes = [(140, 220, 3)] * 5
    opts = {"anglePower": 2, "blending": "multiband", "multibandWeights": "maxweight", "pyrLevels": 4, "pyrSigma": 1.0, "tile": (64, 80),
            "cropBorder": False}
    with Switches():
        full, _, cov, _ = rp.renderPanorama({}, imgs, sizes, cams, "spherical", 2, opts, return_covered=True)
        tent = rp.renderPanorama({}, imgs, sizes, cams, "spherical", 2, dict(opts, multibandWeights="tent"))[0]
        parts = [rp.renderPanorama({}, imgs, sizes, cams, "spherical", 2, opts, return_covered=True, tile_subset=(k, 2)) for k in range(2)]
    assert np.array_equal(np.maximum(parts[0][0], parts[1][0]), full)
    assert np.array_equal(np.maximum(parts[0][2], parts[1][2]), cov)
    assert not np.any((parts[0][2] == 1) & (parts[1][2] == 1)) and not np.array_equal(full, tent)
