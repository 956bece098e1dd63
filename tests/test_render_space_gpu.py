"""The render across the parameter space the rest of the suite never enters (render_space_cases.py; test_render_space_cases.py
holds the scenes to their arms on the CPU): angle powers other than 2 - 1 is the default of renderPanorama - views of different
sizes, a gray one, fx != fy, off-centre principal points, rolled cameras, twelve views on one pixel, more than 128 entries in
one tile, a stack across theta = +-pi, images of two and three rows or columns, and the blend operators above 16 layers.

Every whole render is compared five ways, each at the tolerance the project already states for it:
  default batched path   against oracle.render    the tolerance of test_render_gpu's module docstring: coverage differs on at most
                                                  0.1 % of the pixels, at least 99.8 % within one grey level and, for the blended
                                                  modes, at most 2 on every pixel both sides cover
  APS_WARP_EXACT=1       against the per-tile path (APS_RENDER_LEGACY=1): every byte of panorama and coverage
  default                against APS_WARP_EXACT=1: the bounds of test_batched_multiband_equals_per_tile_path (equal coverage,
                                                  at most 2, at least 99.95 % within 1)
  APS_RENDER_DEVICE_COVER=1 against default:      every byte
  APS_RENDER_CHECK_RECTS=1: the library checks its analytic footprints against the exact ones inside the call and raises if one
                                                  leaves its rectangle; the bytes are the default's
No bound here was measured on the code under test.  The one arm the library refuses - more than 64 layers in one tile on the
per-tile multiband path (APS_E_DIM) - is pinned as a refusal; `crowd` meets it, and there the exact warp is compared with the
oracle instead, `crowd40` (40 layers in the tile) and crowd's 'linear' renders make the byte comparison."""
from importlib import import_module

import numpy as np
import pytest

import oracle
import render_space_cases as rc

pytestmark = pytest.mark.gpu

ATOL_F32 = 2e-4
SWITCHES = ("APS_RENDER_LEGACY", "APS_WARP_EXACT", "APS_RENDER_DEVICE_COVER", "APS_RENDER_CHECK_RECTS", "APS_RENDER_NO_CULL",
            "APS_RENDER_NO_FUSE")


@pytest.fixture(scope="module")
def rp(gpu):
    return import_module(gpu.__name__ + ".renderPanorama")


@pytest.fixture(scope="module")
def bl(gpu):
    return import_module(gpu.__name__ + ".blending")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- a. warp_tile ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", rc.POWERS_WARP)
@pytest.mark.parametrize("mode", rc.MODES)
def test_warp_tile_at_other_powers_within_tolerance(rp, mode, power):
    """aps_warp_tile (sample_one: project()'s powf arm, 1 and 0 included) against oracle.warp_tile for a view rolled by 3.5 rad
    with fx != fy and an off-centre principal point and for the gray view; the assertions of test_warp_tile_within_tolerance."""
    sc, geo = rc.scene("fan12"), rc.warp_geometry(mode)
    (r0, c0), ht, wt = rc.WARP_ORIGIN, geo["H"] - rc.WARP_ORIGIN[0], geo["W"] - rc.WARP_ORIGIN[1]
    for k in rc.WARP_VIEWS:
        img, c, g = sc.images[k], sc.cameras[k], sc.gains[k]
        S, M, Wa, Wf = rp.warp_tile(img, c, geo, r0, c0, ht, wt, power, gain=g)
        oS, oM, oWa, oWf = oracle.warp_tile(img, c, geo, r0, c0, ht, wt, power, gain=g)
        both = M & oM
        dS = np.abs(S[both] - oS[both])
        print(f"warp_tile {mode} p={power:g} view {k}: mask {int(oM.sum())} flips {int((M != oM).sum())} "
              f"dWa {np.abs(Wa[both] - oWa[both]).max():.3g} dWf {np.abs(Wf[both] - oWf[both]).max():.3g} "
              f"dS max {dS.max():.3g} mean {dS.mean():.3g}")
        assert oM.sum() > 3000
        assert (M != oM).mean() <= 1e-3
        np.testing.assert_allclose(Wa[both], oWa[both], atol=ATOL_F32)
        np.testing.assert_allclose(Wf[both], oWf[both], atol=ATOL_F32)
        assert dS.max() <= 5e-3
        assert dS.mean() <= ATOL_F32
        assert np.all(S[~M] == 0) and np.all(Wa[~M] == 0) and np.all(Wf[~M] == 0)
        if power == 0.0:
            assert np.all(Wa[M] == 1.0)


# ---- b, c. whole renders -----------------------------------------------------------------------------------------------------------
def render(rp, monkeypatch, case, *switches):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s in switches:
        monkeypatch.setenv(s, "1")
    sc = rc.scene(case.scene)
    # on the canvas the oracle's picture was rendered on (check_case holds the wrapper's own canvas to it)
    pano, _, cov, _ = rp.renderPanorama({}, list(sc.images), list(sc.sizes), list(sc.cameras), case.mode, sc.ref_idx,
                                        rc.render_opts(sc, case.blending, case.power), gains=list(sc.gains), return_covered=True,
                                        geo=rc.geometry(case.scene, case.mode))
    for s in switches:
        monkeypatch.delenv(s)
    return pano, cov


def against_oracle(label, case, pano, cov):
    """The tolerance of test_render_gpu's module docstring."""
    op, oc = rc.oracle_render(*case)
    both = (cov == 1) & (oc == 1)
    diff = np.abs(pano.astype(int) - op.astype(int))[both]
    print(f"{rc.case_id(case)} {label} against the oracle: coverage differs on {int((cov != oc).sum())} of {cov.size}, "
          f"max {int(diff.max())}, within 1: {(diff <= 1).mean():.5f}, above 1: {int((diff > 1).sum())}")
    assert pano.shape == op.shape
    assert (cov != oc).mean() <= 1e-3
    assert (diff <= 1).mean() >= 0.998
    if case.blending != "none":
        assert diff.max() <= 2, int(diff.max())
    assert np.all(pano[cov == 0] == 0)


def check_case(gpu, rp, monkeypatch, case):
    sc, st, want = rc.scene(case.scene), rc.STATS[(case.scene, case.mode)], rc.geometry(case.scene, case.mode)
    # the wrapper sizes the same canvas as the oracle (origins in f64: the last bit may differ, the device takes them as f32)
    o = rp.default_opts(rc.render_opts(sc, case.blending, case.power), list(sc.cameras), sc.ref_idx)
    geo = rp.canvas_geometry(list(sc.cameras), list(sc.sizes), case.mode, sc.ref_idx, o)
    assert (geo["H"], geo["W"]) == st.canvas and geo["refIdx"] == want["refIdx"] and geo["fPan"] == want["fPan"]
    assert abs(geo["o0"] - want["o0"]) <= 1e-12 and abs(geo["o1"] - want["o1"]) <= 1e-12
    fast, fcov = render(rp, monkeypatch, case)
    assert fcov.sum() > 5000 and (fcov == 0).sum() > 100
    against_oracle("default", case, fast, fcov)
    exact, ecov = render(rp, monkeypatch, case, "APS_WARP_EXACT")
    if case.blending == "multiband" and st.max_tile > rc.LEGACY_MB_MAX:
        # the per-tile multiband keeps one mask bit per layer of a tile and refuses more than 64
        with pytest.raises(gpu.ApsError) as e:
            render(rp, monkeypatch, case, "APS_RENDER_LEGACY")
        assert e.value.code == gpu._capi.APS_E_DIM
        against_oracle("exact warp", case, exact, ecov)
    else:
        ref, rcov = render(rp, monkeypatch, case, "APS_RENDER_LEGACY")
        assert np.array_equal(ecov, rcov)
        assert np.array_equal(exact, ref)
    assert np.array_equal(fcov, ecov)
    dd = np.abs(fast.astype(int) - exact.astype(int))[fcov == 1]
    print(f"{rc.case_id(case)} default against the exact warp: max {int(dd.max())}, within 1: {(dd <= 1).mean():.5f}, "
          f"equal: {(dd == 0).mean():.5f}")
    assert dd.max() <= 2 and (dd <= 1).mean() >= 0.9995, (int(dd.max()), (dd <= 1).mean())
    dev, dcov = render(rp, monkeypatch, case, "APS_RENDER_DEVICE_COVER")
    assert np.array_equal(dcov, fcov) and np.array_equal(dev, fast)
    chk, ccov = render(rp, monkeypatch, case, "APS_RENDER_CHECK_RECTS")  # raises if a footprint leaves its rectangle
    assert np.array_equal(ccov, fcov) and np.array_equal(chk, fast)


@pytest.mark.parametrize("case", rc.FAN_CASES, ids=rc.case_id)
def test_fan12_renders_at_powers_other_than_two(gpu, rp, monkeypatch, case):
    """Twelve views of four sizes, one gray, fx != fy, rolled, on one pixel: powers 1 (the staged warp's `wa = cam2` arm), 0.5
    and 3 (__powf in sample_fast, every block through the walking form), blocks of more than kWF and kWL layers (the re-sampling
    of passes B and C), rw_fuse_kernel for 'linear' and 'none'."""
    check_case(gpu, rp, monkeypatch, case)


@pytest.mark.parametrize("case", rc.OTHER_CASES, ids=rc.case_id)
def test_seam_crowd_and_slivers_render_at_the_default_power(gpu, rp, monkeypatch, case):
    """seam: a stack across theta = +-pi against the oracle.  crowd: 140 entries in one tile, the plain loop of
    for_block_layers at every level (and the refusal of the per-tile multiband above 64 layers); crowd40: 40 layers, the
    per-tile path's pointer table without footprints.  slivers: images of two and three rows or columns (sample_one on the
    exact ray) and the 4 x 4 one, the smallest the fast sampler takes."""
    check_case(gpu, rp, monkeypatch, case)


# ---- d. the blend operators above kMaxK layers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 17, 33])
def test_blend_operators_above_sixteen_layers_are_bit_exact(bl, monkeypatch, K):
    """aps_multiband_blend chunks its layers by kMaxK = 16 per launch and normalises above 16 through an uploaded pointer
    table; aps_linear_blend sums K layers in order: the oracle's bits for 16, 17 and 33 layers, fused and unfused."""
    h, w, levels = 33, 47, 4
    rng = np.random.default_rng(160 + K)
    C = rng.random((K, h, w, 3), dtype=np.float32)
    W = rng.random((K, h, w), dtype=np.float32)
    W[:, : h // 3, : w // 2] = 0            # a corner no layer covers
    for k in range(K):                      # disjoint column strips and overlapping row bands of zero weight
        W[k, :, (3 * k) % w: (3 * k) % w + 3] = 0
        if k % 2:
            W[k, (k % 5) * 4: (k % 5) * 4 + 14] = 0
    W[K - 1, :, w // 2:] = 0
    depth = (W > 0).sum(0)
    assert (depth > 0).mean() > 0.5 and (depth == 0).any() and depth.max() > K // 2 and len(np.unique(depth)) > 4
    O = oracle.multiband_blend(C, W, levels, 1.0)
    OL = oracle.linear_blend(C, W)
    for fuse in (True, False):
        if fuse:
            monkeypatch.delenv("APS_RENDER_NO_FUSE", raising=False)
        else:
            monkeypatch.setenv("APS_RENDER_NO_FUSE", "1")
        F = bl.multiBandBlending(list(C), list(W), levels, True, 1.0)
        L = bl.linearBlending(list(C), list(W))
        assert np.array_equal(bits(F), bits(O)), fuse
        assert np.array_equal(bits(L), bits(OL)), fuse
    monkeypatch.delenv("APS_RENDER_NO_FUSE", raising=False)


# ---- e. gain statistics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["spherical", "planar"])
def test_gain_overlap_stats_of_fan12_match_oracle(gpu, rp, mode):
    """aps_gain_overlap_stats on twelve views of four sizes, one gray, on the canvas the default options (anglePower 1) give;
    the comparison of test_gain_overlap_stats_match_oracle: counts up to border flips, pair means and solved gains relative."""
    gc = import_module(gpu.__name__ + ".gainCompensation")
    sc = rc.scene("fan12")
    imgs, cams, sizes, n = list(sc.images), list(sc.cameras), list(sc.sizes), len(sc.images)
    o = rp.default_opts({"anglePower": 1, "margin": rc.MARGIN}, cams, sc.ref_idx)
    geo = rp.canvas_geometry(cams, sizes, mode, sc.ref_idx, o)
    assert (geo["H"], geo["W"]) == rc.STATS[("fan12", mode)].canvas
    Nij, sCi, sCj = gc.gain_overlap_stats(imgs, cams, geo, 3)
    oN, oI, oJ = oracle.gain_overlap_stats(imgs, cams, geo, 3)
    print(f"gain stats {mode}: samples {int(oN.sum())}, count differences {int(np.abs(Nij - oN).sum())}, pairs >= 50: {int((oN >= 50).sum())}")
    assert Nij.shape == (n, n) and np.all(np.tril(Nij) == 0) and oN.sum() > 500
    assert np.abs(Nij - oN).sum() <= 2e-3 * oN.sum()
    big = oN >= 50
    assert big.sum() >= 3
    assert np.allclose((sCi / np.maximum(Nij, 1)[..., None])[big], (oI / np.maximum(oN, 1)[..., None])[big], rtol=2e-3)
    assert np.allclose((sCj / np.maximum(Nij, 1)[..., None])[big], (oJ / np.maximum(oN, 1)[..., None])[big], rtol=2e-3)
    g = gc.solve_gains(Nij, sCi, sCj, {"minOverlapSamples": 50})
    go = gc.solve_gains(oN, oI, oJ, {"minOverlapSamples": 50})
    assert g.shape == (n, 3) and np.allclose(g, go, rtol=2e-3) and np.all((g >= 0.25) & (g <= 4.0))
