"""Keeps the render parameter space honest (CPU, oracle only): every scene of render_space_cases still reaches the arm of the
render it was built for - enough views on one pixel, in one 32 x 8 block and in one tile, masks of the tiny views, a stack
across the seam - and the canvases and counts the scenes were chosen for are pinned as the properties of seeded inputs they
are.  When a constant of the kernels (kWL, kWF, kLM, kMaxK) or a scene changes, this says which case stopped covering its arm;
without it the GPU test would go on passing while testing something else."""
import numpy as np
import pytest

import oracle
import render_space_cases as rc


@pytest.mark.parametrize("name,mode", rc.SCENE_MODES, ids=lambda v: str(v))
def test_scene_statistics_are_the_pinned_ones(name, mode):
    sc, geo, m = rc.scene(name), rc.geometry(name, mode), rc.masks(name, mode)
    depth = m.sum(0)
    st = rc.STATS[(name, mode)]
    got = rc.Stats((geo["H"], geo["W"]), int((depth > 0).sum()), int((depth >= 9).sum()), int(rc.block_counts(m, sc.tile).max()),
                   int(rc.tile_counts(m, sc.tile).max()))
    assert got == st
    # every canvas has covered and void area
    assert st.covered > 5000 and st.canvas[0] * st.canvas[1] - st.covered > 100
    # the sizes the GPU tests may take: nothing above fan12's planar canvas
    assert st.canvas[0] * st.canvas[1] <= 308 * 412
    assert len(sc.images) == len(sc.cameras) == len(sc.sizes) == len(sc.gains)
    assert all(tuple(g) != (1.0, 1.0, 1.0) for g in sc.gains)


@pytest.mark.parametrize("mode", rc.MODES)
def test_fan12_stacks_views_past_the_parked_and_the_staged_layers(mode):
    sc, m = rc.scene("fan12"), rc.masks("fan12", mode)
    st = rc.STATS[("fan12", mode)]
    assert len(sc.images) == 12 and sc.images[rc.FAN_GRAY].ndim == 2 and sum(im.ndim == 2 for im in sc.images) == 1
    assert {im.shape[:2] for im in sc.images} == set(rc.FAN_SIZES)
    assert all(c["K"][0, 0] != c["K"][1, 1] and c["K"][0, 2] != im.shape[1] / 2 for c, im in zip(sc.cameras, sc.images))
    assert st.deep >= 400                      # pixels under nine or more views
    assert int(m.sum(0).max()) == 12           # and some under all twelve
    # a block met by more views than the walking form parks (kWL) and than the staged form takes (kWF): with twelve views
    # that is all a block can ask for; more than kMaxK layers in a tile is crowd40's and crowd's business (below)
    assert st.max_block > rc.KWF > rc.KWL
    assert st.max_tile <= rc.KMAXK             # the per-tile path keeps its footprints here


@pytest.mark.parametrize("mode", ["spherical", "planar"])
def test_crowd_fills_one_tile_past_the_listed_entries(mode):
    for name in ("crowd", "crowd40"):
        sc, st = rc.scene(name), rc.STATS[(name, mode)]
        assert st.canvas[0] <= sc.tile[0] and st.canvas[1] <= sc.tile[1]     # the canvas is one tile
        assert st.canvas[0] <= 256 and st.canvas[1] <= 320
        assert all(36 <= s[0] <= 48 and 40 <= s[1] <= 53 for s in sc.sizes)
    crowd, c40 = rc.STATS[("crowd", mode)], rc.STATS[("crowd40", mode)]
    assert len(rc.scene("crowd").images) >= 136
    assert crowd.max_tile >= rc.LISTED_MAX + 1                               # the plain loop of for_block_layers
    assert crowd.max_tile > rc.LEGACY_MB_MAX                                 # the per-tile multiband refuses this tile
    assert rc.KMAXK < c40.max_tile <= rc.LEGACY_MB_MAX                       # pointer table, no footprints, still rendered
    # at least one aligned block met by more than 16 views' masks
    assert crowd.max_block > 16 and c40.max_block > 16
    # crowd40 is the head of crowd
    a, b = rc.scene("crowd"), rc.scene("crowd40")
    assert all(np.array_equal(x, y) for x, y in zip(a.images[:40], b.images))
    assert all(np.array_equal(x["R"], y["R"]) for x, y in zip(a.cameras[:40], b.cameras))


@pytest.mark.parametrize("mode", ["spherical", "planar"])
def test_slivers_tiny_views_have_masks_inside_the_other_views(mode):
    sc, m = rc.scene("slivers"), rc.masks("slivers", mode)
    assert tuple(im.shape[:2] for im in sc.images[4:]) == rc.TINY_SHAPES
    tiny = tuple(int(v.sum()) for v in m[4:])
    assert tiny == rc.TINY_PIXELS[mode] and min(tiny) > 0
    others = m[:4].any(0)
    for v in m[4:]:
        assert (v & others).sum() >= 0.9 * v.sum()


def test_seam_views_lie_on_both_sides_of_the_canvas():
    m = rc.masks("seam", "spherical")
    q = m.shape[2] // 4
    both = [bool(v[:, :q].any() and v[:, -q:].any()) for v in m]
    assert any(both) and all(both)
    a, b = rc.scene("seam"), rc.scene("fan12")
    assert all(np.array_equal(x, y) for x, y in zip(a.images, b.images[:6]))


def test_case_tables_cover_every_mode_blending_and_power():
    fan = rc.FAN_CASES
    assert {c.mode for c in fan} == set(rc.MODES)
    assert {c.blending for c in fan} == {"multiband", "linear", "none"}
    assert {c.power for c in fan} == set(rc.POWERS_RENDER) and 2.0 not in rc.POWERS_RENDER
    assert {c.mode for c in fan if c.blending == "multiband"} == set(rc.MODES)
    assert len(set(fan + rc.OTHER_CASES)) == len(fan) + len(rc.OTHER_CASES)
    other = {(c.scene, c.mode, c.blending) for c in rc.OTHER_CASES}
    assert all(c.power == 1.0 for c in rc.OTHER_CASES)
    for sc, modes in (("seam", ("spherical",)), ("crowd", ("spherical", "planar")), ("slivers", ("spherical",))):
        for mode in modes:
            assert (sc, mode, "multiband") in other and (sc, mode, "linear") in other
    assert set(rc.POWERS_WARP) == {0.0, 0.5, 1.0, 3.0, 7.25}


# ---- oracle self-consistency that needs no device ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.MODES)
def test_oracle_angle_weight_follows_the_power(mode):
    """Wang = max(cam_z, 0)^p (renderPanorama.m:1118-1124): 1 exactly for p = 0 wherever the mask is set, cam_z for p = 1 and
    that to the power p otherwise; colours, mask and tent weight do not depend on p."""
    sc, geo = rc.scene("fan12"), rc.warp_geometry(mode)
    (r0, c0), ht, wt = rc.WARP_ORIGIN, geo["H"] - rc.WARP_ORIGIN[0], geo["W"] - rc.WARP_ORIGIN[1]
    for k in rc.WARP_VIEWS:
        S1, M1, Wa1, Wf1 = oracle.warp_tile(sc.images[k], sc.cameras[k], geo, r0, c0, ht, wt, 1.0, sc.gains[k])
        assert M1.sum() > 3000 and 0.3 < Wa1[M1].min() < Wa1[M1].max() <= 1.0
        for p in rc.POWERS_WARP:
            S, M, Wa, Wf = oracle.warp_tile(sc.images[k], sc.cameras[k], geo, r0, c0, ht, wt, p, sc.gains[k])
            assert np.array_equal(M, M1) and np.array_equal(S, S1) and np.array_equal(Wf, Wf1)
            assert np.all(Wa[~M] == 0)
            if p == 0.0:
                assert np.all(Wa[M] == 1.0)
            else:
                np.testing.assert_allclose(Wa[M], Wa1[M].astype(np.float64) ** p, rtol=1e-6)


@pytest.mark.parametrize("mode", rc.MODES)
def test_oracle_renders_differ_between_the_powers(mode):
    """A blended render at power 1 differs from the one at power 3 (and 0.5): otherwise the power cases test nothing.
    ('none' with the policy 'maxangle' takes the view of the largest angle weight, which every positive power leaves in
    place: there the power cases check that the comparison survives powf, not that the picture changes.)"""
    for blending in ("multiband", "linear"):
        p1, c1 = rc.oracle_render("fan12", mode, blending, 1.0)
        for p in (0.5, 3.0):
            pp, cp = rc.oracle_render("fan12", mode, blending, p)
            assert np.array_equal(c1, cp)
            assert (p1 != pp).any(axis=2).sum() > 500, (blending, p)
    n1, _ = rc.oracle_render("fan12", mode, "none", 1.0)
    n3, _ = rc.oracle_render("fan12", mode, "none", 3.0)
    assert (n1 != n3).any(axis=2).mean() < 0.01
