"""Scenes, case table and expected pictures of test_maxweight_gpu.py (helper, not a test).  numpy and the oracle only; the
warp pieces (Wang, Wf, S per view) come from the caller, who takes them from renderPanorama.warp_tile on the device or from
oracle.warp_tile on the CPU."""
from collections import namedtuple

import numpy as np

import maxweight_mirror as mm
import oracle

# ---- ray canvases: the cases of tests 3, 4 and 6 (scene: test_render_gpu._scene(rng(21), n=6, W=220, H=140, f=300)) ----------
RayCase = namedtuple("RayCase", "mode levels tile gains white")
GAINS6 = [(1.0, 1.0, 1.0), (0.9, 1.1, 1.0), (1.2, 0.8, 1.0), (1.0, 1.0, 0.7), (1.05, 1.0, 0.95), (1, 1, 1)]
RAY_CASES = (
    RayCase("spherical", 3, (64, 64), False, False),
    RayCase("cylindrical", 6, (33, 47), True, True),     # 33 rows: the level count is clamped to 5
    RayCase("planar", 1, (100, 130), True, False),
    RayCase("stereographic", 3, (33, 47), False, True),
    RayCase("fisheye", 6, (100, 130), True, False),
    RayCase("spherical", 1, (33, 47), False, False),
    RayCase("spherical", 6, (64, 64), True, False),      # 64 rows: six levels exactly
)
SIGMA = 1.0


def ray_id(c):
    return f"{c.mode}-L{c.levels}-{c.tile[0]}x{c.tile[1]}" + ("-gains" if c.gains else "") + ("-white" if c.white else "")


def ray_opts(c, weights=None, **more):
    o = {"anglePower": 2, "blending": "multiband", "pyrLevels": c.levels, "pyrSigma": SIGMA, "tile": c.tile, "cropBorder": False,
         "canvasColor": "white" if c.white else "black", "margin": 0.08}
    if weights is not None:
        o["multibandWeights"] = weights
    o.update(more)
    return o


def tiles_of(H, W, tile):
    return [(r0, c0, min(tile[0], H - r0), min(tile[1], W - c0)) for r0 in range(0, H, tile[0]) for c0 in range(0, W, tile[1])]


def raw_weights(pieces):
    """pieces: per view (S, M, Wang, Wf) over the whole canvas.  The raw weight of the contract: Wang * Wf as one f32 product
    under the mask, else 0."""
    return np.stack([np.where(M, Wa * Wf, np.float32(0)).astype(np.float32) for _, M, Wa, Wf in pieces])


def expected_maxweight(pieces, tile, levels, sigma, white):
    """The contract's picture from pieces: per tile the mirror partition of the raw weights -> oracle.multiband_blend -> the
    renderer's paint rule.  Returns (panorama uint8, coverage uint8)."""
    W = raw_weights(pieces)
    C = np.stack([p[0] for p in pieces])
    _, H, Wd = W.shape
    pano = np.zeros((H, Wd, 3), np.uint8)
    with np.errstate(invalid="ignore"):
        cov = (W > 0).any(0)
    for r0, c0, ht, wt in tiles_of(H, Wd, tile):
        sl = (slice(r0, r0 + ht), slice(c0, c0 + wt))
        Wt = W[(slice(None),) + sl]
        if not cov[sl].any():
            pano[sl] = 255 if white else 0
            continue
        F = oracle.multiband_blend(np.ascontiguousarray(C[(slice(None),) + sl]), mm.partition(Wt), levels, sigma)
        pano[sl] = mm.paint(F, cov[sl], white)
    return pano, cov.astype(np.uint8)


def pure_canvas(W, tile, levels, sigma):
    """mm.pure_mask tile by tile over a canvas of raw weights W (K x H x W)."""
    _, H, Wd = W.shape
    out = np.zeros((H, Wd), bool)
    for r0, c0, ht, wt in tiles_of(H, Wd, tile):
        out[r0:r0 + ht, c0:c0 + wt] = mm.pure_mask(mm.partition(W[:, r0:r0 + ht, c0:c0 + wt]), levels, sigma)
    return out


def near_ties(W, atol):
    """T of test 5: the pixels whose two largest raw weights differ by at most atol (a pixel under one view: that view's
    weight against 0)."""
    top = np.sort(np.nan_to_num(np.concatenate([W, np.zeros_like(W[:1])]), nan=0.0), axis=0)
    return (top[-1] - top[-2]) <= atol


def reach_dilate(T, tile, levels, sigma):
    """T grown by the reach of the pure mask: T and its complement go through the pyramid's weight chain as two binary layers,
    tile by tile; whatever is not pure there lies within the blend's reach of T's boundary."""
    B = np.stack([T, ~T]).astype(np.float32)
    return T | ~pure_canvas(B, tile, levels, sigma)


# ---- one world, several views: tests 5 and 7 -------------------------------------------------------------------------------
ONE_W, ONE_H, ONE_F, ONE_SEED = 800, 560, 1040.0, 11
ONE_TILE, ONE_LEVELS = (256, 320), 3
DISC_DIAMETER, DISC_CENTRE = 15, (280, 540)   # (row, column) in view A, inside its overlap with view B


def one_world_cameras():
    from test_render_oracle import cam

    return [cam(ONE_F, ONE_W, ONE_H, yaw=(i - 1) * 0.42, pitch=0.02 * (-1) ** i) for i in range(3)]


def one_world_views(synth, device="cpu"):
    """Three overlapping views of ONE synthetic world (synth.render_view), dimmed so that a white disc stands out."""
    cams = one_world_cameras()
    views = []
    for c in cams:
        v = synth.render_view(c, ONE_H, ONE_W, ONE_SEED, device, gain=0.6, finest_px=6.0)
        views.append(np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v))
    return views, cams


def paint_disc(view):
    out = view.copy()
    yy, xx = np.mgrid[0:view.shape[0], 0:view.shape[1]]
    out[(yy - DISC_CENTRE[0]) ** 2 + (xx - DISC_CENTRE[1]) ** 2 <= (DISC_DIAMETER / 2.0) ** 2] = 255
    return out


def one_world_opts(weights=None, **more):
    o = {"anglePower": 2, "blending": "multiband", "pyrLevels": ONE_LEVELS, "pyrSigma": SIGMA, "tile": ONE_TILE,
         "cropBorder": False, "margin": 0.02}
    if weights is not None:
        o["multibandWeights"] = weights
    o.update(more)
    return o
