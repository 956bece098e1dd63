"""The render parameter space of test_render_space_gpu.py (helper, not a test): seeded scenes, the case table and the arm
of csrc/render_batch.hip / render.hip / render_dev.h each case is there for.  numpy only; the oracle is imported where a
function needs it.

Arms (the constants are restated from the sources; test_render_space_cases.py holds every scene to its arm):
  anglePower  project() / sample_fast take w = cam_z (1), cam_z^2 (2) or powf / __powf (any other); rw_warp_staged_kernel
              stages a block only for 1 and 2, so any other power sends every block through warp_block_walk<true>
  kWL = 6     layers of a 32 x 8 block the walking form parks in LDS; further ones are sampled again in passes B and C
  kWF = 8     layers of a block the staged form takes; above, the walking form
  64 kLM      = 128 entries of a tile listed as bit masks; above, for_block_layers (the warp, rw_fuse_kernel) takes the plain loop
  kMaxK = 16  layers of a tile the per-tile path (APS_RENDER_LEGACY=1) passes as kernel arguments with footprints; above, an
              uploaded pointer table and whole-tile layers.  Its multiband normalisation keeps one mask bit per layer and
              refuses more than 64 layers in a tile (APS_E_DIM); 'linear' has no such limit
  small image fewer than four rows or columns: sample_one on the exact ray instead of sample_fast (closed-form tent, tap pairs)

Scenes (content: random 8 x 8 blocks as test_render_gpu._scene, so that the tolerance of that module's docstring applies):
  fan12    12 views fanned around one direction: four sizes, one gray view, fx != fy, off-centre principal point, roll
  seam     fan12's first six views turned by 3.1 rad: the stack straddles theta = +-pi (spherical)
  crowd    140 views of about 40 x 48 on one canvas that is a single tile: more than 128 entries in the tile
  crowd40  crowd's first 40 views on the same kind of canvas: 17 .. 64 layers in the tile, which the per-tile multiband takes
  slivers  four ordinary views and views of 2 x 37, 41 x 3, 3 x 3 and 4 x 4 pixels inside their footprint"""
import functools
import math
from collections import namedtuple

import numpy as np

KWL, KWF, LISTED_MAX, KMAXK, LEGACY_MB_MAX = 6, 8, 128, 16, 64
BLOCK_W, BLOCK_H = 32, 8  # kUW x kUH: the warp's block

MODES = ("spherical", "cylindrical", "planar", "stereographic")
TILE = (96, 128)
CROWD_TILE = (256, 320)  # at least the canvas: one tile
LEVELS, SIGMA = 4, 1.0
MARGIN = 0.05

POWERS_RENDER = (1.0, 0.5, 3.0)
POWERS_WARP = (0.0, 0.5, 1.0, 3.0, 7.25)

FAN_SIZES = ((96, 128), (90, 120), (128, 96), (75, 131))
FAN_GRAY = 3
TINY_SHAPES = ((2, 37), (41, 3), (3, 3), (4, 4))

Scene = namedtuple("Scene", "name images cameras sizes gains ref_idx tile f_pan auto_ref")


def rot(yaw, pitch, roll):
    """R = (Ry(yaw) Rx(pitch) Rz(roll))', world -> camera."""
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1.0]])
    return (Ry @ Rx @ Rz).T


def blocks(rng, h, w, gray=False):
    """Random 8 x 8 blocks (test_render_gpu._scene's content), h x w x 3 or h x w uint8."""
    base = rng.random((h // 8 + 2, w // 8 + 2, 3))
    img = (np.kron(base, np.ones((8, 8, 1)))[:h, :w] * 255).astype(np.uint8)
    return np.ascontiguousarray(img[..., 1]) if gray else img


def _freeze(images):
    for im in images:
        im.setflags(write=False)
    return tuple(images)


def _sizes(images):
    return tuple((im.shape[0], im.shape[1], 1 if im.ndim == 2 else im.shape[2]) for im in images)


def _gains(n):
    """One triple per view, none of them all ones."""
    return tuple((1.0 + 0.04 * ((k % 5) - 2), 1.0 - 0.03 * ((k % 3) - 1), 0.88 + 0.05 * (k % 4)) for k in range(n))


def fan_camera(k, h, w, yaw_offset=0.0):
    f = 150.0 + 10.0 * (k % 3)
    K = np.array([[f, 0, w / 2 + 3.5], [0, 1.07 * f, h / 2 - 2.25], [0, 0, 1.0]])
    return {"K": K, "R": rot(0.06 * (k - 5.5) + yaw_offset, 0.05 * ((5 * k) % 7 - 3), 0.5 * k)}


@functools.lru_cache(maxsize=None)
def scene(name):
    """The seeded scene `name`, built once, images read-only."""
    if name in ("fan12", "seam"):
        n, off = (12, 0.0) if name == "fan12" else (6, 3.1)
        rng = np.random.default_rng(1201)
        images, cams = [], []
        for k in range(n):
            h, w = FAN_SIZES[k % 4]
            images.append(blocks(rng, h, w, gray=(k == FAN_GRAY)))
            cams.append(fan_camera(k, h, w, off))
        # seam: the spherical canvas spans the whole circle; a smaller fPan keeps it below the planar canvas of fan12
        return Scene(name, _freeze(images), tuple(cams), _sizes(images), _gains(n), 5, TILE, None if name == "fan12" else 110.0, True)
    if name in ("crowd", "crowd40"):
        n = 140 if name == "crowd" else 40
        rng = np.random.default_rng(1402)
        shapes = ((40, 48), (37, 53), (44, 41), (48, 40))
        images, cams = [], []
        for k in range(140):
            h, w = shapes[k % 4]
            img = blocks(rng, h, w, gray=(k % 9 == 4))
            yaw, pitch, roll = rng.uniform(-0.30, 0.30), rng.uniform(-0.20, 0.20), rng.uniform(-math.pi, math.pi)
            f = 200.0 + 10.0 * (k % 3)
            K = np.array([[f, 0, w / 2 + 0.75], [0, 0.95 * f, h / 2 - 0.5], [0, 0, 1.0]])
            if k < n:
                images.append(img)
                cams.append({"K": K, "R": rot(yaw, pitch, roll)})
        # crowd: the reference view is named (it is the one the automatic choice arrives at, after 140 x 140 bounds
        # evaluations on the host): the planar canvas is the same and the test does not wait for the search
        ref, auto = (75, False) if name == "crowd" else (0, True)
        return Scene(name, _freeze(images), tuple(cams), _sizes(images), _gains(n), ref, CROWD_TILE, None, auto)
    if name == "slivers":
        rng = np.random.default_rng(803)
        images, cams = [], []
        for k in range(4):
            h, w = FAN_SIZES[k]
            images.append(blocks(rng, h, w))
            cams.append(fan_camera(k + 3, h, w))
        # the tiny views: focal lengths that spread the two or three pixels of a short side over some twenty canvas pixels
        tiny = (((2, 37), 120.0, 8.0, 0.05, 0.04, 0.3), ((41, 3), 10.0, 130.0, -0.10, -0.05, -0.2),
                ((3, 3), 12.0, 12.0, 0.12, -0.12, 0.7), ((4, 4), 15.0, 18.0, -0.02, 0.15, -1.1))
        for (h, w), fx, fy, yaw, pitch, roll in tiny:
            images.append(blocks(rng, h, w))
            K = np.array([[fx, 0, (w + 1) / 2 + 0.2], [0, fy, (h + 1) / 2 - 0.1], [0, 0, 1.0]])
            cams.append({"K": K, "R": rot(yaw, pitch, roll)})
        return Scene(name, _freeze(images), tuple(cams), _sizes(images), _gains(8), 1, TILE, None, True)
    raise KeyError(name)


def render_opts(sc, blending, power, **more):
    """The options of a whole render of scene sc (renderPanorama.default_opts fills in the rest)."""
    o = {"anglePower": power, "blending": blending, "pyrLevels": LEVELS, "pyrSigma": SIGMA, "tile": sc.tile, "cropBorder": False,
         "margin": MARGIN, "composeNonePolicy": "maxangle", "autoRef": sc.auto_ref}
    if sc.f_pan is not None:
        o["fPan"] = sc.f_pan
    o.update(more)
    return o


@functools.lru_cache(maxsize=None)
def geometry(name, mode):
    """The canvas of scene `name` in `mode` from oracle.canvas_geometry with the defaults of renderPanorama.m:41-71 and
    margin = MARGIN: the dict renderPanorama.canvas_geometry returns (mode, H, W, fPan, o0, o1, Rref, refIdx)."""
    import oracle

    sc = scene(name)
    f = float(sc.f_pan if sc.f_pan is not None else sc.cameras[sc.ref_idx]["K"][0, 0])
    o = {"fPan": f, "resScale": 1.0, "margin": MARGIN, "maxMegapixel": 50, "robustPct": (1, 99), "uvAbsCap": 8.0, "pixelPad": 24,
         "autoRef": sc.auto_ref}
    g = oracle.canvas_geometry(list(sc.cameras), list(sc.sizes), mode, sc.ref_idx, o)
    return {"mode": mode, "H": g["H"], "W": g["W"], "fPan": f, "o0": g["o0"], "o1": g["o1"],
            "Rref": np.asarray(sc.cameras[g["refIdx"]]["R"], np.float64), "refIdx": g["refIdx"]}


WARP_VIEWS = (7, FAN_GRAY)  # the views of the warp_tile cases: rolled by 3.5 rad (75 x 131, colour) and the gray one
WARP_ORIGIN = (5, 7)        # (r0, c0) of the warped window; it runs to the canvas's far corner


def warp_geometry(mode):
    """The canvas of the warp_tile cases: fan12's; the stereographic one (half angles: every view is half as large) at 1.5
    times the resolution, so that each warped view keeps a few thousand pixels."""
    g = dict(geometry("fan12", mode))
    if mode == "stereographic":
        g.update(fPan=1.5 * g["fPan"], H=int(1.5 * g["H"]), W=int(1.5 * g["W"]))
    return g


@functools.lru_cache(maxsize=None)
def masks(name, mode):
    """oracle.warp_tile's mask of every view over the whole canvas, [n, H, W] bool, read-only."""
    import oracle

    sc, geo = scene(name), geometry(name, mode)
    out = np.stack([oracle.warp_tile(im, c, geo, 0, 0, geo["H"], geo["W"], 1.0)[1] for im, c in zip(sc.images, sc.cameras)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_render(name, mode, blending, power):
    """oracle.render of the scene with render_opts(...): (panorama, coverage), computed once, shared, read-only."""
    import oracle

    sc, geo = scene(name), geometry(name, mode)
    out = oracle.render(list(sc.images), list(sc.cameras), geo, sc.tile, power, blending, LEVELS, SIGMA, "maxangle", False,
                        list(sc.gains))
    for a in out:
        a.setflags(write=False)
    return out


def block_counts(m, tile):
    """Per aligned BLOCK_H x BLOCK_W block of every tile (blocks start at the tile's origin): how many views' masks meet it.
    m: [n, H, W] bool.  Returns a flat int array, one entry per block."""
    n, H, W = m.shape
    out = []
    for r0 in range(0, H, tile[0]):
        for c0 in range(0, W, tile[1]):
            t = m[:, r0:r0 + tile[0], c0:c0 + tile[1]]
            for y in range(0, t.shape[1], BLOCK_H):
                for x in range(0, t.shape[2], BLOCK_W):
                    out.append(int(t[:, y:y + BLOCK_H, x:x + BLOCK_W].any(axis=(1, 2)).sum()))
    return np.asarray(out)


def tile_counts(m, tile):
    """Per tile: how many views have a non-empty mask inside it."""
    n, H, W = m.shape
    return np.asarray([int(m[:, r0:r0 + tile[0], c0:c0 + tile[1]].any(axis=(1, 2)).sum())
                       for r0 in range(0, H, tile[0]) for c0 in range(0, W, tile[1])])


# ---- what the scenes were chosen for, from a CPU run of the oracle (test_render_space_cases.py asserts them exactly) ------------
# per scene and mode: canvas (H, W), covered pixels, pixels under at least nine views, and the largest number of views whose
# masks meet one block / lie in one tile
Stats = namedtuple("Stats", "canvas covered deep max_block max_tile")
STATS = {
    ("fan12", "spherical"): Stats((208, 281), 35958, 1978, 12, 12),
    ("fan12", "cylindrical"): Stats((233, 281), 38842, 1992, 12, 12),
    ("fan12", "planar"): Stats((308, 412), 50822, 2027, 12, 12),
    ("fan12", "stereographic"): Stats((207, 207), 9729, 498, 12, 12),
    ("seam", "spherical"): Stats((135, 761), 16403, 0, 6, 6),
    ("crowd", "spherical"): Stats((153, 191), 18508, 11090, 62, 140),
    ("crowd", "planar"): Stats((250, 207), 20699, 11912, 63, 140),
    ("crowd40", "spherical"): Stats((147, 190), 16189, 809, 18, 40),
    ("crowd40", "planar"): Stats((200, 246), 18031, 822, 18, 40),
    ("slivers", "spherical"): Stats((190, 168), 18439, 0, 7, 8),
    ("slivers", "planar"): Stats((262, 227), 21895, 0, 7, 8),
}
# slivers: mask pixels of the four tiny views, spherical and planar
TINY_PIXELS = {"spherical": (948, 1557, 711, 858), "planar": (972, 1630, 722, 904)}

# ---- the case table of the whole renders -------------------------------------------------------------------------------------------
RenderCase = namedtuple("RenderCase", "scene mode blending power")

# fan12: every mode with multiband; every blending and every power appear; 'none' runs as 'maxangle', the one policy that reads
# the angle weight
FAN_CASES = (
    RenderCase("fan12", "spherical", "multiband", 1.0),
    RenderCase("fan12", "spherical", "multiband", 3.0),
    RenderCase("fan12", "spherical", "linear", 0.5),
    RenderCase("fan12", "cylindrical", "multiband", 0.5),
    RenderCase("fan12", "cylindrical", "none", 3.0),
    RenderCase("fan12", "planar", "multiband", 3.0),
    RenderCase("fan12", "planar", "linear", 1.0),
    RenderCase("fan12", "planar", "none", 0.5),
    RenderCase("fan12", "stereographic", "multiband", 1.0),
    RenderCase("fan12", "stereographic", "linear", 3.0),
    RenderCase("fan12", "stereographic", "none", 1.0),
)
# the other scenes at the real default power
OTHER_CASES = (
    RenderCase("seam", "spherical", "multiband", 1.0),
    RenderCase("seam", "spherical", "linear", 1.0),
    RenderCase("crowd", "spherical", "multiband", 1.0),
    RenderCase("crowd", "spherical", "linear", 1.0),
    RenderCase("crowd", "planar", "multiband", 1.0),
    RenderCase("crowd", "planar", "linear", 1.0),
    RenderCase("crowd40", "spherical", "multiband", 1.0),
    RenderCase("crowd40", "planar", "multiband", 1.0),
    RenderCase("slivers", "spherical", "multiband", 1.0),
    RenderCase("slivers", "spherical", "linear", 1.0),
    RenderCase("slivers", "planar", "multiband", 1.0),
)
SCENE_MODES = tuple(sorted({(c.scene, c.mode) for c in FAN_CASES + OTHER_CASES} | {("fan12", m) for m in MODES}))


def case_id(c):
    return f"{c.scene}-{c.mode}-{c.blending}-p{c.power:g}"
