"""The case tables of test_image_ops_cases.py (CPU) and test_image_ops_gpu.py (helper, not a test): imresize on uint8, imageWarp
and resizeImagesToLimits at the shapes, scales, transforms and layouts where csrc/render.hip's two kernels and their host
wrappers can go wrong.  numpy only; the oracle is imported where a function needs it.

imresize (imresize_u8_dim_kernel: 128 lanes along the untouched dimension, one output sample per blockIdx.y, at most 64 taps)
  edge*      3 x {127, 128, 129} and the transposes: the last lane of a block, a full block, one lane into the next
  s*         scales on 40 x 60 x 3: 0.5 (weights k/8 and k/32: exact .5 ties), 0.37, 1/3, 1.0 (the input's bytes), 1.5, 2; 8 on
             5 x 7; 1/15 and 0.0646 on 62 x 40: 62 and 64 taps, the last scale the library builds
  size*      [oh ow] forms: rows shrink while columns grow (rows first), the reverse (columns first), and 40 x 60 -> 20 x 30,
             where equal scales go rows first (the uint8 intermediate makes the order visible)
  tiny*      1 x 1 -> 3 x 3, 1 x 9 -> 4 x 3, 7 x 1 -> 1 x 1, 9 x 13 x 3 -> 1 x 1 (the smallest scale of a [1 1] target the
             64 taps allow is 1/15)
  ch*        a 2-D array, H x W x 1 and 2, 3, 4 channels
  zeros*, full*, checker*   all 0, all 255 and a 0/255 checkerboard of 2 x 2 cells: bicubic overshoot reaches both clamps

imageWarp (image_warp_h_kernel: 256 lanes per canvas row block, one row per blockIdx.y; three methods; uint8 and single)
  src*       the smallest sources at which a method has any valid pixel: 1 x 1 and 1 x 6 (nearest), 2 x 2 and 3 x 3 (bilinear
             from 2 x 2), 4 x 4 and 5 x 4 (bicubic from 4 x 4)
  w1, w255, w256, w257, extents, one   views of 1, 255, 256 and 257 columns with at most 4 rows, pixel extents (0.75, 1.5) with
             world origins that are no half-integers, and a view of one pixel
  identity, shift, rot90, mirror, zoom8, shrink8   on a 40 x 50 source: integer canvas centres (the valid region is the source's
             bytes), a (0.5, 0.5) shift (every bilinear weight 1/4: rounding ties), a quarter turn, a negative determinant,
             8 and 1/8
  persp-w0   the back-projected third coordinate is exactly 0 on the canvas column X = 8 and changes sign across it
  tiny-w     H(3,3) = 0 and entries of 1e12: every back-projected coordinate is of the order 1e-12, so on the columns 0 < X < 8
             the rule w = sign(w) max(|w|, 1e-12) replaces w
  ch1..ch4   channel counts 1 to 4, both types; fill values 0, 9, 255 (uint8) and 0.25 (single)
  nan-src    NaN in a single-precision source: nearest copies it, bilinear spreads it, bicubic's max(0, min(1, .)) gives 1
  singular, h33-zero, nan, big, small   every pixel is the fill value: det = 0; H(3,3) = 0 with a projective row and a view on
             the far side; a NaN entry; entries of 1e8 (source coordinates near -1); entries of 1e-8 (source coordinates
             above 2^31: validity has to be decided in double before any cast to int)
  border-*   identity H, one canvas row: centres on srcx = in_w exactly (invalid for bilinear: x2 = in_w + 1), on 0.5 and
             in_w + 0.5 (nearest rounds half away from zero) and on the double below 0.5 (round gives 0, floor(x + 0.5) gives 1);
             the number of valid columns of each method is written down in the table
Single-precision sources hold values in [-0.5, 1.5]: bicubic clamps its result to [0, 1], bilinear and nearest do not.

resizeImagesToLimits: sets (a) nothing too large, equal sizes; (b) nothing too large, unequal sizes; (c) mixed; (d) over the
limit in one dimension only; (e) a 2-D and an H x W x 1 image; (f) odd pad and crop differences."""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np

RESIZE_LANES, WARP_LANES, MAX_TAPS = 128, 256, 64
METHODS = ("nearest", "bilinear", "bicubic")


def _seed(name):
    return zlib.crc32(name.encode())


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- imresize -------------------------------------------------------------------------------------------------------------------
ResizeCase = namedtuple("ResizeCase", "name shape arg method content")


def _resize_cases():
    out = []
    for h, w in ((3, 127), (3, 128), (3, 129), (127, 3), (128, 3), (129, 3)):
        out.append(ResizeCase(f"edge{h}x{w}-s0.5-bilinear", (h, w, 3), 0.5, "bilinear", "random"))
        out.append(ResizeCase(f"edge{h}x{w}-s1.5-bicubic", (h, w, 3), 1.5, "bicubic", "random"))
    base = (40, 60, 3)
    for s, tag in ((0.5, "0.5"), (0.37, "0.37"), (1 / 3, "third"), (1.0, "1"), (1.5, "1.5"), (2.0, "2")):
        for method in ("bicubic", "bilinear"):
            out.append(ResizeCase(f"s{tag}-{method}", base, s, method, "random"))
    out.append(ResizeCase("s8-bicubic", (5, 7, 3), 8.0, "bicubic", "random"))
    out.append(ResizeCase("s8-bilinear", (5, 7, 3), 8.0, "bilinear", "random"))
    out.append(ResizeCase("s15th-bicubic", (62, 40, 3), 1 / 15, "bicubic", "random"))     # 62 taps
    out.append(ResizeCase("s15th-bilinear", (62, 40, 3), 1 / 15, "bilinear", "random"))   # 32 taps
    out.append(ResizeCase("s0.0646-bicubic", (62, 40, 3), 0.0646, "bicubic", "random"))   # 64 taps
    out.append(ResizeCase("size-rows-shrink-cols-grow", base, (20, 90), "bicubic", "random"))   # scale_r < scale_c: rows first
    out.append(ResizeCase("size-rows-grow-cols-shrink", base, (60, 30), "bicubic", "random"))   # scale_r > scale_c: columns first
    out.append(ResizeCase("size-equal-scales-bicubic", base, (20, 30), "bicubic", "random"))    # a tie: rows first
    out.append(ResizeCase("size-equal-scales-bilinear", base, (20, 30), "bilinear", "random"))
    out.append(ResizeCase("tiny-1x1-to-3x3", (1, 1), (3, 3), "bicubic", "random"))
    out.append(ResizeCase("tiny-1x9-to-4x3", (1, 9), (4, 3), "bicubic", "random"))
    out.append(ResizeCase("tiny-7x1-to-1x1", (7, 1), (1, 1), "bilinear", "random"))
    out.append(ResizeCase("tiny-9x13x3-to-1x1", (9, 13, 3), (1, 1), "bicubic", "random"))
    for shape, tag in (((17, 23), "2d"), ((17, 23, 1), "c1"), ((17, 23, 2), "c2"), ((17, 23, 3), "c3"), ((17, 23, 4), "c4")):
        out.append(ResizeCase(f"ch-{tag}", shape, 0.37, "bicubic", "random"))
    out.append(ResizeCase("ch-c4-tall", (129, 5, 4), 1.5, "bilinear", "random"))
    for content in ("zeros", "full"):
        out.append(ResizeCase(f"{content}-s0.5", (13, 11, 3), 0.5, "bicubic", content))
        out.append(ResizeCase(f"{content}-s2", (13, 11, 3), 2.0, "bicubic", content))
    out.append(ResizeCase("checker-s2-bicubic", (24, 28, 3), 2.0, "bicubic", "checker"))
    out.append(ResizeCase("checker-s1.5-bicubic", (24, 28, 3), 1.5, "bicubic", "checker"))
    out.append(ResizeCase("checker-s0.5-bicubic", (24, 28, 3), 0.5, "bicubic", "checker"))
    out.append(ResizeCase("checker-s2-bilinear", (24, 28, 3), 2.0, "bilinear", "checker"))
    return tuple(out)


RESIZE_CASES = _resize_cases()
TIE_RESIZE_CASES = ("s0.5-bicubic", "s0.5-bilinear")
CLAMP_RESIZE_CASES = ("checker-s2-bicubic", "checker-s1.5-bicubic")


@functools.lru_cache(maxsize=None)
def resize_image(name):
    """The seeded uint8 source of imresize case `name`, read-only."""
    c = RESIZE_BY_NAME[name]
    if c.content == "zeros":
        img = np.zeros(c.shape, np.uint8)
    elif c.content == "full":
        img = np.full(c.shape, 255, np.uint8)
    elif c.content == "checker":
        yy, xx = np.mgrid[0:c.shape[0], 0:c.shape[1]]
        cells = (((yy // 2 + xx // 2) % 2) * 255).astype(np.uint8)
        img = np.ascontiguousarray(np.broadcast_to(cells[..., None], c.shape)) if len(c.shape) == 3 else cells
    else:
        img = np.random.default_rng(_seed(name)).integers(0, 256, c.shape, dtype=np.uint8)
    return _frozen(img)


RESIZE_BY_NAME = {c.name: c for c in RESIZE_CASES}


def resize_target(c):
    """(oh, ow, scale_r, scale_c) as imresize's scalar form (ceil(s * size)) and size form ([oh ow] / size) define them."""
    h, w = c.shape[:2]
    if np.isscalar(c.arg):
        s = float(c.arg)
        return int(math.ceil(h * s)), int(math.ceil(w * s)), s, s
    return int(c.arg[0]), int(c.arg[1]), c.arg[0] / h, c.arg[1] / w


@functools.lru_cache(maxsize=None)
def oracle_resize(name):
    """oracle.imresize_u8 of the case, computed once, shared, read-only."""
    import oracle

    c = RESIZE_BY_NAME[name]
    return _frozen(oracle.imresize_u8(resize_image(name), c.arg, c.method))


# ---- imageWarp ------------------------------------------------------------------------------------------------------------------
View = namedtuple("View", "oh ow x0 y0 sx sy")  # (x0, y0): the world coordinates of the first pixel's centre (imageWarp.m:43-50)
# kind: 'normal' (between 5 % and 95 % of the view valid), 'one' (a view of one pixel, which is valid), 'degenerate' (every pixel
# is the fill value), 'border' (valid_cols: method -> the number of valid columns of the single row)
WarpCase = namedtuple("WarpCase", "name kind shape dtype H view methods fill valid_cols")

EYE = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
H_GEN = ((0.97, 0.05, 6.5), (-0.04, 1.02, -3.25), (2e-4, -1e-4, 1.0))
BELOW_HALF = float(np.nextafter(0.5, 0.0))


def _warp_cases():
    out = []

    def add(name, kind, shape, dtype, H, view, methods=METHODS, fill=None, valid_cols=None):
        fill = (9 if dtype == "u8" else 0.25) if fill is None else fill
        out.append(WarpCase(name, kind, shape, dtype, tuple(tuple(float(v) for v in r) for r in H), View(*view), tuple(methods),
                            fill, valid_cols))

    def both(name, kind, H, view, methods=METHODS, shape=(40, 50)):
        add(name + "-u8", kind, shape + (3,), "u8", H, view, methods)
        add(name + "-f32", kind, shape + (1,), "f32", H, view, methods)

    # the smallest sources
    add("src1x1", "normal", (1, 1, 3), "u8", EYE, (3, 3, 0.0, 0.0, 1.0, 1.0), ("nearest",))
    add("src1x6", "normal", (1, 6, 1), "f32", EYE, (3, 10, 0.3, 0.6, 0.75, 0.5), ("nearest",))
    add("src2x2", "normal", (2, 2, 3), "u8", EYE, (4, 8, 0.4, 0.75, 0.3, 0.5), ("nearest", "bilinear"), 0)
    add("src3x3", "normal", (3, 3, 2), "f32", EYE, (6, 8, 0.4, 0.6, 0.4, 0.5), ("nearest", "bilinear"))
    add("src4x4", "normal", (4, 4, 3), "u8", EYE, (19, 19, 0.25, 0.25, 0.25, 0.25), ("nearest", "bilinear"), 0)
    add("src4x4-cubic", "normal", (4, 4, 3), "u8", EYE, (10, 10, 1.5, 1.5, 0.25, 0.25), ("bicubic",), 255)
    add("src5x4-cubic", "normal", (5, 4, 1), "f32", EYE, (12, 10, 1.5, 1.5, 0.25, 0.25), ("bicubic",))
    # views around the 256 lanes of a block, at most four rows; one column; one pixel; anisotropic extents
    for ow in (255, 256, 257):
        add(f"w{ow}", "normal", (40, 50, 3), "u8", H_GEN, (3 if ow != 256 else 4, ow, -2.3, 5.2, 0.25, 1.5))
    add("w257-f32", "normal", (40, 50, 2), "f32", H_GEN, (2, 257, -2.3, 5.2, 0.25, 1.5))
    both("w1", "normal", H_GEN, (4, 1, 20.3, -4.7, 1.0, 3.0))
    both("one", "one", H_GEN, (1, 1, 20.3, 17.6, 1.0, 1.0))
    both("extents", "normal", H_GEN, (32, 80, -3.3, -2.7, 0.75, 1.5))
    # the transform grid on 40 x 50
    both("identity", "normal", EYE, (44, 56, -1.0, -1.0, 1.0, 1.0))
    both("shift", "normal", ((1, 0, 0.5), (0, 1, 0.5), (0, 0, 1)), (44, 56, -1.0, -1.0, 1.0, 1.0))
    both("rot90", "normal", ((0, -1, 41.3), (1, 0, 0.2), (0, 0, 1)), (56, 44, -1.0, -1.0, 1.0, 1.0))
    both("mirror", "normal", ((-1, 0, 51.25), (0, 1, 0), (0, 0, 1)), (44, 56, -1.0, -1.0, 1.0, 1.0))
    both("zoom8", "normal", ((8, 0, 0), (0, 8, 0), (0, 0, 1)), (40, 56, -10.5, -10.5, 1.0, 1.0))
    both("shrink8", "normal", ((0.125, 0, 0), (0, 0.125, 0), (0, 0, 1)), (8, 10, -1.5, -1.5, 1.0, 1.0))
    both("persp-w0", "normal", ((1, 0, 0), (0, 1, 0), (0.125, 0, 1)), (12, 16, 1.0, 1.0, 1.0, 1.0))
    both("tiny-w", "normal", ((1e12, 0, 4e12), (0, 1e12, 0), (0.25e12, 0, 0)), (12, 20, 0.5, 1.0, 1.0, 1.0))
    # channels and fill values
    for c, fill in ((1, 0), (2, 9), (3, 255), (4, 9)):
        add(f"ch{c}-u8", "normal", (12, 14, c), "u8", H_GEN, (14, 18, 5.2, -4.1, 1.0, 1.0), METHODS, fill)
        add(f"ch{c}-f32", "normal", (12, 14, c), "f32", H_GEN, (14, 18, 5.2, -4.1, 1.0, 1.0), METHODS, 0.25)
    # NaN in a single-precision source: nearest copies it, bilinear spreads it over its 2 x 2 taps, bicubic's
    # max(0, min(1, .)) turns it into 1 (MATLAB's min and max skip a NaN)
    add("nan-src-f32", "normal", (12, 14, 2), "f32", H_GEN, (14, 18, 5.2, -4.1, 1.0, 1.0))
    # degenerate transforms
    nan_h = [list(r) for r in H_GEN]
    nan_h[0][1] = float("nan")
    for name, H, view in (("singular", ((1, 2, 3), (2, 4, 6), (0, 0, 1)), (6, 9, 0.5, 0.5, 1.0, 1.0)),
                          ("h33-zero", ((1, 0, 4), (0, 1, 0), (0.25, 0, 0)), (6, 4, 0.5, 0.5, 1.0, 1.0)),
                          ("nan", nan_h, (6, 9, 0.5, 0.5, 1.0, 1.0)),
                          ("big", ((1e8, 0, 1e8), (0, 1e8, 1e8), (0, 0, 1)), (6, 9, 0.5, 0.5, 1.0, 1.0)),
                          ("small", ((1e-8, 0, 0), (0, 1e-8, 0), (0, 0, 1)), (6, 9, 30.5, 30.5, 1.0, 1.0))):
        both(name, "degenerate", H, view, METHODS, (12, 14))
    # borders by known answer: identity H, one canvas row at Y = 2 of a 5 x 6 source
    for dtype in ("u8", "f32"):
        add(f"border-int-{dtype}", "border", (5, 6, 2), dtype, EYE, (1, 8, 0.0, 2.0, 1.0, 1.0), METHODS, None,
            {"nearest": 6, "bilinear": 5, "bicubic": 3})      # X = 0 .. 7: X = 6 = in_w is invalid for bilinear
        add(f"border-half-{dtype}", "border", (5, 6, 2), dtype, EYE, (1, 8, -0.5, 2.0, 1.0, 1.0), METHODS, None,
            {"nearest": 6, "bilinear": 5, "bicubic": 3})      # X = -0.5 .. 6.5: 0.5 rounds to 1, 6.5 to 7
        add(f"border-below-half-{dtype}", "border", (5, 6, 2), dtype, EYE, (1, 7, BELOW_HALF, 2.0, 1.0, 1.0), METHODS, None,
            {"nearest": 5, "bilinear": 5, "bicubic": 3})      # X = 0.49999999999999994, 1.5 .. 6.5: the first rounds to 0
    return tuple(out)


WARP_CASES = _warp_cases()
WARP_BY_NAME = {c.name: c for c in WARP_CASES}
TIE_WARP_CASES = ("shift-u8",)
NAN_SOURCE_CASES = ("nan-src-f32",)
NAN_PIXELS = ((3, 4, 0), (3, 5, 0), (7, 9, 1), (10, 2, 0), (10, 2, 1))  # (row, column, channel), 0-based, inside every method's reach
OTHER_FILL = {"u8": 200, "f32": -7.0}  # a second fill value: the pixels that do not follow it are the valid ones


@functools.lru_cache(maxsize=None)
def warp_source(name):
    """The seeded source of warp case `name`: random bytes, or single-precision values in [-0.5, 1.5]; read-only."""
    c = WARP_BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    if c.dtype == "u8":
        return _frozen(rng.integers(0, 256, c.shape, dtype=np.uint8))
    img = (rng.random(c.shape, dtype=np.float32) * np.float32(2.0) - np.float32(0.5)).astype(np.float32)
    if name in NAN_SOURCE_CASES:
        for y, x, ch in NAN_PIXELS:
            img[y, x, ch] = np.nan
    return _frozen(img)


def same_image(a, b):
    """Equal shape and type; uint8 by bytes; single by bits, except that a NaN equals a NaN: NaN payloads are no part of the
    contract."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.uint8:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def output_view(c):
    """The imref2d-like struct imageWarp takes (imageProcessing.imref2dScratch's fields) with the case's exact pixel extents."""
    v = c.view
    return {"ImageSize": (v.oh, v.ow), "XWorldLimits": (v.x0, v.x0 + v.ow * v.sx), "YWorldLimits": (v.y0, v.y0 + v.oh * v.sy),
            "PixelExtentInWorldX": v.sx, "PixelExtentInWorldY": v.sy}


@functools.lru_cache(maxsize=None)
def oracle_warp(name, method, fill=None):
    """oracle.image_warp_h of the case with one of its methods (fill: the case's unless given); computed once, read-only."""
    import oracle

    c = WARP_BY_NAME[name]
    v = c.view
    out = oracle.image_warp_h(warp_source(name), np.array(c.H), v.oh, v.ow, v.x0, v.y0, v.sx, v.sy, c.fill if fill is None else fill,
                              method=method)
    return _frozen(out)


def oracle_valid(name, method):
    """[oh, ow] bool: the pixels the oracle takes from the source - those that do not follow the fill value."""
    c = WARP_BY_NAME[name]
    a, b = oracle_warp(name, method), oracle_warp(name, method, OTHER_FILL[c.dtype])
    same = a.view(np.uint32 if a.dtype == np.float32 else np.uint8) == b.view(np.uint32 if b.dtype == np.float32 else np.uint8)
    return same.all(axis=2)


def warp_runs():
    """(case, method) for every method of every case."""
    return [(c, m) for c in WARP_CASES for m in c.methods]


# ---- resizeImagesToLimits ---------------------------------------------------------------------------------------------------------
LimitSet = namedtuple("LimitSet", "name shapes limits")  # limits: (heightLimit, widthLimit)
LIMIT_MODES = ("fit", "pad", "fillcrop")
LIMIT_SETS = (
    LimitSet("a-equal-within", ((30, 40, 3), (30, 40, 3), (30, 40, 3)), (48, 64)),
    LimitSet("b-unequal-within", ((30, 40, 3), (24, 50, 3), (48, 64, 3)), (48, 64)),
    LimitSet("c-mixed", ((60, 100, 3), (45, 45, 3), (20, 25, 3)), (40, 50)),
    LimitSet("d-one-dimension-over", ((30, 80, 3), (30, 40, 3)), (40, 50)),
    LimitSet("e-2d-and-one-channel", ((50, 70), (33, 41, 1)), (40, 50)),
    LimitSet("f-odd-differences", ((30, 41, 3), (37, 44, 3), (90, 61, 3)), (41, 52)),
)
LIMITS_BY_NAME = {s.name: s for s in LIMIT_SETS}


@functools.lru_cache(maxsize=None)
def limit_images(name):
    s = LIMITS_BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    return tuple(_frozen(rng.integers(0, 256, shp, dtype=np.uint8)) for shp in s.shapes)


def center_crop(J, Ht, Wt):
    """centerCrop (resizeImagesToLimits.m:152-176): y0 = floor((h - Ht) / 2) + 1, 1-based."""
    h, w = J.shape[:2]
    Ht, Wt = min(Ht, h), min(Wt, w)
    r0, c0 = (h - Ht) // 2, (w - Wt) // 2
    return J[r0:r0 + Ht, c0:c0 + Wt]


def pad_to_box(J, Ht, Wt):
    """padToBox (:111-150): crop what is larger, then replicate floor(d / 2) before and the rest after."""
    h, w = J.shape[:2]
    if h > Ht or w > Wt:
        J = center_crop(J, min(Ht, h), min(Wt, w))
        h, w = J.shape[:2]
    top, left = (Ht - h) // 2, (Wt - w) // 2
    pad = ((top, Ht - h - top), (left, Wt - w - left)) + (((0, 0),) if J.ndim == 3 else ())
    return np.pad(J, pad, mode="edge")


def limits_statement(images, height_limit, width_limit, mode):
    """resizeImagesToLimits.m:17-106 on the host, every imresize by oracle.imresize_u8: the expectation of the device path.
    Returns a list; with the early exit of :29-42 its elements are the very objects of `images`."""
    import oracle

    if mode not in LIMIT_MODES:
        raise ValueError(mode)
    if not isinstance(images, (list, tuple)) or len(images) == 0:
        raise ValueError("imageFiles must be a nonempty cell array of images.")
    if not (np.isscalar(height_limit) and np.isscalar(width_limit) and height_limit > 0 and width_limit > 0):
        raise ValueError("heightLimit and widthLimit must be positive scalars.")
    sizes = [tuple(I.shape[:2]) for I in images]
    if not any(h > height_limit or w > width_limit for h, w in sizes) and len(set(sizes)) == 1:
        return list(images)
    stage1 = []
    for I in images:
        h, w = I.shape[:2]
        if mode in ("fit", "pad"):
            s = min(height_limit / h, width_limit / w)
            J = oracle.imresize_u8(I, s, "bicubic") if s < 1 else I
            if mode == "pad":
                J = pad_to_box(J, height_limit, width_limit)
        else:
            s = max(height_limit / h, width_limit / w)
            J = center_crop(oracle.imresize_u8(I, s, "bicubic"), height_limit, width_limit)
        stage1.append(J)
    if mode != "fit":
        return stage1
    sizes1 = {J.shape[:2] for J in stage1}
    if len(sizes1) == 1:
        return stage1
    Hmax, Wmax = max(s[0] for s in sizes1), max(s[1] for s in sizes1)
    return [oracle.imresize_u8(J, (Hmax, Wmax), "bicubic") for J in stage1]
