"""Keeps the image-operator case tables honest (CPU, oracle only; image_ops_cases.py, run on the device by
test_image_ops_gpu.py).

  * A plain float64 numpy restatement of imresize on uint8 (the contract in the header of oracle/render_oracle.c's imresize
    section: imresize is toolbox code) and of imageWarp.m:39-264 - taps summed one by one in tap order, the parenthesisation of
    the .m lines - equals the oracle byte for byte (uint8) and bit for bit (single) on every case.  It is written from the
    text, not from the oracle's or the kernel's source, so it pins the oracle at these edges.
  * The conditions the cases were chosen for: valid fractions, rounding ties, both clamps, the valid columns at the borders.
  * Discriminating power: the restatement takes switches for deliberate deviations (DEVIATIONS); each must change the output of
    at least one case.  A case table that cannot tell them apart is not done.
  * limits_statement (the host statement of resizeImagesToLimits.m:17-106, the expectation of the device test): the early exit,
    the floor rules of padToBox and centerCrop, the argument checks.
  * transformPointsForwardScratch and outputLimitsScratch against the direct formula."""
import math
from importlib import import_module

import numpy as np
import pytest

import image_ops_cases as ic
import oracle

DEVIATIONS_RESIZE = ("swap_order", "half_even", "clamp_short", "no_normalise")
DEVIATIONS_WARP = ("half_even", "bilinear_le", "bicubic_off", "nearest_floor", "no_w_clamp")
DEVIATIONS = tuple(dict.fromkeys(DEVIATIONS_RESIZE + DEVIATIONS_WARP))


same = ic.same_image  # bytes, or bits with NaN equal to NaN


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def round_half_away(v):
    """MATLAB's round: v - trunc(v) is exact, so no v + 0.5 that could round up by itself."""
    t = np.trunc(v)
    return t + np.copysign((np.abs(v - t) >= 0.5).astype(np.float64), v)


def to_u8(v, dev, stats, key="ties"):
    if stats is not None:
        stats[key] = stats.get(key, 0) + int((np.abs(v - np.trunc(v)) == 0.5).sum())
        stats["over"] = stats.get("over", 0) + int((v >= 255.5).sum())
        stats["under"] = stats.get("under", 0) + int((v <= -0.5).sum())
    r = np.rint(v) if "half_even" in dev else round_half_away(v)
    return np.minimum(np.where(r > 0, r, 0.0), 255.0).astype(np.uint8)


def keys(x):
    """Keys' cubic, a = -0.5 (bicubicKernel, imageWarp.m:275-301): |x|^2 and |x|^3 as products, terms left to right."""
    a = np.abs(x)
    a2 = a * a
    a3 = a2 * a
    return np.where(a <= 1.0, (1.5 * a3 - 2.5 * a2) + 1.0, np.where(a <= 2.0, ((-0.5 * a3 + 2.5 * a2) - 4.0 * a) + 2.0, 0.0))


def resize_dim(a, dim, out_len, scale, bicubic, dev, stats):
    """One pass of imresize along `dim` of a uint8 [h, w, C] array: antialiasing on shrink (the kernel stretched by 1 / scale),
    centres u = x / scale + 0.5 (1 - 1 / scale), ceil(width) + 2 taps from floor(u - width / 2), weights normalised to sum 1,
    indices clamped to the image, the sum in double in tap order, rounded half away from zero and saturated."""
    src = a if dim == 0 else a.swapaxes(0, 1)
    in_len = src.shape[0]
    out = np.empty((out_len,) + src.shape[1:], np.uint8)
    kw0 = 4.0 if bicubic else 2.0
    kw = kw0 / scale if scale < 1.0 else kw0
    hi = max(in_len - 1, 1) if "clamp_short" in dev else in_len
    for o in range(out_len):
        u = float(o + 1) / scale + 0.5 * (1.0 - 1.0 / scale)
        left = int(math.floor(u - kw / 2.0))
        P = min(int(math.ceil(kw)) + 2, ic.MAX_TAPS)
        wts = []
        for t in range(P):
            dx = u - float(left + t)
            arg = scale * dx if scale < 1.0 else dx
            v = float(keys(np.float64(arg))) if bicubic else (1.0 - abs(arg) if abs(arg) < 1.0 else 0.0)
            wts.append(scale * v if scale < 1.0 else v)
        s = 0.0
        for v in wts:
            s += v
        if "no_normalise" not in dev:
            wts = [v / s for v in wts]
        acc = np.zeros(src.shape[1:], np.float64)
        for t in range(P):
            idx = min(max(left + t, 1), hi) - 1
            acc = acc + wts[t] * src[idx].astype(np.float64)
        out[o] = to_u8(acc, dev, stats)
    return out if dim == 0 else out.swapaxes(0, 1)


def restate_imresize(img, arg, method, dev=frozenset(), stats=None):
    """imresize(I, s | [oh ow], method) on uint8: the dimension with the smaller scale first (ties: rows), a uint8
    intermediate."""
    a = np.asarray(img)
    sq = a.ndim == 2
    if sq:
        a = a[..., None]
    h, w = a.shape[:2]
    if np.isscalar(arg):
        s = float(arg)
        oh, ow, sr, sc = int(math.ceil(h * s)), int(math.ceil(w * s)), s, s
    else:
        oh, ow = int(arg[0]), int(arg[1])
        sr, sc = oh / h, ow / w
    bic = method == "bicubic"
    rows_first = (sr <= sc) != ("swap_order" in dev)
    if rows_first:
        out = resize_dim(resize_dim(a, 0, oh, sr, bic, dev, stats), 1, ow, sc, bic, dev, stats)
    else:
        out = resize_dim(resize_dim(a, 1, ow, sc, bic, dev, stats), 0, oh, sr, bic, dev, stats)
    out = np.ascontiguousarray(out)
    return out[..., 0] if sq else out


def restate_warp(img, H, view, method, fill, dev=frozenset(), stats=None):
    """imageWarp.m:39-264.  src = H \\ [X; Y; 1] is stated as adj(H) [X; Y; 1] / det(H), cofactors and determinant as sums of
    products left to right; everything else follows the .m lines."""
    a = np.asarray(img)
    a = a[..., None] if a.ndim == 2 else a
    is_u8 = a.dtype == np.uint8
    in_h, in_w, C = a.shape
    src = a.astype(np.float64)
    with np.errstate(all="ignore"):
        h = np.array(H, np.float64)
        if h[2, 2] != 0:  # :61-64
            h = h / h[2, 2]
        A = np.empty((3, 3))  # the adjugate: A[i, j] multiplies (X, Y, 1)[j] in source coordinate i
        A[0, 0] = h[1, 1] * h[2, 2] - h[1, 2] * h[2, 1]
        A[0, 1] = h[0, 2] * h[2, 1] - h[0, 1] * h[2, 2]
        A[0, 2] = h[0, 1] * h[1, 2] - h[0, 2] * h[1, 1]
        A[1, 0] = h[1, 2] * h[2, 0] - h[1, 0] * h[2, 2]
        A[1, 1] = h[0, 0] * h[2, 2] - h[0, 2] * h[2, 0]
        A[1, 2] = h[0, 2] * h[1, 0] - h[0, 0] * h[1, 2]
        A[2, 0] = h[1, 0] * h[2, 1] - h[1, 1] * h[2, 0]
        A[2, 1] = h[0, 1] * h[2, 0] - h[0, 0] * h[2, 1]
        A[2, 2] = h[0, 0] * h[1, 1] - h[0, 1] * h[1, 0]
        det = (h[0, 0] * A[0, 0] + h[0, 1] * A[1, 0]) + h[0, 2] * A[2, 0]
        X, Y = np.meshgrid(view.x0 + np.arange(view.ow, dtype=np.float64) * view.sx,
                           view.y0 + np.arange(view.oh, dtype=np.float64) * view.sy)  # :49-50
        s0 = ((A[0, 0] * X + A[0, 1] * Y) + A[0, 2]) / det
        s1 = ((A[1, 0] * X + A[1, 1] * Y) + A[1, 2]) / det
        s2 = ((A[2, 0] * X + A[2, 1] * Y) + A[2, 2]) / det
        w = s2 if "no_w_clamp" in dev else np.sign(s2) * np.maximum(np.abs(s2), 1e-12)  # :99
        srcx, srcy = s0 / w, s1 / w
        out = np.empty((view.oh, view.ow, C), a.dtype)
        out[...] = np.asarray(fill).astype(a.dtype)

        def px(yy, xx):  # 1-based (row, column) of the valid pixels -> [n, C] double; deviations may step outside: replicate
            return src[np.clip(yy.astype(np.int64), 1, in_h) - 1, np.clip(xx.astype(np.int64), 1, in_w) - 1]

        if method == "nearest":  # :109-123
            rnd = (lambda v: np.floor(v + 0.5)) if "nearest_floor" in dev else round_half_away
            x, y = rnd(srcx), rnd(srcy)
            valid = (x >= 1) & (x <= in_w) & (y >= 1) & (y <= in_h)
            out[valid] = a[y[valid].astype(np.int64) - 1, x[valid].astype(np.int64) - 1]
            return out
        if method == "bilinear":  # :125-168
            x1, y1 = np.floor(srcx), np.floor(srcy)
            x2, y2 = x1 + 1, y1 + 1
            wx, wy = srcx - x1, srcy - y1
            valid = (x1 >= 1) & ((x1 <= in_w) if "bilinear_le" in dev else (x2 <= in_w)) & (y1 >= 1) & (y2 <= in_h)
            wxv, wyv = wx[valid][:, None], wy[valid][:, None]
            w11, w12, w21, w22 = (1 - wxv) * (1 - wyv), (1 - wxv) * wyv, wxv * (1 - wyv), wxv * wyv
            v = ((w11 * px(y1[valid], x1[valid]) + w12 * px(y2[valid], x1[valid])) + w21 * px(y1[valid], x2[valid])) \
                + w22 * px(y2[valid], x2[valid])
            out[valid] = to_u8(v, dev, stats) if is_u8 else v.astype(np.float32)
            return out
        # bicubic, :170-264
        x, y = np.floor(srcx), np.floor(srcy)
        dx, dy = srcx - x, srcy - y
        top = 1 if "bicubic_off" in dev else 2
        valid = (x >= 2) & (x <= in_w - top) & (y >= 2) & (y <= in_h - top)
        xv, yv, dxv, dyv = x[valid], y[valid], dx[valid], dy[valid]
        xw = [keys(ii - dxv)[:, None] for ii in range(-1, 3)]  # :194-197
        yw = [keys(ii - dyv)[:, None] for ii in range(-1, 3)]
        v = np.zeros((len(xv), C))
        for jj in range(4):  # xInterp(:, jj) over ii in ascending order from 0 (:240-247), then the sum over jj (:250)
            xi = np.zeros((len(xv), C))
            for ii in range(4):
                xi = xi + px(yv + (jj - 1), xv + (ii - 1)) * xw[ii]
            v = v + xi * yw[jj]
        if is_u8:
            out[valid] = to_u8(v, dev, stats)  # max(0, min(maxVal, round(.))), :255
        else:
            out[valid] = np.fmax(0.0, np.fmin(1.0, v)).astype(np.float32)  # maxVal = 1, :258; MATLAB's min and max skip a NaN, as fmin and fmax do
        return out


def restated_resize(c, dev=frozenset(), stats=None):
    return restate_imresize(ic.resize_image(c.name), c.arg, c.method, dev, stats)


def restated_warp(c, method, dev=frozenset(), stats=None):
    return restate_warp(ic.warp_source(c.name), c.H, c.view, method, c.fill, dev, stats)


# ---- the restatement equals the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ic.RESIZE_CASES, ids=lambda c: c.name)
def test_imresize_restatement_equals_the_oracle(c):
    ref = ic.oracle_resize(c.name)
    oh, ow, sr, sc = ic.resize_target(c)
    assert ref.shape[:2] == (oh, ow) and ref.shape[2:] == tuple(c.shape[2:])
    assert 4.0 / min(1.0, sr, sc) + 2 <= ic.MAX_TAPS  # a scale the library builds
    assert same(restated_resize(c), ref)
    if c.arg == 1.0:
        assert same(ref, ic.resize_image(c.name))
    if c.content in ("zeros", "full"):
        assert np.all(ref == (0 if c.content == "zeros" else 255))


@pytest.mark.parametrize("c,method", ic.warp_runs(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_warp_restatement_equals_the_oracle_and_the_view_is_partly_valid(c, method):
    ref = ic.oracle_warp(c.name, method)
    assert ref.shape == (c.view.oh, c.view.ow, c.shape[2]) and ref.dtype == (np.uint8 if c.dtype == "u8" else np.float32)
    assert same(restated_warp(c, method), ref)
    valid = ic.oracle_valid(c.name, method)
    assert np.all(ref[~valid] == np.asarray(c.fill).astype(ref.dtype))
    if c.kind == "normal":
        assert 0.05 <= valid.mean() <= 0.95, valid.mean()
    elif c.kind == "one":
        assert valid.shape == (1, 1) and valid.all()  # a view of one pixel has no fraction in between: the pixel is valid
    elif c.kind == "degenerate":
        assert valid.sum() == 0
    else:
        assert c.view.oh == 1 and int(valid.sum()) == c.valid_cols[method]


def test_case_tables_hold_what_they_were_chosen_for():
    names = [c.name for c in ic.RESIZE_CASES] + [c.name for c in ic.WARP_CASES]
    assert len(set(names)) == len(names)
    shapes = {c.shape[:2] for c in ic.RESIZE_CASES}
    assert {(3, 127), (3, 128), (3, 129), (127, 3), (128, 3), (129, 3)} <= shapes
    assert any(len(c.shape) == 2 for c in ic.RESIZE_CASES) and {c.shape[2] for c in ic.RESIZE_CASES if len(c.shape) == 3} >= {1, 2, 3, 4}
    orders = {(sr <= sc, sr < 1, sc < 1) for sr, sc in (ic.resize_target(c)[2:] for c in ic.RESIZE_CASES)}
    assert (True, True, False) in orders and (False, False, True) in orders  # rows shrink / columns grow, and the reverse
    taps = {int(math.ceil(4.0 / min(1.0, ic.resize_target(c)[2]))) + 2 for c in ic.RESIZE_CASES if c.method == "bicubic"}
    assert {62, 64} <= taps and max(taps) == ic.MAX_TAPS
    assert {c.view.ow for c in ic.WARP_CASES} >= {1, ic.WARP_LANES - 1, ic.WARP_LANES, ic.WARP_LANES + 1}
    assert all(c.view.oh <= 4 for c in ic.WARP_CASES if c.view.ow >= ic.WARP_LANES - 1)
    for dtype in ("u8", "f32"):
        assert {c.shape[2] for c in ic.WARP_CASES if c.dtype == dtype} >= {1, 2, 3, 4}
    assert {c.fill for c in ic.WARP_CASES if c.dtype == "u8"} >= {0, 9, 255}
    assert {c.fill for c in ic.WARP_CASES if c.dtype == "f32"} == {0.25}
    for c in ic.WARP_CASES:
        if c.dtype == "f32" and c.shape[0] * c.shape[1] >= 100:
            s = ic.warp_source(c.name)
            assert np.nanmin(s) < -0.3 and np.nanmax(s) > 1.3
    assert max(c.shape[0] * c.shape[1] for c in ic.RESIZE_CASES + ic.WARP_CASES) <= 62 * 40


def test_identity_on_the_pixel_grid_returns_the_source_bytes():
    for name in ("identity-u8", "identity-f32"):
        c, s = ic.WARP_BY_NAME[name], ic.warp_source(name)
        for method, m in (("nearest", 0), ("bilinear", 1), ("bicubic", 2)):
            out = ic.oracle_warp(name, method)
            # the view starts at world (-1, -1): source pixel (1, 1) is canvas pixel (2, 2), 0-based
            hi_y, hi_x = c.shape[0] - m, c.shape[1] - m
            lo = 1 if m == 2 else 0
            want = s[lo:hi_y, lo:hi_x]
            if method == "bicubic" and c.dtype == "f32":
                want = np.clip(want, 0.0, 1.0)
            assert same(out[2 + lo:2 + hi_y, 2 + lo:2 + hi_x], want), (name, method)
            assert int(ic.oracle_valid(name, method).sum()) == (hi_y - lo) * (hi_x - lo)


def test_the_perspective_case_has_a_zero_third_coordinate_on_one_column():
    """w = sign(w) max(|w|, 1e-12) leaves w = 0 at 0: the column X = 8 has non-finite source coordinates and takes the fill
    value; on its far side w is negative."""
    c = ic.WARP_BY_NAME["persp-w0-u8"]
    X = c.view.x0 + np.arange(c.view.ow) * c.view.sx
    w = 1.0 - 0.125 * X
    col = int(np.nonzero(w == 0)[0][0])
    assert X[col] == 8.0 and (w[:col] > 0).all() and (w[col + 1:] < 0).all() and col + 1 < c.view.ow
    for method in c.methods:
        assert not ic.oracle_valid(c.name, method)[:, col:].any()
    c = ic.WARP_BY_NAME["tiny-w-u8"]
    X = c.view.x0 + np.arange(c.view.ow) * c.view.sx
    w = (0.25 * X - 1.0) * 1e-12  # s2 of this H
    assert ((np.abs(w) < 1e-12) & (w > 0)).sum() >= 3 and (np.abs(w) > 1e-12).sum() >= 3


def test_half_scales_and_the_half_shift_produce_rounding_ties_and_the_checkerboard_both_clamps():
    for name in ic.TIE_RESIZE_CASES:
        stats = {}
        restated_resize(ic.RESIZE_BY_NAME[name], stats=stats)
        assert stats["ties"] >= 20, (name, stats)
    for name in ic.TIE_WARP_CASES:
        stats = {}
        restated_warp(ic.WARP_BY_NAME[name], "bilinear", stats=stats)
        assert stats["ties"] >= 20, (name, stats)
    for name in ic.CLAMP_RESIZE_CASES:
        stats = {}
        restated_resize(ic.RESIZE_BY_NAME[name], stats=stats)
        ref = ic.oracle_resize(name)
        assert stats["over"] >= 20 and stats["under"] >= 20 and ref.min() == 0 and ref.max() == 255, (name, stats)


def test_nan_in_a_single_precision_source():
    """nearest copies a NaN, bilinear spreads it over the pixels whose four taps meet it (a zero weight does not stop it), and
    bicubic's max(0, min(1, .)) turns it into 1: MATLAB's min and max skip a NaN."""
    name = ic.NAN_SOURCE_CASES[0]
    c, src = ic.WARP_BY_NAME[name], ic.warp_source(name)
    assert int(np.isnan(src).sum()) == len(ic.NAN_PIXELS)
    near, bil, cub = (ic.oracle_warp(name, m) for m in ic.METHODS)
    assert np.isnan(near).sum() >= 3 and np.isnan(bil).sum() > np.isnan(near).sum() and not np.isnan(cub).any()
    v = c.view
    clean = oracle.image_warp_h(np.where(np.isnan(src), np.float32(0.5), src), np.array(c.H), v.oh, v.ow, v.x0, v.y0, v.sx, v.sy, c.fill,
                                method="bicubic")
    touched = cub.view(np.uint32) != clean.view(np.uint32)
    assert touched.sum() >= 16 and np.all(cub[touched] == 1.0)


# ---- discriminating power ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deviation", DEVIATIONS)
def test_every_deviation_changes_the_output_of_some_case(deviation):
    dev = frozenset([deviation])
    caught = []
    if deviation in DEVIATIONS_RESIZE:
        hit = [c.name for c in ic.RESIZE_CASES if not same(restated_resize(c, dev), ic.oracle_resize(c.name))]
        assert hit, f"no imresize case tells '{deviation}' from the rule"
        caught += hit
    if deviation in DEVIATIONS_WARP:
        hit = [f"{c.name}/{m}" for c, m in ic.warp_runs() if not same(restated_warp(c, m, dev), ic.oracle_warp(c.name, m))]
        assert hit, f"no imageWarp case tells '{deviation}' from the rule"
        caught += hit
    print(f"{deviation}: caught by {len(caught)} runs, e.g. {caught[:4]}")


# ---- resizeImagesToLimits on the host ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ic.LIMIT_MODES)
@pytest.mark.parametrize("s", ic.LIMIT_SETS, ids=lambda s: s.name)
def test_limits_statement(s, mode):
    imgs = list(ic.limit_images(s.name))
    HL, WL = s.limits
    out = ic.limits_statement(imgs, HL, WL, mode)
    assert len(out) == len(imgs) and all(o.dtype == np.uint8 and o.ndim == i.ndim for o, i in zip(out, imgs))
    over = any(h > HL or w > WL for h, w in (i.shape[:2] for i in imgs))
    if s.name.startswith("a-"):
        assert not over and all(o is i for o, i in zip(out, imgs))  # :29-42, in every mode
        return
    assert over == (s.name[0] in "cdef")
    if mode == "fit":
        assert len({o.shape[:2] for o in out}) == 1 and out[0].shape[0] <= HL and out[0].shape[1] <= WL
    else:
        assert all(o.shape[:2] == (HL, WL) for o in out)
    if mode == "pad":
        for o, i in zip(out, imgs):
            h, w = i.shape[:2]
            sc = min(HL / h, WL / w)
            J = oracle.imresize_u8(i, sc, "bicubic") if sc < 1 else i
            top, left = (HL - J.shape[0]) // 2, (WL - J.shape[1]) // 2  # floor: the odd pixel goes after
            assert np.array_equal(o[top:top + J.shape[0], left:left + J.shape[1]], J)
            assert np.array_equal(o[0, left:left + J.shape[1]], J[0]) and np.array_equal(o[-1, left:left + J.shape[1]], J[-1])
            assert np.array_equal(o[top:top + J.shape[0], 0], J[:, 0]) and np.array_equal(o[top:top + J.shape[0], -1], J[:, -1])


def test_limit_set_f_has_odd_pad_and_crop_differences():
    s = ic.LIMITS_BY_NAME["f-odd-differences"]
    HL, WL = s.limits
    pad_odd, crop_odd = 0, 0
    for h, w in (shp[:2] for shp in s.shapes):
        sc = min(HL / h, WL / w)
        h1, w1 = (math.ceil(h * sc), math.ceil(w * sc)) if sc < 1 else (h, w)
        pad_odd += (HL - h1) % 2 + (WL - w1) % 2
        sc = max(HL / h, WL / w)
        crop_odd += (math.ceil(h * sc) - HL) % 2 + (math.ceil(w * sc) - WL) % 2
    assert pad_odd >= 2 and crop_odd >= 2, (pad_odd, crop_odd)


def test_limits_statement_rejects_what_the_reference_rejects():
    img = ic.limit_images("a-equal-within")[0]
    for bad in ([], ()):
        with pytest.raises(ValueError):
            ic.limits_statement(bad, 40, 50, "fit")
    for HL, WL in ((0, 50), (40, 0), (-1, 50), (40, -3.5)):
        with pytest.raises(ValueError):
            ic.limits_statement([img], HL, WL, "fit")
    with pytest.raises(ValueError):
        ic.limits_statement([img], 40, 50, "stretch")


# ---- transformPointsForwardScratch / outputLimitsScratch ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ip():
    import apsamd

    return import_module(apsamd.__name__ + ".imageProcessing")


def direct_forward(H, pts):
    """[u v] = (H11 x + H12 y + H13, H21 x + H22 y + H23) / (H31 x + H32 y + H33), NaN where |w| < 1e-12
    (transformPointsForwardScratch.m:63-74)."""
    out = []
    for x, y in pts:
        q = [H[r][0] * x + H[r][1] * y + H[r][2] for r in range(3)]
        out.append((q[0] / q[2], q[1] / q[2]) if abs(q[2]) >= 1e-12 else (math.nan, math.nan))
    return np.array(out, np.float64).reshape(-1, 2)


# three-term sums without cancellation and one division: a few rounding errors of 2^-53 each; 1e-13 relative is far above them
FORWARD_RTOL = 1e-13


@pytest.mark.parametrize("H", [ic.H_GEN, ((0, -1, 41.3), (1, 0, 0.2), (0, 0, 1)), ((1, 0, 0), (0, 1, 0), (0.125, 0, 1)),
                               ((2.0, 0.5, 1.0), (0.25, 3.0, 2.0), (0.001, 0.002, 0.5))], ids=["gen", "rot90", "persp", "scaled"])
def test_transform_points_forward_equals_the_direct_formula(ip, H):
    rng = np.random.default_rng(5)
    pts = rng.uniform(1.0, 90.0, (40, 2))
    got = ip.transformPointsForwardScratch(np.array(H), pts)
    np.testing.assert_allclose(got, direct_forward(H, pts), rtol=FORWARD_RTOL, atol=0)
    assert ip.transformPointsForwardScratch(np.array(H), np.zeros((0, 2))).shape == (0, 2)


def test_transform_points_forward_gives_nan_below_the_guard(ip):
    H = ((1, 0, 0), (0, 1, 0), (-0.125, 0, 1))  # w = 1 - x / 8
    pts = np.array([[8.0, 3.0], [8.0 + 4e-12, 3.0], [8.0 - 4e-12, -2.0], [8.0 + 1.6e-11, 3.0], [7.0, 1.0]])
    got = ip.transformPointsForwardScratch(np.array(H), pts)
    w = 1.0 - 0.125 * pts[:, 0]
    assert list(np.abs(w) < 1e-12) == [True, True, True, False, False]
    assert np.isnan(got[:3]).all() and np.isfinite(got[3:]).all()
    np.testing.assert_allclose(got[3:], direct_forward(H, pts[3:]), rtol=FORWARD_RTOL, atol=0)


def test_output_limits_are_the_nan_extrema_over_the_nine_points(ip):
    xl, yl = (0.5, 50.5), (0.5, 40.5)
    nine = [(x, y) for y in (yl[0], 0.5 * (yl[0] + yl[1]), yl[1]) for x in (xl[0], 0.5 * (xl[0] + xl[1]), xl[1])]
    for H in (ic.H_GEN, ((0, -1, 41.3), (1, 0, 0.2), (0, 0, 1)), ((-1, 0, 51.25), (0, 1, 0), (0, 0, 1))):
        uv = direct_forward(H, nine)
        (x0, x1), (y0, y1) = ip.outputLimitsScratch(np.array(H), xl, yl)
        np.testing.assert_allclose([x0, x1, y0, y1], [uv[:, 0].min(), uv[:, 0].max(), uv[:, 1].min(), uv[:, 1].max()],
                                   rtol=FORWARD_RTOL, atol=0)
    # w = 1 - x / 50.5 vanishes on the right edge: its three points are NaN and the extrema come from the other six
    H = ((1, 0, 0), (0, 1, 0), (-1 / 50.5, 0, 1))
    uv = direct_forward(H, nine)
    assert np.isnan(uv[:, 0]).sum() == 3
    (x0, x1), (y0, y1) = ip.outputLimitsScratch(np.array(H), xl, yl)
    np.testing.assert_allclose([x0, x1, y0, y1], [np.nanmin(uv[:, 0]), np.nanmax(uv[:, 0]), np.nanmin(uv[:, 1]), np.nanmax(uv[:, 1])],
                               rtol=FORWARD_RTOL, atol=0)
    assert np.isfinite([x0, x1, y0, y1]).all()
