"""Host-side mirror of PP/renderPanorama/renderPanorama.m: option defaults, bounds and canvas sizing stay
on the host in float64 exactly as the reference computes them; the tile loop (rays, sampling, fusion,
multiband blending, paint) runs on the device through aps_render.

Cameras are dicts with 'K' and 'R' (3x3, world->camera), optionally 'noRotation' and 'H2refined'
(cameras struct, initializeCameraMatrices.m:114-122).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import check, lib, ptr

_MODES = {"cylindrical": _capi.APS_PROJ_CYLINDRICAL, "spherical": _capi.APS_PROJ_SPHERICAL,
          "equirectangular": _capi.APS_PROJ_SPHERICAL, "planar": _capi.APS_PROJ_PLANAR,
          "perspective": _capi.APS_PROJ_PLANAR, "stereographic": _capi.APS_PROJ_STEREOGRAPHIC,
          # not in the reference (its README's "inclusion of other projections"); DESIGN.md, "Projection contract"
          "miller": _capi.APS_PROJ_MILLER, "fisheye": _capi.APS_PROJ_FISHEYE, "panini": _capi.APS_PROJ_PANINI}
_PLANE_MODES = ("planar", "perspective", "panini")  # asymmetric bounds about Rref, planarBounds' structure
_DISC_MODES = ("stereographic", "fisheye")          # a centred square about Rref, stereographicBounds' structure
_BLEND = {"none": _capi.APS_BLEND_NONE, "linear": _capi.APS_BLEND_LINEAR, "multiband": _capi.APS_BLEND_MULTIBAND}
_POLICY = {"last": _capi.APS_NONE_LAST, "first": _capi.APS_NONE_FIRST, "maxangle": _capi.APS_NONE_MAXANGLE}
_MULTIBAND_WEIGHTS = ("tent", "maxweight")


def multiband_weights(opts):
    """opts['multibandWeights'] for a multiband blend: 'tent' (default: the reference's normalised tent weights in every
    band) or 'maxweight' (Brown & Lowe Eq. 15-19: each band blended over the partition by largest weight; DESIGN.md,
    "Max-weight multiband contract").  The key is read only with blending = 'multiband'; any other value is a ValueError."""
    if str(opts.get("blending", "multiband")).lower() != "multiband":
        return "tent"
    v = opts.get("multibandWeights", "tent")
    if not isinstance(v, str) or v.lower() not in _MULTIBAND_WEIGHTS:
        raise ValueError(f"multibandWeights must be 'tent' or 'maxweight', not {v!r}")
    return v.lower()


def blend_mode(opts):
    """The APS_BLEND_* value of opts['blending'] and opts['multibandWeights'] (None for an unknown blending)."""
    mode = _BLEND.get(str(opts["blending"]).lower())
    if mode == _capi.APS_BLEND_MULTIBAND and multiband_weights(opts) == "maxweight":
        mode = _capi.APS_BLEND_MULTIBAND_MAXWEIGHT
    return mode


def default_opts(opts, cameras, refIdx):
    """renderPanorama.m:41-71."""
    o = dict(opts or {})
    o.setdefault("fPan", float(np.asarray(cameras[refIdx]["K"])[0, 0]))
    for k, v in (("resScale", 1.0), ("anglePower", 1), ("cropBorder", True), ("margin", 0.01),
                 ("tile", None), ("maxMegapixel", 50), ("robustPct", (1, 99)), ("uvAbsCap", 8.0),
                 ("pixelPad", 24), ("autoRef", True), ("canvasColor", "black"),
                 ("gainCompensation", True), ("blending", "multiband"), ("pyrLevels", 3),
                 ("pyrSigma", 1.0), ("composeNonePolicy", "last")):
        o.setdefault(k, v)
    return o


_GRID_CACHE = {}


def _grid_points(H, W, nx, ny, border):
    """The sample pixels of the bounds functions for one image size: 48 x 32 interior grid in MATLAB's U(:) order and,
    for the planar / stereographic bounds, 4 x `border` edge samples (renderPanorama.m:1524-1530,1612-1625)."""
    key = (int(H), int(W), nx, ny, border)
    xy1 = _GRID_CACHE.get(key)
    if xy1 is None:
        xs = np.linspace(1, W, nx)
        ys = np.linspace(1, H, ny)
        U, V = np.meshgrid(xs, ys)
        u = U.T.reshape(-1)  # MATLAB U(:) walks column-major
        v = V.T.reshape(-1)
        if border:
            xb = np.linspace(1, W, border)
            yb = np.linspace(1, H, border)
            u = np.concatenate([u, xb, xb, np.ones(border), W * np.ones(border)])
            v = np.concatenate([v, np.ones(border), H * np.ones(border), yb, yb])
        xy1 = np.stack([u, v, np.ones_like(u)])
        if len(_GRID_CACHE) > 64:
            _GRID_CACHE.clear()
        _GRID_CACHE[key] = xy1
    return xy1


_RAYC_CACHE = {}


def _solve_K(Ks, B):
    """K \\ B for a stack of intrinsic matrices (n x 3 x 3) and right-hand sides (n x 3 x m).  MATLAB's mldivide takes the
    triangular solver for an upper-triangular K (every pinhole K is): back substitution, which is also what the oracle
    does (oracle/bounds_oracle.c::solve_K) and a tenth of the cost of one LAPACK factorisation per camera.  Any other K
    goes through the general solver."""
    Ks = np.asarray(Ks, np.float64)
    if np.all(Ks[:, 1, 0] == 0) and np.all(Ks[:, 2, 0] == 0) and np.all(Ks[:, 2, 1] == 0):
        k = lambda r, c: Ks[:, r, c][:, None]  # noqa: E731
        x3 = B[:, 2] / k(2, 2)
        x2 = (B[:, 1] - k(1, 2) * x3) / k(1, 1)
        x1 = (B[:, 0] - k(0, 1) * x2 - k(0, 2) * x3) / k(0, 0)
        return np.stack([x1, x2, x3], axis=1)
    return np.linalg.solve(Ks, B)


def _grid_rays(cam, H, W, nx=48, ny=32, border=0):
    pts = _grid_points(H, W, nx, ny, border)
    rayC = _solve_K(np.asarray(cam["K"], np.float64)[None], pts[None])[0]
    return np.asarray(cam["R"], np.float64).T @ rayC


def _all_grid_rays(cams, imgSize, border=0, stacked=False):
    """_grid_rays of every camera, batched per image size (one LAPACK call and one matrix product for all cameras of
    a size; the per-camera results are the same numbers as the one-at-a-time form).  stacked: the per-size stacks
    (n_cameras_of_that_size x 3 x points) instead of one array per camera, for callers that only reduce over everything."""
    out = [None] * len(cams)
    stacks = []
    groups = {}
    for i in range(len(cams)):
        groups.setdefault((int(imgSize[i][0]), int(imgSize[i][1])), []).append(i)
    for (H, W), ids in groups.items():
        xy1 = _grid_points(H, W, 48, 32, border)
        Ks = np.stack([np.asarray(cams[i]["K"], np.float64) for i in ids])
        Rt = np.stack([np.asarray(cams[i]["R"], np.float64).T for i in ids])
        # the camera-frame rays depend on the intrinsics and the image size only: kept from call to call (a video or a
        # re-render with refined rotations solves nothing again)
        key = (Ks.tobytes(), H, W, border)
        rayC = _RAYC_CACHE.get(key)
        if rayC is None:
            if len(_RAYC_CACHE) >= 8:
                _RAYC_CACHE.clear()
            rayC = _RAYC_CACHE[key] = _solve_K(Ks, np.broadcast_to(xy1, (len(ids),) + xy1.shape))
        rays = Rt @ rayC
        stacks.append(rays)
        for q, i in enumerate(ids):
            out[i] = rays[q]
    return stacks if stacked else out


def sphericalBounds(cams, imgSize):
    """renderPanorama.m:1544-1579."""
    tmin = pmin = math.inf
    tmax = pmax = -math.inf

    def ext(r):
        x, y, z = r[:, 0], r[:, 1], r[:, 2]
        th = np.arctan2(x, z)
        ph = np.arctan2(y, np.hypot(x, z))
        return th.min(), th.max(), ph.min(), ph.max()

    # (Round 5: the same evaluation cut into camera chunks on four host threads is no faster - 0.88 against 0.73 ms for 64
    # cameras on the GPU box's host - so it stays one piece.)
    for rays in _all_grid_rays(cams, imgSize, stacked=True):  # (all cameras of a size at once: the same elementwise values)
        a, b, c, d = ext(rays)
        tmin, tmax = min(tmin, a), max(tmax, b)
        pmin, pmax = min(pmin, c), max(pmax, d)
    return tmin, tmax, pmin, pmax


def cylindricalBounds(cams, imgSize):
    """renderPanorama.m:1507-1542."""
    tmin = hmin = math.inf
    tmax = hmax = -math.inf
    for rays in _all_grid_rays(cams, imgSize, stacked=True):
        x, y, z = rays[:, 0], rays[:, 1], rays[:, 2]
        th = np.arctan2(x, z)
        hh = y / np.hypot(x, z)
        tmin, tmax = min(tmin, th.min()), max(tmax, th.max())
        hmin, hmax = min(hmin, hh.min()), max(hmax, hh.max())
    return tmin, tmax, hmin, hmax


def _prctile(x, p):
    """MATLAB prctile: linear interpolation with sample i at 100*(i-0.5)/n percent."""
    x = np.sort(np.asarray(x, np.float64))
    n = x.size
    pos = p / 100.0 * n + 0.5  # 1-based fractional rank
    pos = min(max(pos, 1.0), float(n))
    lo = int(math.floor(pos))
    hi = min(lo + 1, n)
    return x[lo - 1] + (pos - lo) * (x[hi - 1] - x[lo - 1])


def planarBounds(cams, imgSize, Rref, robustPct, uvAbsCap):
    """renderPanorama.m:1581-1665."""
    umin = vmin = math.inf
    umax = vmax = -math.inf
    for rays in _all_grid_rays(cams, imgSize, border=512):
        rayR = np.asarray(Rref, np.float64) @ rays
        zr = rayR[2]
        m = zr > 1e-4
        if not m.any():
            continue
        ur, vr = rayR[0, m] / zr[m], rayR[1, m] / zr[m]
        if np.isfinite(uvAbsCap) and uvAbsCap > 0:
            ur = np.clip(ur, -uvAbsCap, uvAbsCap)
            vr = np.clip(vr, -uvAbsCap, uvAbsCap)
        umin, umax = min(umin, _prctile(ur, robustPct[0])), max(umax, _prctile(ur, robustPct[1]))
        vmin, vmax = min(vmin, _prctile(vr, robustPct[0])), max(vmax, _prctile(vr, robustPct[1]))
    if not (np.isfinite(umin) and np.isfinite(umax)) or umin >= umax:
        umin, umax = -1.0, 1.0
    if not (np.isfinite(vmin) and np.isfinite(vmax)) or vmin >= vmax:
        vmin, vmax = -1.0, 1.0
    return umin, umax, vmin, vmax


def stereographicBounds(cams, imgSize, Rref, robustPct, absCap):
    """renderPanorama.m:1667-1754."""
    amin = bmin = math.inf
    amax = bmax = -math.inf
    for rays in _all_grid_rays(cams, imgSize, border=512):
        rayR = np.asarray(Rref, np.float64) @ rays
        nr = np.sqrt((rayR ** 2).sum(0))
        xr, yr, zr = rayR / nr
        den = 1 + zr
        valid = den > 1e-6
        if not valid.any():
            continue
        a, b = xr[valid] / den[valid], yr[valid] / den[valid]
        if np.isfinite(absCap) and absCap > 0:
            a = np.clip(a, -absCap, absCap)
            b = np.clip(b, -absCap, absCap)
        amin, amax = min(amin, _prctile(a, robustPct[0])), max(amax, _prctile(a, robustPct[1]))
        bmin, bmax = min(bmin, _prctile(b, robustPct[0])), max(bmax, _prctile(b, robustPct[1]))
    if not (np.isfinite(amin) and np.isfinite(amax)) or amin >= amax:
        amin, amax = -1.0, 1.0
    if not (np.isfinite(bmin) and np.isfinite(bmax)) or bmin >= bmax:
        bmin, bmax = -1.0, 1.0
    return amin, amax, bmin, bmax


def millerHeight(ph):
    """The Miller cylindrical projection's canvas height of the elevation ph (f64): 1.25 asinh(tan(0.8 ph)); the poles
    lie at +-2.3034.  Its inverse, 1.25 atan(sinh(0.8 y)), is what the device evaluates per canvas row."""
    return 1.25 * np.arcsinh(np.tan(0.8 * np.asarray(ph, np.float64)))


MILLER_POLE = 1.25 * math.asinh(math.tan(0.4 * math.pi))  # 2.3034...: the canvas height of a pole


def millerBounds(cams, imgSize):
    """sphericalBounds with both elevation limits mapped through millerHeight (monotonic, so the extrema map to the extrema)."""
    tmin, tmax, pmin, pmax = sphericalBounds(cams, imgSize)
    return tmin, tmax, float(millerHeight(pmin)), float(millerHeight(pmax))


def fisheyeBounds(cams, imgSize, Rref, robustPct):
    """stereographicBounds' structure (512-sample border grid, percentiles per image, +-1 fallbacks) for the equidistant
    azimuthal map about Rref: theta = acos(z) of the unit ray, (a, b) = theta * (x, y) / hypot(x, y), (0, 0) on the axis.
    |(a, b)| <= pi, so there is nothing to cap."""
    amin = bmin = math.inf
    amax = bmax = -math.inf
    for rays in _all_grid_rays(cams, imgSize, border=512):
        rayR = np.asarray(Rref, np.float64) @ rays
        nr = np.sqrt((rayR ** 2).sum(0))
        xr, yr, zr = rayR / nr
        theta = np.arccos(np.clip(zr, -1.0, 1.0))
        rho = np.hypot(xr, yr)
        with np.errstate(all="ignore"):
            k = np.where(rho > 0, theta / np.where(rho > 0, rho, 1.0), 0.0)
        a, b = k * xr, k * yr
        amin, amax = min(amin, _prctile(a, robustPct[0])), max(amax, _prctile(a, robustPct[1]))
        bmin, bmax = min(bmin, _prctile(b, robustPct[0])), max(bmax, _prctile(b, robustPct[1]))
    if not (np.isfinite(amin) and np.isfinite(amax)) or amin >= amax:
        amin, amax = -1.0, 1.0
    if not (np.isfinite(bmin) and np.isfinite(bmax)) or bmin >= bmax:
        bmin, bmax = -1.0, 1.0
    return amin, amax, bmin, bmax


def paniniBounds(cams, imgSize, Rref, robustPct, uvAbsCap):
    """planarBounds' structure for the Pannini map (d = 1) about Rref: on unit rays, hz = hypot(x, z), valid where
    hz + z > 1e-4 (everything but the half plane straight behind the axis), a = 2 x / (hz + z), b = 2 y / (hz + z)."""
    umin = vmin = math.inf
    umax = vmax = -math.inf
    for rays in _all_grid_rays(cams, imgSize, border=512):
        rayR = np.asarray(Rref, np.float64) @ rays
        xr, yr, zr = rayR / np.sqrt((rayR ** 2).sum(0))
        den = np.hypot(xr, zr) + zr
        m = den > 1e-4
        if not m.any():
            continue
        ur, vr = 2.0 * xr[m] / den[m], 2.0 * yr[m] / den[m]
        if np.isfinite(uvAbsCap) and uvAbsCap > 0:
            ur = np.clip(ur, -uvAbsCap, uvAbsCap)
            vr = np.clip(vr, -uvAbsCap, uvAbsCap)
        umin, umax = min(umin, _prctile(ur, robustPct[0])), max(umax, _prctile(ur, robustPct[1]))
        vmin, vmax = min(vmin, _prctile(vr, robustPct[0])), max(vmax, _prctile(vr, robustPct[1]))
    if not (np.isfinite(umin) and np.isfinite(umax)) or umin >= umax:
        umin, umax = -1.0, 1.0
    if not (np.isfinite(vmin) and np.isfinite(vmax)) or vmin >= vmax:
        vmin, vmax = -1.0, 1.0
    return umin, umax, vmin, vmax


def canvas_geometry(cameras, imgSize, mode, refIdx, opts):
    """Bounds + canvas size (renderPanorama.m:84-232).  Returns dict(mode, H, W, fPan, o0, o1, Rref, refIdx).  'fisheye' is
    sized like 'stereographic' (a centred square, autoRef by its area) and 'panini' like 'planar'; 'miller' like 'spherical'."""
    mode = str(mode).lower()
    if mode not in _MODES:
        raise ValueError("mode must be cylindrical, spherical, or planar/perspective")
    o = opts
    f = float(o["fPan"])
    n = len(cameras)
    if mode in _PLANE_MODES + _DISC_MODES and o["autoRef"]:  # :84-122
        best, best_idx = math.inf, refIdx
        for ii in range(n):
            Rr = cameras[ii]["R"]
            if mode in _DISC_MODES:
                if mode == "stereographic":
                    a0, a1, b0, b1 = stereographicBounds(cameras, imgSize, Rr, o["robustPct"], o["uvAbsCap"])
                else:
                    a0, a1, b0, b1 = fisheyeBounds(cameras, imgSize, Rr, o["robustPct"])
                ext = max(abs(a0), abs(a1), abs(b0), abs(b1)) * (1 + 2 * o["margin"]) + o["pixelPad"] / f
                Wi = max(1, math.ceil(2 * f * ext * o["resScale"]))
                area = float(Wi) * Wi
            else:
                plane = paniniBounds if mode == "panini" else planarBounds
                u0, u1, v0, v1 = plane(cameras, imgSize, Rr, o["robustPct"], o["uvAbsCap"])
                du, dv = u1 - u0, v1 - v0
                u0, u1 = u0 - o["margin"] * du - o["pixelPad"] / f, u1 + o["margin"] * du + o["pixelPad"] / f
                v0, v1 = v0 - o["margin"] * dv - o["pixelPad"] / f, v1 + o["margin"] * dv + o["pixelPad"] / f
                area = float(max(1, math.ceil(f * (u1 - u0) * o["resScale"]))) * max(1, math.ceil(f * (v1 - v0) * o["resScale"]))
            if area < best:
                best, best_idx = area, ii
        refIdx = best_idx
    Rref = np.asarray(cameras[refIdx]["R"], np.float64)
    rs = o["resScale"]
    if mode == "cylindrical":
        a0, a1, b0, b1 = cylindricalBounds(cameras, imgSize)
    elif mode in ("spherical", "equirectangular"):
        a0, a1, b0, b1 = sphericalBounds(cameras, imgSize)
    elif mode == "miller":
        a0, a1, b0, b1 = millerBounds(cameras, imgSize)
    elif mode in ("planar", "perspective"):
        a0, a1, b0, b1 = planarBounds(cameras, imgSize, Rref, o["robustPct"], o["uvAbsCap"])
    elif mode == "panini":
        a0, a1, b0, b1 = paniniBounds(cameras, imgSize, Rref, o["robustPct"], o["uvAbsCap"])
    else:
        if mode == "stereographic":
            a0, a1, b0, b1 = stereographicBounds(cameras, imgSize, Rref, o["robustPct"], o["uvAbsCap"])
        else:
            a0, a1, b0, b1 = fisheyeBounds(cameras, imgSize, Rref, o["robustPct"])
        ext = max(abs(a0), abs(a1), abs(b0), abs(b1))
        a0, a1, b0, b1 = -ext, ext, -ext, ext
    da, db = a1 - a0, b1 - b0
    a0, a1 = a0 - o["margin"] * da, a1 + o["margin"] * da
    b0, b1 = b0 - o["margin"] * db, b1 + o["margin"] * db
    if mode == "miller":  # the margin must not push rows past a pole: there the elevation runs beyond 90 degrees and the ray
        b0, b1 = max(b0, -MILLER_POLE), min(b1, MILLER_POLE)  # wraps to the opposite azimuth ("Projection contract")
    if mode in _PLANE_MODES + _DISC_MODES:
        a0, a1 = a0 - o["pixelPad"] / f, a1 + o["pixelPad"] / f
        b0, b1 = b0 - o["pixelPad"] / f, b1 + o["pixelPad"] / f
    W = max(1, math.ceil(f * (a1 - a0) * rs))
    H = max(1, math.ceil(f * (b1 - b0) * rs))
    if mode in _PLANE_MODES + _DISC_MODES:  # global pixel cap (:170-177)
        maxPixel = round(o["maxMegapixel"] * 1e6)
        if float(H) * float(W) > maxPixel:
            s = math.sqrt(maxPixel / (float(H) * float(W)))
            rs = rs * s
            W = max(1, math.ceil(f * (a1 - a0) * rs))
            H = max(1, math.ceil(f * (b1 - b0) * rs))
    return {"mode": mode, "H": int(H), "W": int(W), "fPan": f, "o0": float(a0), "o1": float(b0),
            "Rref": Rref, "refIdx": refIdx}


def effective_tile(opts, geo):
    """The tile side renderPanorama uses for a canvas: opts['tile'] when given, else 2048 clamped to the canvas."""
    if opts.get("tile") is not None:
        return tuple(int(v) for v in opts["tile"])
    H, W = int(geo["H"]), int(geo["W"])
    side = max(512, min(2048, H, W)) if min(H, W) >= 512 else min(H, W)
    return (side, side)


def cropNonzeroBbox(panorama, canvasColor="black"):
    """[panoCropped, rect, didCrop] = cropNonzeroBbox(panorama, canvasColor) (renderPanorama.m:1459-1504): bounding box of
    rgb2gray(panorama) > 0 (or < 255 on a white canvas), 6 px pad; the box is a device reduction (aps_crop_nonzero_bbox),
    the crop itself a slice (a view of a resident panorama, no copy).  rect = (r1, r2, c1, c2), 1-based inclusive."""
    H, W = int(panorama.shape[0]), int(panorama.shape[1])
    if _capi.is_torch(panorama):
        src = panorama if panorama.is_contiguous() else panorama.contiguous()
    else:
        src = np.ascontiguousarray(panorama, np.uint8)
    if src.ndim == 2:
        src = src[..., None].repeat(3, axis=2) if not _capi.is_torch(src) else src[..., None].expand(H, W, 3).contiguous()
    rect = np.zeros(4, np.int64)
    did = C.c_int(0)
    check(lib.aps_crop_nonzero_bbox(ptr(src), H, W, _capi.APS_IMG_U8_HWC, 1 if str(canvasColor).lower() == "white" else 0,
                                    ptr(rect), C.byref(did)))
    r1, r2, c1, c2 = (int(v) for v in rect)
    if not did.value:
        return panorama, (1, H, 1, W), False
    return panorama[r1 - 1:r2, c1 - 1:c2], (r1, r2, c1, c2), True


# ---- rgbAnnotation: outlines and numbers (renderPanorama.m:438-477, :653-679, :1148-1280) -----------------------------
def vivid_palette(n):
    """n x 3 uint8 outline colours.  The reference's brightColors draws from rand and cannot be reproduced; this is a stated
    deterministic stand-in: hue_k = frac(k * (sqrt(5) - 1) / 2), k = 0 .. n-1 (golden-ratio steps), saturation = value = 1,
    the usual six-sector HSV -> RGB in f64, each channel floor(255 v + 0.5).  Every row has a channel at 255."""
    k = np.arange(int(n), dtype=np.float64)
    h6 = 6.0 * np.mod(k * ((math.sqrt(5.0) - 1.0) / 2.0), 1.0)
    sector = np.floor(h6).astype(np.int64) % 6
    f = h6 - np.floor(h6)
    one, zero = np.ones_like(f), np.zeros_like(f)
    table = np.stack([np.stack([one, f, zero], 1), np.stack([1 - f, one, zero], 1), np.stack([zero, one, f], 1),
                      np.stack([zero, 1 - f, one], 1), np.stack([f, zero, one], 1), np.stack([one, zero, 1 - f], 1)])
    rgb = table[sector, np.arange(int(n))] if n else np.zeros((0, 3))
    return np.floor(255.0 * rgb + 0.5).astype(np.uint8)


def warped_boxes(cameras, imgSize, geo):
    """allWarpedBoxes / warpedBBoxes (renderPanorama.m:1148-1280) for the canvas `geo` (canvas_geometry): the corners
    (1,1), (1,W), (H,W), (H,1) [row, col] of every image as rays rayW = R' * (K \\ [x; y; 1]), through the forward map of
    geo['mode'], in f64.  Returns (polys [n, 4, 2] as x, y; centers [n, 2] = the mean of the four corners), in 1-based
    coordinates of the UNCROPPED canvas: x = (a - o0) * fPan + 1, the exact inverse of the pixel-to-direction map the
    renderer uses (pixel column c looks along a = o0 + (c - 1) / fPan), so an image corner lands on the canvas pixel that
    samples it.  (The reference writes x = (a - o0) * fPan, one pixel up and to the left; DESIGN.md, "Annotation contract".)"""
    mode = geo["mode"]
    f, o0, o1 = float(geo["fPan"]), float(geo["o0"]), float(geo["o1"])
    Rref = np.asarray(geo["Rref"], np.float64)
    n = len(cameras)
    polys = np.zeros((n, 4, 2), np.float64)
    with np.errstate(all="ignore"):
        for i, cam in enumerate(cameras):
            Hc, Wc = float(imgSize[i][0]), float(imgSize[i][1])
            xy1 = np.array([[1.0, Wc, Wc, 1.0], [1.0, 1.0, Hc, Hc], [1.0, 1.0, 1.0, 1.0]])
            rayC = _solve_K(np.asarray(cam["K"], np.float64)[None], xy1[None])[0]
            rayW = np.asarray(cam["R"], np.float64).T @ rayC
            if mode in ("planar", "perspective"):
                rayR = Rref @ rayW
                a, b = rayR[0] / rayR[2], rayR[1] / rayR[2]
            elif mode == "cylindrical":
                a = np.arctan2(rayW[0], rayW[2])
                b = rayW[1] / np.hypot(rayW[0], rayW[2])
            elif mode in ("spherical", "equirectangular"):
                a = np.arctan2(rayW[0], rayW[2])
                b = np.arctan2(rayW[1], np.hypot(rayW[0], rayW[2]))
            elif mode == "stereographic":
                rayR = Rref @ rayW
                xr, yr, zr = rayR / np.sqrt((rayR ** 2).sum(0))
                den = np.maximum(1 + zr, 1e-6)  # :1269
                a, b = xr / den, yr / den
            elif mode == "miller":
                a = np.arctan2(rayW[0], rayW[2])
                b = millerHeight(np.arctan2(rayW[1], np.hypot(rayW[0], rayW[2])))
            elif mode == "fisheye":
                rayR = Rref @ rayW
                xr, yr, zr = rayR / np.sqrt((rayR ** 2).sum(0))
                rho = np.hypot(xr, yr)
                k = np.where(rho > 0, np.arccos(np.clip(zr, -1.0, 1.0)) / np.where(rho > 0, rho, 1.0), 0.0)
                a, b = k * xr, k * yr
            elif mode == "panini":
                rayR = Rref @ rayW
                xr, yr, zr = rayR / np.sqrt((rayR ** 2).sum(0))
                den = np.maximum(np.hypot(xr, zr) + zr, 1e-6)  # (clamped like the stereographic denominator)
                a, b = 2.0 * xr / den, 2.0 * yr / den
            else:
                raise ValueError("mode")
            polys[i, :, 0] = (a - o0) * f + 1.0
            polys[i, :, 1] = (b - o1) * f + 1.0
    return polys, polys.mean(axis=1)


def planar_boxes(shapes, tforms, view):
    """The boxes of pureNonRotationalImagesToCanvas (renderPanorama.m:738-742): the corners (x, y) = (1,1), (W,1), (W,H), (1,H)
    through transformPointsForwardScratch, minus the world limits of the canvas; the centre is the mean over the CLOSED
    five-point polygon the reference builds (the first corner counts twice), as written."""
    from .imageProcessing import transformPointsForwardScratch

    n = len(shapes)
    polys, centers = np.zeros((n, 4, 2), np.float64), np.zeros((n, 2), np.float64)
    for k in range(n):
        r, c = float(shapes[k][0]), float(shapes[k][1])
        q = np.asarray(transformPointsForwardScratch(tforms[k], np.array([[1, 1], [c, 1], [c, r], [1, r], [1, 1]], np.float64)),
                       np.float64)
        q = q - np.array([float(view["XWorldLimits"][0]), float(view["YWorldLimits"][0])])
        polys[k] = q[:4]
        centers[k] = q.mean(axis=0)
    return polys, centers


def annotate_panorama(pano, polys, anchors, colors=None, lineWidth=2):
    """rgbAnnotation = insertText(insertShape(pano, 'Polygon', ...), anchors, 1:numValid) on the device
    (aps_annotate_panorama; the raster rule is DESIGN.md's "Annotation contract").  pano: uint8 H x W x 3 (H x W and
    H x W x 1 are replicated), a numpy array or a torch tensor; the result is a new array of the same kind, resident when
    pano is, and pano is not written.  polys [n, 4, 2] (x, y), anchors [n, 2], 1-based canvas coordinates; colors [n, 3]
    uint8 (default vivid_palette(n)).  Returns (annotated, number of polygons drawn = the highest label)."""
    polys = np.ascontiguousarray(np.asarray(polys, np.float64).reshape(-1, 4, 2))
    n = int(polys.shape[0])
    anchors = np.ascontiguousarray(np.asarray(anchors, np.float64).reshape(-1, 2))
    colors = vivid_palette(n) if colors is None else np.ascontiguousarray(np.asarray(colors).reshape(-1, 3).astype(np.uint8))
    if anchors.shape[0] != n or colors.shape[0] != n:
        raise ValueError("polys, anchors and colors must have one row per polygon")
    from .imageProcessing import drawing_buffers

    drawn = C.c_int(0)
    src, dst, H, W = drawing_buffers(pano, "pano")
    check(lib.aps_annotate_panorama(ptr(src), H, W, ptr(polys), ptr(anchors), ptr(colors), n, int(lineWidth), ptr(dst),
                                    C.byref(drawn)))
    return dst, int(drawn.value)


def _wants_annotation(opts):
    return bool(opts) and bool(opts.get("showPanoramaImgsNums")) and bool(opts.get("showCropBoundingBox"))


def make_image_structs(images, cameras, gains=None):
    n = len(images)
    arr = (_capi.aps_image * n)()
    keep = []
    for i, img in enumerate(images):
        if _capi.is_torch(img):
            t = img.contiguous()
            h, w = t.shape[0], t.shape[1]
            c = 1 if t.dim() == 2 else t.shape[2]
        else:
            t = np.ascontiguousarray(img, np.uint8)
            h, w = t.shape[0], t.shape[1]
            c = 1 if t.ndim == 2 else t.shape[2]
        keep.append(t)
        a = arr[i]
        a.data = ptr(t)
        a.height, a.width, a.channels, a.layout = int(h), int(w), int(c), _capi.APS_IMG_U8_HWC
        K = np.asarray(cameras[i]["K"], np.float64)
        R = np.asarray(cameras[i]["R"], np.float64)
        for e in range(9):
            a.K[e] = K[e % 3, e // 3]
            a.R[e] = R[e % 3, e // 3]
        g = (1.0, 1.0, 1.0) if gains is None else gains[i]
        for ch in range(3):
            a.gain[ch] = float(g[ch])
    return arr, keep


def make_canvas_struct(geo):
    cv = _capi.aps_canvas()
    cv.mode = _MODES[geo["mode"]]
    cv.height, cv.width = geo["H"], geo["W"]
    cv.f_pan, cv.origin0, cv.origin1 = geo["fPan"], geo["o0"], geo["o1"]
    R = np.asarray(geo["Rref"], np.float64)
    for e in range(9):
        cv.R_ref[e] = R[e % 3, e // 3]
    return cv


def make_render_opts(opts):
    ro = _capi.aps_render_opts()
    tile = opts["tile"]
    ro.tile_h, ro.tile_w = int(tile[0]), int(tile[1])
    ro.angle_power = float(opts["anglePower"])
    ro.blending = blend_mode(opts)
    if ro.blending is None:
        raise KeyError(str(opts["blending"]).lower())
    ro.pyr_levels = int(opts["pyrLevels"])
    ro.pyr_sigma = float(opts["pyrSigma"])
    ro.none_policy = _POLICY[str(opts["composeNonePolicy"]).lower()]
    ro.canvas_white = 1 if str(opts["canvasColor"]).lower() == "white" else 0
    return ro


def warpWeights(images):
    """srcWeights = warpWeights(images, numImages) (renderPanorama.m:1282-1312): the separable tent map
    wy * wx of every image, single.  (The tiled render path never materialises it: the device samples the
    two 1-D tables; the planar-scan path below warps the map itself, as the reference does.)"""
    out = []
    for im in images:
        h, w = np.asarray(im).shape[:2]

        def tent(n):
            t = np.zeros(n, np.float32)
            a = (n + 1) // 2
            t[:a] = np.linspace(0, 1, a, dtype=np.float64).astype(np.float32) if a > 1 else 1.0
            b = n - n // 2
            t[n // 2:] = np.linspace(1, 0, b, dtype=np.float64).astype(np.float32) if b > 1 else 0.0
            return t

        out.append(np.outer(tent(h), tent(w)).astype(np.float32))
    return out


def _matlab_round(x):
    return float(np.sign(x) * np.floor(abs(x) + 0.5))


def pureNonRotationalImagesToCanvas(images, tforms, outputView, srcWeights, opts=None):
    """[Iw, Ww, xBoxes, yBoxes, centers] = pureNonRotationalImagesToCanvas(...) (renderPanorama.m:701-822):
    every image and its weight map warped to the common canvas with the device imageWarp (bilinear, fill 0,
    valid only where all four taps are inside, imageWarp.m:125-168); weights clamped to [0,1]."""
    from .imageProcessing import imageWarp, transformPointsForwardScratch

    Iw, Ww, xB, yB = [], [], [], []
    centers = np.zeros((len(images), 2))
    Hc, Wc = outputView["ImageSize"]
    for k, im in enumerate(images):
        Ik = np.asarray(im)
        r, c = Ik.shape[:2]
        corners = np.array([[1, 1], [c, 1], [c, r], [1, r], [1, 1]], np.float64)  # (x, y) of :751
        q = transformPointsForwardScratch(tforms[k], corners)
        xB.append(q[:, 0] - outputView["XWorldLimits"][0])
        yB.append(q[:, 1] - outputView["YWorldLimits"][0])
        centers[k] = (xB[-1].mean(), yB[-1].mean())
        Ik = Ik.astype(np.float32) / 255.0 if Ik.dtype == np.uint8 else Ik.astype(np.float32)
        Iwk = imageWarp(Ik, tforms[k], outputView)[:Hc, :Wc]
        Ws = np.ones((r, c), np.float32) if not srcWeights else np.asarray(srcWeights[k], np.float32)
        Wk = imageWarp(Ws, tforms[k], outputView)[:Hc, :Wc]
        Iw.append(Iwk if Iwk.ndim == 3 else Iwk[..., None])
        Ww.append(np.clip(Wk, 0.0, 1.0).astype(np.float32))
    return Iw, Ww, xB, yB, centers


def _planar_args(images, tforms):
    """Checks and marshals the image list and the homographies of the planar entry points (before the library is touched)."""
    n = len(images)
    if n == 0 or len(tforms) != n:
        raise ValueError("images and tforms must be non-empty lists of equal length")
    keep, hs, ws, cs = [], [], [], []
    Hs = np.zeros((n, 9), np.float64)
    for k, (im, T) in enumerate(zip(images, tforms)):
        T = np.asarray(T, np.float64)
        if T.shape != (3, 3):
            raise ValueError(f"tforms[{k}] must be a 3x3 matrix, got {T.shape}")
        Hs[k] = T.T.reshape(9)  # column-major
        if _capi.is_torch(im):
            import torch

            if im.dtype != torch.uint8:
                raise ValueError(f"images[{k}] must be uint8, got {im.dtype}")
            a = im if im.is_contiguous() else im.contiguous()
        else:
            a = np.asarray(im)
            if a.dtype != np.uint8:
                raise ValueError(f"images[{k}] must be uint8, got {a.dtype}")
            a = np.ascontiguousarray(a)
        if a.ndim not in (2, 3) or (a.ndim == 3 and int(a.shape[2]) not in (1, 3)) or min(int(v) for v in a.shape[:2]) < 1:
            raise ValueError(f"images[{k}] must be h x w, h x w x 1 or h x w x 3, got {tuple(a.shape)}")
        keep.append(a)
        hs.append(int(a.shape[0]))
        ws.append(int(a.shape[1]))
        cs.append(1 if a.ndim == 2 else int(a.shape[2]))
    if any(_capi.is_torch(a) and a.is_cuda for a in keep):
        import torch

        torch.cuda.current_stream().synchronize()  # torch produced them; the library reads on its own stream
    pim = (C.c_void_p * n)(*[ptr(a) for a in keep])
    ih, iw, ic = (np.asarray(v, np.int32) for v in (hs, ws, cs))
    return n, keep, pim, ih, iw, ic, Hs


def _planar_view(view):
    Hc, Wc = (int(v) for v in view["ImageSize"])
    if Hc < 1 or Wc < 1:
        raise ValueError("degenerate planar canvas")
    return (Hc, Wc, float(view["XWorldLimits"][0]), float(view["YWorldLimits"][0]), float(view["PixelExtentInWorldX"]),
            float(view["PixelExtentInWorldY"]))


def planar_composite_bytes(shapes, canvas, blending="multiband", levels=3):
    """Device memory (bytes) planar_composite requests for images of `shapes` [(h, w, c), ...] on a canvas (H, W): the
    formula of aps_planar_composite_bytes (include/aps.h).  Host only; ValueError for arguments the composite refuses."""
    ih, iw, ic = (np.asarray([int(s[i]) if len(s) > i else 1 for s in shapes], np.int32) for i in range(3))
    mode = _BLEND.get(str(blending).lower())
    if mode is None:
        raise ValueError("Wrong blening mode.")
    b = int(lib.aps_planar_composite_bytes(len(shapes), ptr(ih), ptr(iw), ptr(ic), int(canvas[0]), int(canvas[1]), mode, int(levels)))
    if b < 0:
        raise ValueError((lib.aps_last_error() or b"").decode("utf-8", "replace"))
    return b


def planar_footprints(shapes, tforms, view):
    """The canvas rectangles planar_composite confines every image to: (rects [N,4] = x0, y0, x1, y1, 0-based half-open,
    whole [N] = the whole-canvas fallback was taken).  Host only (aps_planar_footprints)."""
    n = len(shapes)
    if n == 0 or len(tforms) != n:
        raise ValueError("shapes and tforms must be non-empty lists of equal length")
    Hc, Wc, x0, y0, sx, sy = _planar_view(view)
    ih, iw = (np.asarray([int(s[i]) for s in shapes], np.int32) for i in range(2))
    Hs = np.stack([np.asarray(T, np.float64).T.reshape(9) for T in tforms])
    rects, whole = np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
    check(lib.aps_planar_footprints(n, ptr(ih), ptr(iw), ptr(Hs), Hc, Wc, x0, y0, sx, sy, ptr(rects), ptr(whole)))
    return rects, whole.astype(bool)


def planar_gain_stats(images, tforms, view, ds=4, _entry="aps_planar_gain_stats"):
    """gain_overlap_stats_warped's result for the images warped to `view`, accumulated from the resident float4 layers of the
    planar compositor (aps_planar_gain_stats): no canvas visits the host.  Returns (Nij, sumCi, sumCj) float64."""
    n, keep, pim, ih, iw, ic, Hs = _planar_args(images, tforms)
    Hc, Wc, x0, y0, sx, sy = _planar_view(view)
    Nij = np.zeros((n, n), np.float64, order="F")
    sCi = np.zeros((n, n, 3), np.float64, order="F")
    sCj = np.zeros((n, n, 3), np.float64, order="F")
    check(getattr(lib, _entry)(C.addressof(pim), ptr(ih), ptr(iw), ptr(ic), n, ptr(Hs), Hc, Wc, x0, y0, sx, sy, int(ds),
                               ptr(Nij), ptr(sCi), ptr(sCj)))
    del keep
    return np.ascontiguousarray(Nij), np.ascontiguousarray(sCi), np.ascontiguousarray(sCj)


def planar_gain_stats_compact(images, tforms, view, ds=4):
    """planar_gain_stats from the footprint-compact layers (aps_planar_gain_stats_compact): any number of images up to 65535,
    device memory that follows the footprints.  Same outputs."""
    return planar_gain_stats(images, tforms, view, ds, _entry="aps_planar_gain_stats_compact")


def planar_composite_compact_bytes(shapes, canvas, tforms, view, blending="multiband", levels=3):
    """Device memory (bytes) planar_composite_compact requests: the formula of aps_planar_composite_compact_bytes
    (include/aps.h), which follows the footprints and therefore takes the homographies and the canvas `view` (`canvas` must be
    its ImageSize).  Host only; ValueError for arguments the composite refuses."""
    ih, iw, ic = (np.asarray([int(s[i]) if len(s) > i else 1 for s in shapes], np.int32) for i in range(3))
    mode = _BLEND.get(str(blending).lower())
    if mode is None:
        raise ValueError("Wrong blening mode.")
    if len(tforms) != len(shapes):
        raise ValueError("shapes and tforms must be lists of equal length")
    Hc, Wc, x0, y0, sx, sy = _planar_view(view)
    if (int(canvas[0]), int(canvas[1])) != (Hc, Wc):
        raise ValueError("canvas must be the view's ImageSize")
    Hs = np.stack([np.asarray(T, np.float64).T.reshape(9) for T in tforms]) if len(shapes) else np.zeros((0, 9))
    b = int(lib.aps_planar_composite_compact_bytes(len(shapes), ptr(ih), ptr(iw), ptr(ic), ptr(np.ascontiguousarray(Hs)), Hc, Wc,
                                                   x0, y0, sx, sy, mode, int(levels)))
    if b < 0:
        raise ValueError((lib.aps_last_error() or b"").decode("utf-8", "replace"))
    return b


def planar_composite_compact(images, tforms, view, opts=None, gains=None, device_out=False):
    """planar_composite through the footprint-compact compositor (aps_planar_composite_compact, with
    aps_planar_gain_stats_compact for opts['gainCompensation']): the same bytes for any number of images, every layer stored
    inside its footprint only."""
    return planar_composite(images, tforms, view, opts, gains, device_out, _compact=True)


def planar_composite(images, tforms, view, opts=None, gains=None, device_out=False, _compact=False):
    """panorama = planar_composite(images, tforms, view, opts): the compositing of pureNonRotationalPanoramas
    (renderPanorama.m:519-699) in one device-resident call (aps_planar_composite).  images: uint8 h x w x 3, h x w x 1 or
    h x w, numpy arrays or resident CUDA tensors, sizes may differ; tforms: 3x3 homographies (H2refined); view: the canvas
    (imref2dScratch).  opts: blending, pyrLevels, pyrSigma, canvasColor as pureNonRotationalPanoramas; with
    opts['gainCompensation'] and no `gains` the overlap statistics are taken from the resident layers and solved on the host
    (gainCompensationH).  Returns the uint8 out_h x out_w x 3 panorama (a CUDA tensor with device_out=True), byte-identical to
    the host-orchestrated path."""
    o = {"blending": "multiband", "pyrLevels": 3, "pyrSigma": 1.0, "canvasColor": "black", "sigmaN": 10.0, "sigmag": 0.1}
    o.update(opts or {})
    n, keep, pim, ih, iw, ic, Hs = _planar_args(images, tforms)
    Hc, Wc, x0, y0, sx, sy = _planar_view(view)
    mode = blend_mode(o)
    if mode is None:
        raise ValueError("Wrong blening mode.")
    levels, sigma = int(o["pyrLevels"]), float(o["pyrSigma"])
    if mode in (_capi.APS_BLEND_MULTIBAND, _capi.APS_BLEND_MULTIBAND_MAXWEIGHT):
        if int(o["pyrLevels"]) != o["pyrLevels"] or levels < 1:
            raise ValueError("levels must be a positive integer")
        if sigma <= 0:
            raise ValueError("sigma must be positive")
    if gains is None and o.get("gainCompensation"):
        from .gainCompensation import solve_gains_H

        if n <= 1:
            gains = np.ones((n, 3), np.float32)
        else:
            stats = planar_gain_stats_compact if _compact else planar_gain_stats
            gains = solve_gains_H(*stats(keep, tforms, view, max(1, int(o.get("overlapDownsample", 4)))), o)
    g = None
    if gains is not None:
        g = np.stack([np.broadcast_to(np.asarray(x, np.float32).reshape(-1), (3,)) for x in gains]).astype(np.float32)
        if g.shape != (n, 3):
            raise ValueError("gains must be N x 3")
        g = np.ascontiguousarray(g)
    if device_out:
        import torch

        pano = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device="cuda")
    else:
        pano = np.zeros((Hc, Wc, 3), np.uint8)
    entry = getattr(lib, "aps_planar_composite_compact" if _compact else "aps_planar_composite")
    check(entry(C.addressof(pim), ptr(ih), ptr(iw), ptr(ic), n, ptr(Hs), Hc, Wc, x0, y0, sx, sy, mode, levels, sigma,
                1 if str(o["canvasColor"]).lower() == "white" else 0, ptr(g), ptr(pano), None))
    del keep
    return pano


def _planar_device_covers(images, opts):
    """The inputs the device compositors cover: uint8 images of 1 or 3 channels (one channel count per set).  Returns None
    (the host path), 'device' (aps_planar_composite: at most 64 images) or 'compact' (aps_planar_composite_compact: asked for
    with opts['planarCompositor'] = 'compact', or more than 64 images)."""
    import os

    which = str((opts or {}).get("planarCompositor", "device")).lower()
    if which == "host" or os.environ.get("APS_PLANAR_HOST"):
        return None
    if len(images) < 1:
        return None
    ch = set()
    for im in images:
        if _capi.is_torch(im):
            import torch

            if im.dtype != torch.uint8:
                return None
        elif np.asarray(im).dtype != np.uint8:
            return None
        if im.ndim not in (2, 3) or (im.ndim == 3 and int(im.shape[2]) not in (1, 3)):
            return None
        ch.add(1 if im.ndim == 2 else int(im.shape[2]))
    if len(ch) != 1:
        return None
    return "compact" if which == "compact" or len(images) > 64 else "device"


def _planar_device_composite(route, images, tforms, view, o, gains, device_out):
    """The dense compositor wherever it runs; the compact one when asked for, for more than 64 images, and when the dense
    request (planar_composite_bytes) exceeds opts['planarDenseLimitBytes'] - by default the free device memory at the time
    of the call, which is what the dense call itself compares its request with (APS_E_OOM before any launch)."""
    if route == "device" and o.get("planarDenseLimitBytes") is not None:
        shapes = [(int(im.shape[0]), int(im.shape[1]), 1 if im.ndim == 2 else int(im.shape[2])) for im in images]
        levels = o["pyrLevels"] if str(o["blending"]).lower() == "multiband" else 1
        if planar_composite_bytes(shapes, view["ImageSize"], o["blending"], levels) > int(o["planarDenseLimitBytes"]):
            route = "compact"
    if route == "device":
        try:
            return planar_composite(images, tforms, view, o, gains, device_out)
        except _capi.ApsError as e:
            if e.code != _capi.APS_E_OOM or o.get("planarDenseLimitBytes") is not None:
                raise
    return planar_composite_compact(images, tforms, view, o, gains, device_out)


def pureNonRotationalPanoramas(images, cameras, numImages, opts, gains=None, device_out=False):
    """[panorama, rgbAnnotation] = pureNonRotationalPanoramas(images, cameras, numImages, opts)
    (renderPanorama.m:519-699): planar-scan compositing.  Canvas = bounding box of all H2refined corner
    maps with MATLAB-rounded size (:547-575), computed here in f64; then every image is warped to it and blended
    'none' (winner-take-all by weight, first maximum) / 'linear' / 'multiband'; void pixels painted; uint8.
    The compositing runs in one device-resident call for uint8 images of 1 or 3 channels: planar_composite (one
    canvas-sized layer per image) for up to 64 images that fit, planar_composite_compact (footprint-sized layers) for more
    images, for sets whose dense request exceeds opts['planarDenseLimitBytes'] (default: the free device memory) and with
    opts['planarCompositor'] = 'compact';
    other inputs, opts['planarCompositor'] = 'host' and APS_PLANAR_HOST=1 take the host-orchestrated path
    (_planar_host: every image warped to the FULL canvas by imageWarp, numpy in between), whose bytes the device path
    reproduces.
    Gains: pass `gains` (N x 3), or set opts['gainCompensation'] to have gainCompensationH run on the warped images
    (:584-591: overlap statistics on the device, solve on the host); otherwise ones.
    rgbAnnotation (:653-679): with opts['showPanoramaImgsNums'] and opts['showCropBoundingBox'] both true, the panorama with
    every image's outline (planar_boxes) and number drawn on the device (annotate_panorama; opts['annotationColors'] N x 3
    overrides vivid_palette), for all three compositors; otherwise None.  The panorama itself is the same bytes either way."""
    from .imageProcessing import imref2dScratch, outputLimitsScratch

    o = {"blending": "multiband", "pyrLevels": 3, "pyrSigma": 1.0, "canvasColor": "black",
         "sigmaN": 10.0, "sigmag": 0.1}  # (renderPanorama.m:56-58: the defaults opts carries into gainCompensationH)
    o.update(opts or {})
    multiband_weights(o)  # (an unknown value is refused before any work)
    images = [im if _capi.is_torch(im) else np.asarray(im) for im in images[:numImages]]
    tforms = [np.asarray(cam["H2refined"], np.float64) for cam in cameras[:numImages]]
    lims = [outputLimitsScratch(T, (1, int(im.shape[1])), (1, int(im.shape[0])))
            for T, im in zip(tforms, images)]
    xMin, xMax = min(l[0][0] for l in lims), max(l[0][1] for l in lims)
    yMin, yMax = min(l[1][0] for l in lims), max(l[1][1] for l in lims)
    width, height = int(_matlab_round(xMax - xMin)), int(_matlab_round(yMax - yMin))
    if width < 1 or height < 1:
        raise ValueError("degenerate planar canvas")
    view = imref2dScratch((height, width), (xMin, xMax), (yMin, yMax))
    route = _planar_device_covers(images, o)
    if route:
        if str(o["blending"]).lower() not in _BLEND:
            raise ValueError("Wrong blening mode.")
        pano = _planar_device_composite(route, images, tforms, view, o, gains, device_out)
        gray = images[0].ndim == 2 or int(images[0].shape[2]) == 1
        one = gains is None and not o.get("gainCompensation") or gains is not None and all(np.size(g) == 1 for g in gains)
        if gray and one and str(o["blending"]).lower() == "none":
            pano = pano[:, :, :1]  # (the host path's 'none' keeps the single channel of its input; the blends return three)
        return pano, _planar_annotation(pano, images, tforms, view, o)
    if any(_capi.is_torch(im) for im in images):
        images = [im.cpu().numpy() if _capi.is_torch(im) else im for im in images]
    pano = _planar_host(images, tforms, view, o, gains)
    if device_out:
        import torch

        pano = torch.from_numpy(pano).cuda()
    return pano, _planar_annotation(pano, images, tforms, view, o)


def _planar_annotation(pano, images, tforms, view, o):
    """renderPanorama.m:653-679: the annotated planar-scan panorama (None unless both flags are set); resident when pano is."""
    if not _wants_annotation(o):
        return None
    polys, centers = planar_boxes([im.shape for im in images], tforms, view)
    ann, _ = annotate_panorama(pano, polys, centers, o.get("annotationColors"), int(o.get("annotationLineWidth", 2)))
    return ann


def _planar_host(images, tforms, view, o, gains=None):
    """The host-orchestrated compositing of pureNonRotationalPanoramas: 2N whole-canvas imageWarp calls, gains, the blend
    operators and the uint8 tail in numpy.  The yardstick of planar_composite and the path of inputs it does not cover."""
    from .blending import linearBlending, multiBandBlending

    Iw, Ww, _, _, _ = pureNonRotationalImagesToCanvas(images, tforms, view, warpWeights(images), o)
    if gains is None and o.get("gainCompensation"):
        # renderPanorama.m:584-591: gains from the warped canvases (statistics on the device, N x N solve on the host).  As
        # in the ray renderer below only when the caller asks for it explicitly; otherwise ones (or the caller's own).
        from .gainCompensation import gainCompensationH

        gains = gainCompensationH(Iw, Ww, o)
    if gains is not None:
        Iw = [I * np.asarray(g, np.float32).reshape(1, 1, -1) for I, g in zip(Iw, gains)]
    mode = str(o["blending"]).lower()
    if mode == "none":
        Wst = np.stack(Ww, 2)
        idx = np.argmax(Wst, 2)  # first maximum, like MATLAB's max
        pano = np.take_along_axis(np.stack(Iw, 3), idx[:, :, None, None], 3)[..., 0]
    elif mode == "linear":
        pano = linearBlending(Iw, Ww)
    elif mode == "multiband":
        pano = multiBandBlending(Iw, Ww, int(o["pyrLevels"]), True, float(o["pyrSigma"]), Weights=multiband_weights(o))
    else:
        raise ValueError("Wrong blening mode.")
    pano = np.array(pano, np.float32, copy=True)
    void = ~(np.stack(Ww, 2) > 0).any(2)
    pano[void] = 1.0 if str(o["canvasColor"]).lower() == "white" else 0.0
    v = 255.0 * pano.astype(np.float64)
    out = np.sign(v) * np.floor(np.abs(v) + 0.5)  # MATLAB round
    return np.clip(out, 0, 255).astype(np.uint8)


def renderPanorama(input, images, imgSize, cameras, mode, refIdx, opts=None, gains=None,
                   return_covered=False, device_out=False, tile_subset=None, geo=None, zero_rest=True):
    """[panorama, rgbAnnotation] = renderPanorama(input, images, imgSize, cameras, mode, refIdx, opts)
    (renderPanorama.m:1-500).  refIdx is 0-based here.  Differences that are deliberate:
      * opts['tile'] must be explicit; the reference derives it from free GPU/CPU memory (:269-298),
        which makes its multiband output machine dependent.  Default here: [2048 2048] clamped to the
        canvas — the value the reference's auto-tiler reaches whenever memory is plentiful.
      * gains: pass `gains` (N x 3), or set opts['gainCompensation'] explicitly to have gainCompensationRKf run
        (statistics on the device, solve on the host); otherwise ones.
      * rgbAnnotation (:438-477) is produced when opts carries showPanoramaImgsNums and showCropBoundingBox, both true: the
        (cropped) panorama with every image's warped outline (warped_boxes, shifted by the crop origin as :434-455) and its
        number, drawn on the device by annotate_panorama under this project's own raster rule ("Annotation
        contract"; insertShape / insertText are closed).  Colours: opts['annotationColors'] (N x 3) or vivid_palette(N) -
        brightColors draws from rand.  Resident when device_out is set; None otherwise and for a tile shard.  The panorama
        itself is the same bytes with and without the flags."""
    if cameras and (cameras[0].get("noRotation", 0) == 1 or input.get("forcePlanarScan", False)):
        # renderPanorama.m:78-90: planar scans bypass the tiled ray renderer
        pano, ann = pureNonRotationalPanoramas(images, cameras, len(images), opts or {}, gains, device_out)
        return (pano, ann, None, None) if return_covered else (pano, ann)
    o = default_opts(opts, cameras, refIdx)
    multiband_weights(o)  # (an unknown value is refused before any library call)
    imgSize = [tuple(int(v) for v in s) for s in imgSize]
    if geo is None:  # (a caller that has sized the canvas already - the sharded driver - passes it in)
        geo = canvas_geometry(cameras, imgSize, mode, refIdx, o)
    o["tile"] = effective_tile(o, geo)
    if gains is None and opts and opts.get("gainCompensation"):
        # renderPanorama.m:303-330: overlap statistics on the device, N x N solve on the host.  Only when the
        # caller asks for it explicitly; otherwise gains are ones (or the caller's own).
        from .gainCompensation import gainCompensationRKf

        gains = gainCompensationRKf(images, cameras, mode, refIdx, opts, geo)
    arr, keep = make_image_structs(images, cameras, gains)
    cv = make_canvas_struct(geo)
    ro = make_render_opts(o)
    H, W = geo["H"], geo["W"]
    if device_out:
        import torch

        pano = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        cov = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    else:
        pano = np.zeros((H, W, 3), np.uint8)
        cov = np.zeros((H, W), np.uint8)
    # ONE call renders all tiles on the calling thread (render_batch.hip: multiband level-major, 'linear' / 'none' as one fused
    # launch; APS_RENDER_LEGACY=1: the per-tile path the tests compare it with, tile after tile inside the same call)
    if tile_subset is None:
        check(lib.aps_render(arr, len(images), C.byref(cv), C.byref(ro), _capi.APS_IMG_U8_HWC, ptr(pano), ptr(cov)))
    elif tile_subset[0] == "range":
        # ("range", begin, end): the contiguous tiles begin <= t < end - a rank's band of the canvas (parallel.tile_ranges)
        import torch

        # zero_rest=False (a resident shard whose tiles alone are sent on: parallel.gather_tiles_to_root): the ~1 GB fill of
        # the canvas outside the run is skipped - those pixels are never read
        if device_out and zero_rest:
            pano.zero_()
            cov.zero_()
            torch.cuda.current_stream().synchronize()  # torch's fills must land before the library's stream paints tiles
        check(lib.aps_render_tile_range(arr, len(images), C.byref(cv), C.byref(ro), _capi.APS_IMG_U8_HWC,
                                        int(tile_subset[1]), int(tile_subset[2]), ptr(pano), ptr(cov)))
    else:  # (first, step): only tiles t with t % step == first — an interleaved shard of the tile loop
        first, step = int(tile_subset[0]), int(tile_subset[1])
        if device_out:
            import torch

            pano.zero_()
            cov.zero_()
            torch.cuda.current_stream().synchronize()  # torch's fills must land before the library's stream paints tiles
        check(lib.aps_render_tiles(arr, len(images), C.byref(cv), C.byref(ro), _capi.APS_IMG_U8_HWC,
                                   first, step, ptr(pano), ptr(cov)))
    del keep
    rect = (1, H, 1, W)
    if o["cropBorder"] and tile_subset is None:  # renderPanorama.m:430-432 (a tile shard is cropped after it is combined)
        if device_out:
            check(lib.aps_synchronize())  # the panorama was painted on the library's stream of this thread
        pano, rect, _ = cropNonzeroBbox(pano, o["canvasColor"])
    ann = None
    if _wants_annotation(o) and tile_subset is None:
        polys, centers = warped_boxes(cameras, imgSize, geo)
        shift = np.array([rect[2] - 1, rect[0] - 1], np.float64)  # dx = c1 - 1, dy = r1 - 1 (:434-455)
        ann, _ = annotate_panorama(pano, polys - shift, centers - shift, o.get("annotationColors"),
                                   int(o.get("annotationLineWidth", 2)))
    if return_covered:
        return pano, ann, cov, geo
    return pano, ann


def warp_tile(image, camera, geo, r0, c0, ht, wt, anglePower=2.0, gain=(1.0, 1.0, 1.0)):
    """sampleOneTile for one tile/image (renderPanorama.m:1063-1146): returns S, M, Wang, Wf."""
    arr, keep = make_image_structs([image], [camera], [gain])
    cv = make_canvas_struct(geo)
    S = np.zeros((ht, wt, 3), np.float32)
    M = np.zeros((ht, wt), np.uint8)
    Wa = np.zeros((ht, wt), np.float32)
    Wf = np.zeros((ht, wt), np.float32)
    check(lib.aps_warp_tile(arr, C.byref(cv), r0, c0, ht, wt, float(anglePower), ptr(S), ptr(M), ptr(Wa), ptr(Wf)))
    return S, M.astype(bool), Wa, Wf


_DISPLAY_PROJECTIONS = ("planar", "cylindrical", "spherical", "equirectangular", "stereographic", "miller", "fisheye", "panini")


def displayPanorama(input, finalPanoramaTforms, finalrefIdxs, imagesAll, imageSizesAll, panoIndices, device_out=False):
    """panoStore = displayPanorama(input, finalPanoramaTforms, finalrefIdxs, imagesAll, imageSizesAll, panoIndices)
    (displayPanorama.m:58-137): every component rendered in every projection of input['panorama2DisplaynSave'] (one
    string or a list of them) with the opts of :100-111.  finalPanoramaTforms: per component its list of camera dicts (an
    empty one is skipped, :90); finalrefIdxs and panoIndices are 1-based like the reference's (the messages name 1..N).
    Returns the list of dicts cropNsavePanorama consumes: one per component, projection -> [panorama, annotated or None]
    (the reference's 1 x C struct array of 1 x 2 cells); the arrays are resident torch tensors with device_out.  Same
    length and index checks, same messages.  No figures are drawn (input.displayPanoramas is not read); input['tile'], when
    present, is passed on as opts['tile'] (renderPanorama's explicit tile)."""
    nC = len(finalPanoramaTforms)
    if np.size(finalrefIdxs) != nC:
        raise ValueError(f"displayPanorama:InvalidRefIdxsLength: finalrefIdxs must have one entry per component ({nC}).")
    if len(panoIndices) != nC:
        raise ValueError(f"displayPanorama:InvalidPanoIndicesLength: panoIndices must have one cell per component ({nC}).")
    refs = np.asarray(finalrefIdxs).reshape(-1)
    nImgs = len(imagesAll)
    idx_lists = []
    for ii in range(nC):
        raw = panoIndices[ii]
        try:
            idxs = np.asarray(raw)
            numeric = idxs.dtype.kind in "iuf" and idxs.ndim <= 2 and (idxs.ndim < 2 or 1 in idxs.shape or idxs.size == 0)
        except Exception:  # noqa: BLE001 - a ragged or non-array cell is not a numeric vector
            idxs, numeric = np.zeros(0), False
        if not numeric:
            if idxs.size == 0:
                idx_lists.append(np.zeros(0, np.int64))
                continue
            raise ValueError(f"displayPanorama:InvalidPanoIndexType: panoIndices{{{ii + 1}}} must be a numeric vector of image indices.")
        idxs = idxs.reshape(-1)
        if idxs.size and (idxs.min() < 1 or idxs.max() > nImgs):
            raise ValueError(f"displayPanorama:ImageIndexOutOfBounds: panoIndices{{{ii + 1}}} has indices outside 1..{nImgs}.")
        idx_lists.append(idxs.astype(np.int64))
    projections = input["panorama2DisplaynSave"]
    projections = [projections] if isinstance(projections, str) else [str(p) for p in projections]
    panoStore = [dict() for _ in range(nC)]
    for ii in range(nC):
        cameras = finalPanoramaTforms[ii]
        if cameras is None or len(cameras) == 0:
            continue
        refIdx = int(refs[ii]) - 1
        images = [imagesAll[k - 1] for k in idx_lists[ii]]
        imageSizes = [tuple(int(v) for v in np.asarray(imageSizesAll[k - 1]).reshape(-1)) for k in idx_lists[ii]]
        opts = {"fPan": float(np.asarray(cameras[refIdx]["K"])[0, 0]), "resScale": 1.0, "anglePower": 2, "cropBorder": True,
                "canvasColor": input["canvasColor"], "gainCompensation": input["gainCompensation"], "sigmaN": input["sigmaN"],
                "sigmag": input["sigmag"], "pyrLevels": input["bands"], "blending": input["blending"],
                "pyrSigma": input["MBBsigma"], "showPanoramaImgsNums": input["showPanoramaImgsNums"],
                "showCropBoundingBox": input["showCropBoundingBox"], "useMATLABImwarp": input.get("useMATLABImwarp", 0)}
        if input.get("tile") is not None:
            opts["tile"] = input["tile"]
        if input.get("multibandWeights") is not None:
            opts["multibandWeights"] = input["multibandWeights"]
        for projection in projections:
            panorama, annoRGB = renderPanorama(input, images, imageSizes, cameras, projection, refIdx, opts, device_out=device_out)
            if projection in _DISPLAY_PROJECTIONS:  # :126-136
                panoStore[ii][projection] = [panorama, annoRGB]
    return panoStore
