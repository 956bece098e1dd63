"""A numpy restatement of the projection contract ("Projection contract") for the three canvas modes the C oracle
does not know: 'miller', 'fisheye', 'panini'.

  * inverse(mode, geo, xp, yp): canvas pixel (0-based) -> unit ray in the world frame, in float32 and in the operation order
    the device uses (canvas_ray in csrc/render_dev.h);
  * forward(mode, geo, rays): world ray -> canvas coordinates (a, b) and the 0-based pixel, in float64, written from the
    projections' textbook forward formulas and NOT by inverting `inverse`;
  * warp_tile(...): `inverse` followed by a restatement of project + sample_one (bilinear colour, tent weight, angle weight),
    which yields S, M, Wang, Wf of a tile like renderPanorama.warp_tile and oracle.warp_tile do.

The sampling half is mode independent; tests/test_projections.py pins it once against oracle.warp_tile in 'spherical' mode
(this module knows the four older modes for that purpose).  numpy has no fused multiply-add: where the device writes fmaf the
mirror rounds an exact float64 evaluation to float32, which differs from the fused result by double rounding only (one ulp,
rarely), far inside the tolerance of anything behind the ray generator."""
import numpy as np

F32 = np.float32
PI_F32 = F32(3.14159265)  # the literal of the device code: rounds to the float32 nearest to pi
MODES = ("miller", "fisheye", "panini")
MILLER_POLE = 1.25 * np.arcsinh(np.tan(0.8 * (np.pi / 2)))  # 2.3034...


def _canvas_f32(geo):
    return F32(geo["fPan"]), F32(geo["o0"]), F32(geo["o1"]), np.asarray(geo["Rref"], np.float64).astype(F32)


def ab_of_pixel(geo, xp, yp):
    """a = o0 + xp / f, b = o1 + yp / f in float32 (xp, yp: 0-based canvas pixel, any broadcastable shapes)."""
    f, o0, o1, _ = _canvas_f32(geo)
    return o0 + np.asarray(xp, F32) / f, o1 + np.asarray(yp, F32) / f


def _from_ref(Rref, rx, ry, rz):
    """world = Rref' * r, each component as (R0 rx + R1 ry) + R2 rz."""
    return tuple((Rref[0, c] * rx + Rref[1, c] * ry) + Rref[2, c] * rz for c in range(3))


def inverse(mode, geo, xp, yp):
    """Unit world rays [..., 3] (float32) of the canvas pixels; the zero vector where a fisheye pixel lies beyond r = pi."""
    _, _, _, Rref = _canvas_f32(geo)
    a, b = ab_of_pixel(geo, xp, yp)
    a, b = np.broadcast_arrays(a, b)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        if mode in ("spherical", "equirectangular", "miller"):
            ph = F32(1.25) * np.arctan(np.sinh(F32(0.8) * b)) if mode == "miller" else b
            cp, sp = np.cos(ph), np.sin(ph)
            x, y, z = cp * np.sin(a), sp, cp * np.cos(a)
        elif mode == "cylindrical":
            x, y, z = np.sin(a), b, np.cos(a)
        else:
            if mode in ("planar", "perspective"):
                rx, ry, rz = a, b, np.ones_like(a)
            elif mode == "stereographic":
                r2 = a * a + b * b
                den = one + r2
                rx, ry, rz = F32(2.0) * a / den, F32(2.0) * b / den, (one - r2) / den
            elif mode == "fisheye":
                r = np.sqrt(a * a + b * b)
                s = np.where(r > F32(1e-6), np.sin(r) / np.where(r > F32(1e-6), r, one), one).astype(F32)
                seen = ~(r > PI_F32)
                zero = np.zeros_like(a)
                rx, ry, rz = np.where(seen, s * a, zero), np.where(seen, s * b, zero), np.where(seen, np.cos(r), zero)
            elif mode == "panini":
                rx, ry, rz = a, b, one - F32(0.25) * a * a
            else:
                raise ValueError(mode)
            x, y, z = _from_ref(Rref, rx, ry, rz)
        n = np.sqrt((x * x + y * y) + z * z)
        n = np.where(n > F32(1e-8), n, F32(1e-8)).astype(F32)
        d = np.stack([x / n, y / n, z / n], axis=-1)
    assert d.dtype == F32
    return d


def forward(mode, geo, rays):
    """World rays [..., 3] (any length) -> (a, b, xp, yp) in float64: canvas coordinates and the 0-based pixel position that
    looks along the ray, xp = (a - o0) * f."""
    d = np.asarray(rays, np.float64)
    d = d / np.sqrt((d ** 2).sum(-1, keepdims=True))
    f, o0, o1 = float(geo["fPan"]), float(geo["o0"]), float(geo["o1"])
    if mode == "miller":
        lon = np.arctan2(d[..., 0], d[..., 2])
        lat = np.arcsin(np.clip(d[..., 1], -1.0, 1.0))
        a, b = lon, 1.25 * np.log(np.tan(np.pi / 4 + 0.4 * lat))  # Miller's own form: (5/4) ln tan(pi/4 + 2 lat / 5)
    else:
        r = d @ np.asarray(geo["Rref"], np.float64).T  # reference frame: Rref * d
        if mode == "fisheye":
            theta = np.arctan2(np.hypot(r[..., 0], r[..., 1]), r[..., 2])  # angle from the axis
            psi = np.arctan2(r[..., 1], r[..., 0])
            a, b = theta * np.cos(psi), theta * np.sin(psi)
        elif mode == "panini":
            lon = np.arctan2(r[..., 0], r[..., 2])
            tan_lat = r[..., 1] / np.hypot(r[..., 0], r[..., 2])
            s = 2.0 / (1.0 + np.cos(lon))  # d = 1: S = (d + 1) / (d + cos lon)
            a, b = s * np.sin(lon), s * tan_lat
        else:
            raise ValueError(mode)
    return a, b, (a - o0) * f, (b - o1) * f


def random_directions(mode, n, rng):
    """n unit rays inside the domain where the mode's map is one-to-one and well conditioned (world frame, Rref = I)."""
    d = rng.normal(size=(4 * n + 64, 3))
    d /= np.sqrt((d ** 2).sum(1, keepdims=True))
    if mode == "miller":
        keep = np.abs(d[:, 1]) < np.sin(1.5)  # away from the poles, where the azimuth is undefined
    elif mode == "fisheye":
        keep = d[:, 2] > np.cos(3.0)  # theta < 3 rad: short of the antipode, where the whole rim is one direction
    else:
        keep = np.hypot(d[:, 0], d[:, 2]) + d[:, 2] > 0.05  # away from the half plane behind the axis
    d = d[keep][:n]
    assert len(d) == n
    return d


def inverse_f64(mode, a, b):
    """The three inverse maps in float64 with Rref = I (for the forward-after-inverse identity): unnormalised rays."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if mode == "miller":
        ph = 1.25 * np.arctan(np.sinh(0.8 * b))
        return np.stack([np.cos(ph) * np.sin(a), np.sin(ph), np.cos(ph) * np.cos(a)], -1)
    if mode == "fisheye":
        r = np.sqrt(a * a + b * b)
        s = np.where(r > 1e-6, np.sin(r) / np.where(r > 1e-6, r, 1.0), 1.0)
        return np.stack([s * a, s * b, np.cos(r)], -1)
    if mode == "panini":
        return np.stack([a, b, 1.0 - 0.25 * a * a], -1)
    raise ValueError(mode)


def tent(n):
    """warpWeights' 1-D tent (renderPanorama.m:1282-1312): linspace(0, 1, ceil(n / 2)) up, linspace(1, 0, n - floor(n / 2)) down
    from floor(n / 2); the second assignment wins where they meet."""
    t = np.zeros(n, F32)
    a = (n + 1) // 2
    t[:a] = np.linspace(0, 1, a).astype(F32) if a > 1 else 1.0
    nb = n - n // 2
    t[n // 2:] = np.linspace(1, 0, nb).astype(F32) if nb > 1 else 0.0
    return t


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def sample(image, camera, d, angle_power=2.0, gain=(1.0, 1.0, 1.0)):
    """project + sample_one of csrc/render_dev.h on rays d [..., 3] (float32): S [..., 3], M, Wang, Wf."""
    img = np.asarray(image)
    if img.ndim == 2:
        img = np.repeat(img[..., None], 3, 2)
    h, w = img.shape[:2]
    K = np.asarray(camera["K"], np.float64)
    R = np.asarray(camera["R"], np.float64).astype(F32)
    fx, fy, cx, cy = F32(K[0, 0]), F32(K[1, 1]), F32(K[0, 2]), F32(K[1, 2])
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    cam = [_fma(d2, R[c, 2], _fma(d1, R[c, 1], d0 * R[c, 0])) for c in range(3)]
    eps = F32(1e-6)
    front = cam[2] > eps
    cz = np.where(front, cam[2], eps).astype(F32)
    with np.errstate(all="ignore"):
        u = fx * (cam[0] / cz) + cx
        v = fy * (cam[1] / cz) + cy
        wa = np.where(cam[2] > 0, cam[2], F32(0)).astype(F32)
        if angle_power == 2.0:
            wa = wa * wa
        elif angle_power != 1.0:
            wa = np.power(wa, F32(angle_power))
    wa = np.where(front, wa, F32(0)).astype(F32)
    bad = ~np.isfinite(u) | ~np.isfinite(v)
    u = np.where(bad, F32(1), u).astype(F32)
    v = np.where(bad, F32(1), v).astype(F32)
    M = (u >= 1) & (u <= F32(w)) & (v >= 1) & (v <= F32(h)) & (wa > 0)
    x0 = np.clip(np.floor(u).astype(np.int64), 1, max(w - 1, 1))
    y0 = np.clip(np.floor(v).astype(np.int64), 1, max(h - 1, 1))
    x1, y1 = np.minimum(x0 + 1, w), np.minimum(y0 + 1, h)
    s, t = (u - x0.astype(F32)).astype(F32), (v - y0.astype(F32)).astype(F32)
    one = F32(1)

    def bilinear(p00, p10, p01, p11):
        top = (one - s) * p00 + s * p10
        bot = (one - s) * p01 + s * p11
        return top * (one - t) + bot * t

    S = np.zeros(d.shape[:-1] + (3,), F32)
    for c in range(3):
        g = F32(gain[c])
        tap = lambda yy, xx: (img[yy - 1, xx - 1, c].astype(F32) / F32(255.0)) * g  # noqa: E731
        S[..., c] = bilinear(tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1))
    wx, wy = tent(w), tent(h)
    Wf = bilinear(wy[y0 - 1] * wx[x0 - 1], wy[y0 - 1] * wx[x1 - 1], wy[y1 - 1] * wx[x0 - 1], wy[y1 - 1] * wx[x1 - 1])
    S = np.where(M[..., None], S, F32(0)).astype(F32)
    return S, M, np.where(M, wa, F32(0)).astype(F32), np.where(M, Wf, F32(0)).astype(F32)


def warp_tile(image, camera, geo, r0, c0, ht, wt, angle_power=2.0, gain=(1.0, 1.0, 1.0)):
    """S [ht, wt, 3], M [ht, wt] bool, Wang, Wf [ht, wt] of the tile whose top-left canvas pixel is (r0, c0), 0-based."""
    yp = (r0 + np.arange(ht))[:, None]
    xp = (c0 + np.arange(wt))[None, :]
    return sample(image, camera, inverse(geo["mode"], geo, xp, yp), angle_power, gain)
