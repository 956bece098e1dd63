"""NumPy restatement of the SURF contract (DESIGN.md "SURF contract") -- test infrastructure, not a test.

Written from the contract, not from the kernel: integers where the contract has integers (gray plane, integral image,
every box and Haar sum, in int64 here), ``np.float32`` arrays with the contract's written operation and summation order
where it has f32 (one rounding per written operation), and the same f64 -> f32 tables (``math.exp`` / ``math.cos`` /
``math.sin``, the C library's functions).  ``extract`` returns what ``aps_surf_extract`` returns.
"""
import math

import numpy as np

f32 = np.float32
ORI = [(di, dj) for di in range(-5, 6) for dj in range(-5, 6) if di * di + dj * dj < 36]
assert len(ORI) == 109
ORI_DI = np.array([p[0] for p in ORI], np.int64)
ORI_DJ = np.array([p[1] for p in ORI], np.int64)
ORI_G = np.array([math.exp(-(di * di + dj * dj) / 8.0) for di, dj in ORI], np.float64).astype(f32)


def _windows():
    c, s = np.zeros(64, f32), np.zeros(64, f32)
    for w in range(64):
        q, r = divmod(w, 16)
        cw, sw = f32(math.cos(2.0 * math.pi * r / 64.0)), f32(math.sin(2.0 * math.pi * r / 64.0))
        for _ in range(q):  # one exact quarter turn
            cw, sw = -sw, cw
        c[w], s[w] = cw, sw
    return c, s


WIN_C, WIN_S = _windows()
DESC_G = np.array([math.exp(-(((c - 10) + 0.5) ** 2 + ((r - 10) + 0.5) ** 2) / (2.0 * 3.3 * 3.3))
                   for r in range(20) for c in range(20)], np.float64).astype(f32)
TAN30 = f32(0.57735026)


def gray_plane(img):
    """rgb2gray's integer plane (0..255); a gray input is passed through."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.astype(np.int64)
    d = 0.298936021293775 * img[..., 0].astype(np.float64) + 0.587043074451121 * img[..., 1].astype(np.float64)
    d = d + 0.114020904255103 * img[..., 2].astype(np.float64)
    return np.floor(d + 0.5).astype(np.int64)


def integral(gray):
    """(h+1) x (w+1), I[y+1][x+1] = sum of gray[0..y][0..x]; exact integers."""
    h, w = gray.shape
    if h * w * 255 >= 2 ** 32:
        raise ValueError("image exceeds the 32-bit integral image")
    I = np.zeros((h + 1, w + 1), np.int64)
    I[1:, 1:] = np.cumsum(np.cumsum(gray.astype(np.int64), 0), 1)
    return I


def box(I, r0, r1, c0, c1):
    """Sum over rows r0..r1, columns c0..c1 (inclusive); index arrays broadcast."""
    return I[r1 + 1, c1 + 1] - I[r0, c1 + 1] - I[r1 + 1, c0] + I[r0, c0]


def filter_size(o, lv):
    return 3 * ((1 << o) * (lv + 1) + 1)


def response(I, y, x, S):
    """(det, trace) f32 of the box Hessian at pixels (y, x) (int arrays) for filter side S; 0 where the filter leaves the image."""
    h, w = I.shape[0] - 1, I.shape[1] - 1
    y, x = np.broadcast_arrays(np.asarray(y, np.int64), np.asarray(x, np.int64))
    b, l = (S - 1) // 2, S // 3
    hl = (l - 1) // 2
    fit = (y - b >= 0) & (y + b <= h - 1) & (x - b >= 0) & (x + b <= w - 1)
    yy, xx = np.where(fit, y, b), np.where(fit, x, b)
    Dxx = box(I, yy - (l - 1), yy + (l - 1), xx - b, xx + b) - 3 * box(I, yy - (l - 1), yy + (l - 1), xx - hl, xx + hl)
    Dyy = box(I, yy - b, yy + b, xx - (l - 1), xx + (l - 1)) - 3 * box(I, yy - hl, yy + hl, xx - (l - 1), xx + (l - 1))
    Dxy = (box(I, yy - l, yy - 1, xx - l, xx - 1) + box(I, yy + 1, yy + l, xx + 1, xx + l)
           - box(I, yy - l, yy - 1, xx + 1, xx + l) - box(I, yy + 1, yy + l, xx - l, xx - 1))
    inv = f32(1.0 / ((2.0 * l - 1.0) * l))  # one lobe of Dxx / Dyy
    inv_xy = f32(1.0 / (float(l) * float(l)))  # one box of Dxy
    dxx, dyy, dxy = Dxx.astype(f32) * inv, Dyy.astype(f32) * inv, Dxy.astype(f32) * inv_xy
    t1, t2 = dxx * dyy, dxy * dxy
    t3 = f32(0.81) * t2
    det = t1 - t3
    tr = dxx + dyy
    z = f32(0)
    return np.where(fit, det, z).astype(f32), np.where(fit, tr, z).astype(f32)


def refine(a):
    """a: [n, 3, 3, 3] f32 (level, row, col).  Returns (ok, ox, oy, os)."""
    a = np.asarray(a, f32)
    A = lambda dz, dy, dx: a[:, dz + 1, dy + 1, dx + 1]  # noqa: E731
    h_, q_ = f32(0.5), f32(0.25)
    with np.errstate(all="ignore"):
        v2 = A(0, 0, 0) + A(0, 0, 0)
        gx, gy, gs = (A(0, 0, 1) - A(0, 0, -1)) * h_, (A(0, 1, 0) - A(0, -1, 0)) * h_, (A(1, 0, 0) - A(-1, 0, 0)) * h_
        hxx, hyy, hss = (A(0, 0, 1) + A(0, 0, -1)) - v2, (A(0, 1, 0) + A(0, -1, 0)) - v2, (A(1, 0, 0) + A(-1, 0, 0)) - v2
        hxy = ((A(0, 1, 1) - A(0, 1, -1)) - (A(0, -1, 1) - A(0, -1, -1))) * q_
        hxs = ((A(1, 0, 1) - A(1, 0, -1)) - (A(-1, 0, 1) - A(-1, 0, -1))) * q_
        hys = ((A(1, 1, 0) - A(1, -1, 0)) - (A(-1, 1, 0) - A(-1, -1, 0))) * q_
        c00, c01, c02 = hyy * hss - hys * hys, hxs * hys - hxy * hss, hxy * hys - hxs * hyy
        c11, c12, c22 = hxx * hss - hxs * hxs, hxy * hxs - hxx * hys, hxx * hyy - hxy * hxy
        D = (hxx * c00 + hxy * c01) + hxs * c02
        ox = -((c00 * gx + c01 * gy) + c02 * gs) / D
        oy = -((c01 * gx + c11 * gy) + c12 * gs) / D
        os = -((c02 * gx + c12 * gy) + c22 * gs) / D
        ok = (D != 0) & (np.abs(ox) <= 1) & (np.abs(oy) <= 1) & (np.abs(os) <= 1)
    return ok, ox, oy, os


def plan(h, w, n_octaves=8, n_levels=4):
    """The octaves (1-based numbers) whose largest filter fits the image."""
    out = []
    for o in range(1, n_octaves + 1):
        if filter_size(o, n_levels - 1) > min(h, w):
            break
        out.append(o)
    return out


def level_responses(I, o, lv):
    """Response plane of octave o, level lv on the octave's sample grid."""
    h, w = I.shape[0] - 1, I.shape[1] - 1
    step = 1 << (o - 1)
    ys, xs = np.arange(0, h, step), np.arange(0, w, step)
    return response(I, ys[:, None], xs[None, :], filter_size(o, lv))[0]


def detect(I, thr=1000.0, n_octaves=8, n_levels=4):
    """Keypoints in canonical order (octave, level, row, col): dict of arrays."""
    h, w = I.shape[0] - 1, I.shape[1] - 1
    thr = f32(thr)
    K = {k: [] for k in ("o", "m", "i", "j", "ox", "oy", "os", "metric", "trace")}
    for o in plan(h, w, n_octaves, n_levels):
        step = 1 << (o - 1)
        R = np.stack([level_responses(I, o, lv) for lv in range(n_levels)])
        gh, gw = R.shape[1:]
        for m in range(1, n_levels - 1):
            reach = step + (filter_size(o, m + 1) - 1) // 2
            ii, jj = np.mgrid[0:gh, 0:gw]
            y, x = ii * step, jj * step
            cand = (R[m] > thr) & (y - reach >= 0) & (y + reach <= h - 1) & (x - reach >= 0) & (x + reach <= w - 1)
            ci, cj = np.nonzero(cand)  # row-major: ascending (row, col)
            if ci.size == 0:
                continue
            nb = np.stack([np.stack([np.stack([R[m + dz, ci + dy, cj + dx] for dx in (-1, 0, 1)], -1) for dy in (-1, 0, 1)], -2)
                           for dz in (-1, 0, 1)], -3)  # [n, 3, 3, 3]
            v = nb[:, 1, 1, 1]
            others = nb.reshape(-1, 27)[:, [k for k in range(27) if k != 13]]
            mx = (v[:, None] > others).all(1)
            ok, ox, oy, os = refine(nb)
            keep = mx & ok
            ci, cj = ci[keep], cj[keep]
            tr = response(I, ci * step, cj * step, filter_size(o, m))[1]
            for k, val in (("o", np.full(ci.size, o)), ("m", np.full(ci.size, m)), ("i", ci), ("j", cj), ("ox", ox[keep]),
                           ("oy", oy[keep]), ("os", os[keep]), ("metric", v[keep]), ("trace", tr)):
                K[k].append(val)
    out = {}
    for k, lst in K.items():
        dt = np.int64 if k in ("o", "m", "i", "j") else f32
        out[k] = np.concatenate(lst).astype(dt) if lst else np.zeros(0, dt)
    o, m = out["o"], out["m"]
    step = (1 << (o - 1)).astype(f32)
    out["px"] = (out["j"].astype(f32) + out["ox"]) * step
    out["py"] = (out["i"].astype(f32) + out["oy"]) * step
    S = (3 * ((1 << o) * (m + 1) + 1)).astype(f32)
    dS = (3 * (1 << o)).astype(f32)
    sizef = S + out["os"] * dS
    out["scale"] = (f32(1.2) * sizef) / f32(9.0)
    return out


def _round(v):
    return np.floor(v + f32(0.5)).astype(np.int64)


def haar(I, iy, ix, hs):
    """Integer Haar responses (dx, dy) with half side hs (arrays broadcast); zeros where the window leaves the image."""
    h, w = I.shape[0] - 1, I.shape[1] - 1
    iy, ix, hs = np.broadcast_arrays(iy, ix, hs)
    ok = (iy - hs >= 0) & (iy + hs <= h - 1) & (ix - hs >= 0) & (ix + hs <= w - 1)
    y, x, s = np.where(ok, iy, 1), np.where(ok, ix, 1), np.where(ok, hs, 1)
    dx = box(I, y - s, y + s, x + 1, x + s) - box(I, y - s, y + s, x - s, x - 1)
    dy = box(I, y + 1, y + s, x - s, x + s) - box(I, y - s, y - 1, x - s, x + s)
    return np.where(ok, dx, 0), np.where(ok, dy, 0)


def orientation(I, px, py, s):
    """(c, sn, angle_deg) per keypoint."""
    n = px.size
    hs = np.maximum(1, _round(f32(2.0) * s))
    X = px[:, None] + ORI_DJ.astype(f32)[None, :] * s[:, None]
    Y = py[:, None] + ORI_DI.astype(f32)[None, :] * s[:, None]
    dx, dy = haar(I, _round(Y), _round(X), hs[:, None])
    vx, vy = ORI_G[None, :] * dx.astype(f32), ORI_G[None, :] * dy.astype(f32)
    sx, sy = np.zeros((n, 64), f32), np.zeros((n, 64), f32)
    z = f32(0)
    for k in range(109):  # members are summed in sample order
        ax, ay = vx[:, k, None], vy[:, k, None]
        dot = ax * WIN_C[None, :] + ay * WIN_S[None, :]
        crs = ax * WIN_S[None, :] - ay * WIN_C[None, :]
        mem = (dot > 0) & (np.abs(crs) <= TAN30 * dot)
        sx = sx + np.where(mem, ax, z)
        sy = sy + np.where(mem, ay, z)
    score = sx * sx + sy * sy
    win = np.argmax(score, 1)  # the first (lowest) window among equals
    r = np.arange(n)
    bx, by, best = sx[r, win], sy[r, win], score[r, win]
    with np.errstate(all="ignore"):
        nrm = np.sqrt(bx * bx + by * by)
        c = np.where(best > 0, bx / nrm, f32(1)).astype(f32)
        sn = np.where(best > 0, by / nrm, f32(0)).astype(f32)
    ang = np.degrees(np.arctan2(by.astype(np.float64), bx.astype(np.float64)))
    ang = np.where(ang < 0, ang + 360.0, ang)
    return c, sn, np.where(best > 0, ang, 0.0).astype(f32)


def descriptor(I, px, py, s, c, sn):
    n = px.size
    hs = np.maximum(1, _round(s))
    q = np.arange(400)
    half = f32(0.5)
    fu = ((q % 20 - 10).astype(f32) + half)[None, :] * s[:, None]
    fv = ((q // 20 - 10).astype(f32) + half)[None, :] * s[:, None]
    C, S = c[:, None], sn[:, None]
    X = px[:, None] + (C * fu - S * fv)
    Y = py[:, None] + (S * fu + C * fv)
    dx, dy = haar(I, _round(Y), _round(X), hs[:, None])
    fx, fy = dx.astype(f32), dy.astype(f32)
    tx = DESC_G[None, :] * (C * fx + S * fy)
    ty = DESC_G[None, :] * (C * fy - S * fx)
    lane = np.arange(64)
    sr, comp = lane >> 2, lane & 3
    sri, srj = sr >> 2, sr & 3
    acc = np.zeros((n, 64), f32)
    for a in range(5):
        for b in range(5):
            idx = (sri * 5 + a) * 20 + srj * 5 + b
            v = np.where((comp & 1)[None, :] == 1, ty[:, idx], tx[:, idx])
            acc = acc + np.where(comp[None, :] >= 2, np.abs(v), v)
    sq = acc * acc
    for off in (32, 16, 8, 4, 2, 1):  # butterfly over the 64 columns
        sq = sq + sq[:, lane ^ off]
    with np.errstate(all="ignore"):
        nrm = np.sqrt(sq)
        out = np.where(nrm > 0, acc / nrm, f32(0))
    return out.astype(f32)


def extract(img, MetricThreshold=1000.0, NumOctaves=8, NumScaleLevels=4, upright=False):
    """(desc n x 64 f32, loc n x 2 f64 [x y] 1-based, aux n x 4 f32 [scale, angle_deg, metric, sign_of_laplacian])."""
    I = integral(gray_plane(img))
    k = detect(I, MetricThreshold, NumOctaves, NumScaleLevels)
    n = k["px"].size
    if upright or n == 0:
        c, sn, ang = np.ones(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    else:
        c, sn, ang = orientation(I, k["px"], k["py"], k["scale"])
    desc = descriptor(I, k["px"], k["py"], k["scale"], c, sn) if n else np.zeros((0, 64), f32)
    loc = np.stack([k["px"].astype(np.float64) + 1.0, k["py"].astype(np.float64) + 1.0], 1)
    aux = np.stack([k["scale"], ang, k["metric"], np.sign(k["trace"]).astype(f32)], 1).astype(f32)
    return desc, loc, aux
