"""NumPy restatement of the KAZE contract (DESIGN.md "KAZE contract") -- test infrastructure, not a test.

Written from the contract, not from the kernels: ``np.float32`` arrays with the contract's written operation and summation
order (one rounding per written operation), the same f64 -> f32 host tables (``math.exp`` / ``math.cos`` / ``math.pow``, the
C library's functions), integers where the contract has integers (gray plane, histogram).  Every plane stencil reads an
index outside the plane at the nearest row / column (``_at``).  ``extract`` returns what ``aps_kaze_extract`` returns.
"""
import math

import numpy as np

from surf_mirror import ORI_DI, ORI_DJ, TAN30, WIN_C, WIN_S, gray_plane, refine

f32 = np.float32
TAU_MAX = 0.25
ORI_G = np.array([math.exp(-(di * di + dj * dj) / 12.5) for di, dj in zip(ORI_DI.tolist(), ORI_DJ.tolist())], np.float64).astype(f32)
G1 = np.array([math.exp(-((a - 4) ** 2 + (b - 4) ** 2) / 12.5) for a in range(9) for b in range(9)], np.float64).astype(f32)
G2 = np.array([math.exp(-((R - 1.5) ** 2 + (C - 1.5) ** 2) / 4.5) for R in range(4) for C in range(4)], np.float64).astype(f32)


def gauss_weights(sigma, radius):
    w = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(radius + 1)]
    total = w[0] + sum(2.0 * v for v in w[1:])
    return np.array([v / total for v in w], np.float64).astype(f32)


G_BASE, G_ONE = gauss_weights(1.6, 7), gauss_weights(1.0, 4)   # radius ceil(4 sigma)


def levels(n_octaves=3, n_sublevels=4):
    """Host tables of the O * S evolution levels (+ sigma of the level after the last, which the last margin needs)."""
    nl = n_octaves * n_sublevels
    sig = [1.6 * math.pow(2.0, i / n_sublevels) for i in range(nl + 1)]
    step = [int(math.floor(s + 0.5)) for s in sig[:nl]]
    return {
        "n": nl, "sigma64": sig, "sigma": np.array(sig[:nl], np.float64).astype(f32), "step": step,
        "margin": [int(math.ceil(5.0 * sig[i + 1])) + 2 for i in range(nl)],
        "inv": [f32(1.0 / (32.0 * s)) for s in step], "norm4": [f32(s * s * s * s) for s in sig[:nl]],
    }


def fed_taus(T):
    """(tau_j in f64 in the order of application, the same in natural order) of one FED cycle of stopping time T."""
    n = int(math.ceil(math.sqrt(3.0 * T / TAU_MAX + 0.25) - 0.5 - 1.0e-8) + 0.5)
    scale, c = 3.0 * T / (TAU_MAX * float(n * (n + 1))), 1.0 / (4.0 * n + 2.0)
    tau = []
    for j in range(n):
        hc = math.cos(math.pi * (2.0 * j + 1.0) * c)
        tau.append(scale * TAU_MAX / (2.0 * hc * hc))
    prime = n + 1
    while prime < 2 or any(prime % d == 0 for d in range(2, int(math.isqrt(prime)) + 1)):
        prime += 1
    kappa = max(1, n // 2)
    out, k = [], 0
    for _ in range(n):
        while ((k + 1) * kappa) % prime - 1 >= n:
            k += 1
        out.append(tau[((k + 1) * kappa) % prime - 1])
        k += 1
    return out, tau


def cycle_time(lv, i):
    s = lv["sigma64"]
    return 0.5 * s[i + 1] * s[i + 1] - 0.5 * s[i] * s[i]


def _at(P, dy, dx):
    """P[clamp(y + dy)][clamp(x + dx)] for every (y, x): the border rule."""
    h, w = P.shape
    return P[np.clip(np.arange(h) + dy, 0, h - 1)[:, None], np.clip(np.arange(w) + dx, 0, w - 1)[None, :]]


def blur(P, g):
    """Separable Gaussian, rows first: acc = w0 x0, then acc = acc + wk (x[-k] + x[+k]), k ascending."""
    for axis in (1, 0):
        sh = (lambda k: (0, k)) if axis == 1 else (lambda k: (k, 0))
        acc = g[0] * P
        for k in range(1, len(g)):
            acc = acc + g[k] * (_at(P, *sh(-k)) + _at(P, *sh(k)))
        P = acc
    return P


def scharr(P, s, inv):
    """(d/dx, d/dy) at step s: differences first, the outer rows (columns) summed before the weights."""
    da, db, dc = _at(P, -s, s) - _at(P, -s, -s), _at(P, 0, s) - _at(P, 0, -s), _at(P, s, s) - _at(P, s, -s)
    ea, eb, ec = _at(P, s, -s) - _at(P, -s, -s), _at(P, s, 0) - _at(P, -s, 0), _at(P, s, s) - _at(P, -s, s)
    return (f32(3) * (da + dc) + f32(10) * db) * inv, (f32(3) * (ea + ec) + f32(10) * eb) * inv


def contrast_factor(P0):
    """k (f32): 70th percentile of the gradient magnitude of the sigma 1 smoothed input over a 300-bin integer histogram."""
    lx, ly = scharr(blur(P0, G_ONE), 1, f32(0.03125))
    mag = np.sqrt(lx * lx + ly * ly)
    hmax = mag.max()
    pos = mag[mag > 0]
    with np.errstate(all="ignore"):
        bins = np.minimum(299, ((pos / hmax) * f32(300)).astype(np.int64))
    hist = np.bincount(bins, minlength=300)
    want, seen, k = (int(pos.size) * 7) // 10, 0, 0
    while seen < want and k < 300:
        seen += int(hist[k])
        k += 1
    return f32(0.03) if k == 0 else hmax * (f32(k) / f32(300))


def conductivity(Ls, k2):
    lx, ly = scharr(Ls, 1, f32(0.03125))
    return f32(1) / (f32(1) + (lx * lx + ly * ly) / k2)


def fed_step(L, c, half_tau):
    xpos = (c + _at(c, 0, 1)) * (_at(L, 0, 1) - L)
    xneg = (_at(c, 0, -1) + c) * (L - _at(L, 0, -1))
    ypos = (c + _at(c, 1, 0)) * (_at(L, 1, 0) - L)
    yneg = (_at(c, -1, 0) + c) * (L - _at(L, -1, 0))
    return L + f32(half_tau) * ((xpos - xneg) + (ypos - yneg))


def level_planes(L, lv, i):
    """(Ls, Lx, Ly, response) of level i from its plane L."""
    Ls = blur(L, G_ONE)
    s, inv = lv["step"][i], lv["inv"][i]
    lx, ly = scharr(Ls, s, inv)
    lxx, lxy = scharr(lx, s, inv)
    lyy = scharr(ly, s, inv)[1]
    return Ls, lx, ly, (lxx * lyy - lxy * lxy) * lv["norm4"][i]


def scale_space(img, n_octaves=3, n_sublevels=4):
    """(levels, Lx[i], Ly[i], R[i]) of an image (uint8, gray or RGB)."""
    lv = levels(n_octaves, n_sublevels)
    P0 = gray_plane(img).astype(f32) * f32(1.0 / 255.0)
    k = contrast_factor(P0)
    k2 = k * k
    L = blur(P0, G_BASE)
    LX, LY, RR = [], [], []
    for i in range(lv["n"]):
        Ls, lx, ly, r = level_planes(L, lv, i)
        LX.append(lx), LY.append(ly), RR.append(r)
        if i + 1 < lv["n"]:
            c = conductivity(Ls, k2)
            for tau in fed_taus(cycle_time(lv, i))[0]:
                L = fed_step(L, c, f32(0.5 * tau))
    return lv, LX, LY, RR


def detect(lv, RR, thr):
    """Keypoints in canonical order (level, row, col): dict of arrays."""
    h, w = RR[0].shape
    thr = f32(thr)
    K = {k: [] for k in ("m", "i", "j", "ox", "oy", "os", "metric")}
    for m in range(1, lv["n"] - 1):
        mg = lv["margin"][m]
        ii, jj = np.mgrid[0:h, 0:w]
        cand = (RR[m] > thr) & (ii >= mg) & (ii <= h - 1 - mg) & (jj >= mg) & (jj <= w - 1 - mg)
        ci, cj = np.nonzero(cand)  # row-major: ascending (row, col)
        if ci.size == 0:
            continue
        nb = np.stack([np.stack([np.stack([RR[m + dz][ci + dy, cj + dx] for dx in (-1, 0, 1)], -1) for dy in (-1, 0, 1)], -2)
                       for dz in (-1, 0, 1)], -3)  # [n, 3, 3, 3]
        v = nb[:, 1, 1, 1]
        others = nb.reshape(-1, 27)[:, [k for k in range(27) if k != 13]]
        mx = (v[:, None] > others).all(1)
        ok, ox, oy, os_ = refine(nb)
        keep = mx & ok
        for k, val in (("m", np.full(int(keep.sum()), m)), ("i", ci[keep]), ("j", cj[keep]), ("ox", ox[keep]), ("oy", oy[keep]),
                       ("os", os_[keep]), ("metric", v[keep])):
            K[k].append(val)
    out = {}
    for k, lst in K.items():
        dt = np.int64 if k in ("m", "i", "j") else f32
        out[k] = np.concatenate(lst).astype(dt) if lst else np.zeros(0, dt)
    m, sg = out["m"], lv["sigma"]
    out["px"] = out["j"].astype(f32) + out["ox"]
    out["py"] = out["i"].astype(f32) + out["oy"]
    if m.size:
        up = sg[m] + out["os"] * (sg[m + 1] - sg[m])
        dn = sg[m] + out["os"] * (sg[m] - sg[m - 1])
        out["scale"] = np.where(out["os"] >= 0, up, dn).astype(f32)
    else:
        out["scale"] = np.zeros(0, f32)
    return out


def _round(v):
    return np.floor(v + f32(0.5)).astype(np.int64)


def orientation(LX, LY, m, px, py, s):
    """(c, sn, angle_deg) per keypoint, from the stored derivative planes of its level."""
    n = px.size
    h, w = LX[0].shape
    X = px[:, None] + ORI_DJ.astype(f32)[None, :] * s[:, None]
    Y = py[:, None] + ORI_DI.astype(f32)[None, :] * s[:, None]
    ix, iy = np.clip(_round(X), 0, w - 1), np.clip(_round(Y), 0, h - 1)
    dx, dy = np.zeros((n, 109), f32), np.zeros((n, 109), f32)
    for lvl in np.unique(m):
        q = m == lvl
        dx[q], dy[q] = LX[lvl][iy[q], ix[q]], LY[lvl][iy[q], ix[q]]
    vx, vy = ORI_G[None, :] * dx, ORI_G[None, :] * dy
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


def _bilinear(P, y0, y1, x0, x1, ay, ax):
    p00, p01, p10, p11 = P[y0, x0], P[y0, x1], P[y1, x0], P[y1, x1]
    top, bot = p00 + ax * (p01 - p00), p10 + ax * (p11 - p10)
    return top + ay * (bot - top)


def descriptor(LX, LY, m, px, py, s, c, sn):
    n = px.size
    h, w = LX[0].shape
    q = np.arange(576)
    fu = (q % 24 - 12).astype(f32)[None, :] * s[:, None]
    fv = (q // 24 - 12).astype(f32)[None, :] * s[:, None]
    C, S = c[:, None], sn[:, None]
    X = px[:, None] + (C * fu - S * fv)
    Y = py[:, None] + (S * fu + C * fv)
    xf, yf = np.floor(X), np.floor(Y)
    ax, ay = X - xf, Y - yf
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    x0, x1, y0, y1 = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1), np.clip(yi, 0, h - 1), np.clip(yi + 1, 0, h - 1)
    fx, fy = np.zeros((n, 576), f32), np.zeros((n, 576), f32)
    for lvl in np.unique(m):
        k = m == lvl
        fx[k] = _bilinear(LX[lvl], y0[k], y1[k], x0[k], x1[k], ay[k], ax[k])
        fy[k] = _bilinear(LY[lvl], y0[k], y1[k], x0[k], x1[k], ay[k], ax[k])
    tx, ty = C * fx + S * fy, C * fy - S * fx
    lane = np.arange(64)
    sr, comp = lane >> 2, lane & 3
    sri, srj = sr >> 2, sr & 3
    acc = np.zeros((n, 64), f32)
    for a in range(9):
        for b in range(9):
            idx = (sri * 5 + a) * 24 + srj * 5 + b
            t = G1[a * 9 + b] * np.where((comp & 1)[None, :] == 1, ty[:, idx], tx[:, idx])
            acc = acc + np.where(comp[None, :] >= 2, np.abs(t), t)
    acc = acc * G2[sri * 4 + srj][None, :]
    sq = acc * acc
    for off in (32, 16, 8, 4, 2, 1):  # butterfly over the 64 columns
        sq = sq + sq[:, lane ^ off]
    with np.errstate(all="ignore"):
        nrm = np.sqrt(sq)
        out = np.where(nrm > 0, acc / nrm, f32(0))
    return out.astype(f32)


def extract(img, Threshold=0.0001, NumOctaves=3, NumScaleLevels=4):
    """(desc n x 64 f32, loc n x 2 f64 [x y] 1-based, aux n x 4 f32 [scale, angle_deg, metric, level])."""
    img = np.asarray(img)
    lv = levels(NumOctaves, NumScaleLevels)
    if min(img.shape[:2]) < 2 * lv["margin"][1] + 1:
        return np.zeros((0, 64), f32), np.zeros((0, 2), np.float64), np.zeros((0, 4), f32)
    lv, LX, LY, RR = scale_space(img, NumOctaves, NumScaleLevels)
    k = detect(lv, RR, Threshold)
    n = k["px"].size
    if n == 0:
        return np.zeros((0, 64), f32), np.zeros((0, 2), np.float64), np.zeros((0, 4), f32)
    c, sn, ang = orientation(LX, LY, k["m"], k["px"], k["py"], k["scale"])
    desc = descriptor(LX, LY, k["m"], k["px"], k["py"], k["scale"], c, sn)
    loc = np.stack([k["px"].astype(np.float64) + 1.0, k["py"].astype(np.float64) + 1.0], 1)
    aux = np.stack([k["scale"], ang, k["metric"], k["m"].astype(f32)], 1).astype(f32)
    return desc, loc, aux
