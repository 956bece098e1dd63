"""NumPy restatement of the lens distortion contract ("Lens distortion contract"; include/aps.h, aps_lens): f64
throughout, every expression parenthesised and ordered as the contract writes it, so that the device's bytes and bits can be
compared with no tolerance.  A lens is a dict with the nine keys of aps_lens."""
import numpy as np

FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2")
INVERSE_STEPS = 20

# the lenses of the test cases: name -> (H, W, fx, fy, k, p); cx = (W + 1) / 2 + 1.3, cy = (H + 1) / 2 - 0.7
_BARREL_K, _BARREL_P = (-0.25, 0.08), (1e-3, -5e-4)
CASES = {
    "barrel": (61, 83, 70.0, 70.0, _BARREL_K, _BARREL_P),
    "pincushion": (61, 83, 70.0, 70.0, (0.12, 0.02), (0.0, 0.0)),
    "small": (47, 49, 40.0, 40.0, (-0.2, 0.05, 0.01), (1e-3, 1e-3)),
    "anisotropic": (70, 131, 90.0, 84.0, _BARREL_K, _BARREL_P),
    "long-row": (129, 1030, 800.0, 800.0, _BARREL_K, _BARREL_P),
}


def lens(fx, fy, cx, cy, k=(0.0, 0.0), p=(0.0, 0.0)):
    k = tuple(float(v) for v in k) + (0.0,) * (3 - len(k))
    return dict(zip(FIELDS, (float(fx), float(fy), float(cx), float(cy)) + k + (float(p[0]), float(p[1]))))


def case(name):
    """(H, W, lens) of a named test case."""
    h, w, fx, fy, k, p = CASES[name]
    return h, w, lens(fx, fy, (w + 1) / 2 + 1.3, (h + 1) / 2 - 0.7, k, p)


def _terms(L, x, y):
    r2 = x * x + y * y
    rad = 1 + r2 * (L["k1"] + r2 * (L["k2"] + r2 * L["k3"]))
    dx = ((2 * L["p1"]) * x) * y + L["p2"] * (r2 + (2 * x) * x)
    dy = L["p1"] * (r2 + (2 * y) * y) + ((2 * L["p2"]) * x) * y
    return rad, dx, dy


def distort(L, u, v):
    """The forward map: ideal (u, v) -> distorted (ud, vd), elementwise on f64 arrays."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    x, y = (u - L["cx"]) / L["fx"], (v - L["cy"]) / L["fy"]
    rad, dx, dy = _terms(L, x, y)
    return L["fx"] * (x * rad + dx) + L["cx"], L["fy"] * (y * rad + dy) + L["cy"]


def undistort_points(L, pts):
    """The inverse map of n x 2 [x y] points: exactly INVERSE_STEPS fixed-point steps, no convergence test."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    xd, yd = (pts[:, 0] - L["cx"]) / L["fx"], (pts[:, 1] - L["cy"]) / L["fy"]
    x, y = xd.copy(), yd.copy()
    with np.errstate(all="ignore"):
        for _ in range(INVERSE_STEPS):
            rad, dx, dy = _terms(L, x, y)
            x, y = (xd - dx) / rad, (yd - dy) / rad
    return np.stack([L["fx"] * x + L["cx"], L["fy"] * y + L["cy"]], axis=1)


def valid_view(L, h, w):
    """(x0, y0, out_h, out_w) of the 'valid' view: the rectangle inside the undistorted images of the four border lines."""
    cols, rows = np.arange(1, w + 1, dtype=np.float64), np.arange(1, h + 1, dtype=np.float64)
    top = undistort_points(L, np.stack([cols, np.full(w, 1.0)], 1))[:, 1]
    bottom = undistort_points(L, np.stack([cols, np.full(w, float(h))], 1))[:, 1]
    left = undistort_points(L, np.stack([np.full(h, 1.0), rows], 1))[:, 0]
    right = undistort_points(L, np.stack([np.full(h, float(w)), rows], 1))[:, 0]
    x0, x1 = int(np.ceil(left.max())), int(np.floor(right.min()))
    y0, y1 = int(np.ceil(top.max())), int(np.floor(bottom.min()))
    if x1 < x0 or y1 < y0:
        raise ValueError("the valid view is empty")
    return x0, y0, y1 - y0 + 1, x1 - x0 + 1


def view(L, h, w, output_view):
    return (1, 1, h, w) if output_view == "same" else valid_view(L, h, w)


def is_identity(L):
    return all(L[k] == 0 for k in ("k1", "k2", "k3", "p1", "p2"))


def sample_map(L, h, w, x0, y0, out_h, out_w):
    """(ud, vd, valid) of every output pixel of the view: the sample positions in the h x w source."""
    u, v = np.meshgrid(np.arange(out_w, dtype=np.float64) + x0, np.arange(out_h, dtype=np.float64) + y0)
    ud, vd = (u, v) if is_identity(L) else distort(L, u, v)
    with np.errstate(invalid="ignore"):
        valid = (ud >= 1) & (ud <= w) & (vd >= 1) & (vd <= h)
    return ud, vd, valid


def _round_half_away(s):
    t = np.trunc(s)  # (s - t is exact, so the tie test is too; floor(s + 0.5) is not: 0.49999999999999994 + 0.5 == 1)
    return t + np.sign(s) * (np.abs(s - t) >= 0.5)


def bilinear(img, xs, ys, valid, fill):
    """The four-tap sum of the contract at the 1-based positions (xs, ys) of img (H x W x C uint8); fill where not valid."""
    h, w, c = img.shape
    xs, ys = np.where(valid, xs, 1.0), np.where(valid, ys, 1.0)
    fx1, fy1 = np.floor(xs), np.floor(ys)
    x1, y1 = fx1.astype(np.int64), fy1.astype(np.int64)
    x2, y2 = np.minimum(x1 + 1, w), np.minimum(y1 + 1, h)
    wx, wy = xs - fx1, ys - fy1
    w11, w12, w21, w22 = (1 - wx) * (1 - wy), (1 - wx) * wy, wx * (1 - wy), wx * wy
    out = np.empty(xs.shape + (c,), np.uint8)
    for ch in range(c):
        p = img[:, :, ch].astype(np.float64)
        s = ((w11 * p[y1 - 1, x1 - 1] + w12 * p[y2 - 1, x1 - 1]) + w21 * p[y1 - 1, x2 - 1]) + w22 * p[y2 - 1, x2 - 1]
        out[..., ch] = np.where(valid, np.clip(_round_half_away(s), 0, 255), fill).astype(np.uint8)
    return out


def undistort_image(img, L, output_view="same", fill=0):
    """(J, (x0, y0)) as imageProcessing.undistortImage returns them, for img uint8 H x W or H x W x C."""
    img = np.asarray(img)
    sq = img.ndim == 2
    a = img[:, :, None] if sq else img
    h, w = a.shape[:2]
    x0, y0, oh, ow = view(L, h, w, output_view)
    ud, vd, valid = sample_map(L, h, w, x0, y0, oh, ow)
    out = bilinear(a, ud, vd, valid, fill)
    return (out[:, :, 0] if sq else out), (x0, y0)


def distort_image(img, L):
    """A distorted photograph of img for the tests (not part of the contract): every pixel of the result samples img bilinearly
    at undistort_points of its centre; 0 outside."""
    img = np.asarray(img)
    a = img[:, :, None] if img.ndim == 2 else img
    h, w = a.shape[:2]
    u, v = np.meshgrid(np.arange(1, w + 1, dtype=np.float64), np.arange(1, h + 1, dtype=np.float64))
    q = undistort_points(L, np.stack([u.ravel(), v.ravel()], 1))
    xs, ys = q[:, 0].reshape(h, w), q[:, 1].reshape(h, w)
    valid = (xs >= 1) & (xs <= w) & (ys >= 1) & (ys <= h)
    out = bilinear(a, xs, ys, valid, 0)
    return out[:, :, 0] if img.ndim == 2 else out
