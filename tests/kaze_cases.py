"""Seeded test images and the device cases of the KAZE tests (helper, not a test).  The images are surf_cases' band-limited noise
and its frozen homography pair; the mirror's result of a case is computed once and shared read-only."""
import numpy as np

import kaze_mirror as km
import surf_cases as sc
from surf_cases import PAIR_H, band_limited, pair, ratio_matches, transfer_error  # noqa: F401  (the tests take them from here)

# name: (image builder, keyword arguments of kaze_mirror.extract = keys of kaze_extract's input) - what it catches.
# The plane kernels work on 64 x 16 tiles, the detection on 64 x 8 tiles = one 64-bit bitmap word per row and tile, the histogram
# in sweeps of 1024 x 256 pixels.
CASES = {
    "64x64": (lambda: band_limited(2, 64, 64, 2.0), {}),                       # one tile column: borders everywhere, three levels fit
    "97x131": (lambda: band_limited(2, 97, 131, 2.5), {}),                     # odd sizes, tails of every tile and bitmap word
    "131x97x3": (lambda: band_limited(3, 131, 97, 2.5, channels=3), {}),       # RGB path, transposed tails
    "pairA": (lambda: pair()[0], {}),                                          # 240 x 320: every level of the default call
    "48x2100": (lambda: band_limited(4, 48, 2100, 2.5), {}),                   # 33 tile columns and bitmap words in three tile rows
    "2100x48": (lambda: band_limited(5, 2100, 48, 2.5), {}),                   # 132 tile rows, 263 detection rows, one word per row
    "O1S3": (lambda: band_limited(7, 200, 240, 2.5), {"NumOctaves": 1, "NumScaleLevels": 3}),   # a single interior level
    "O4S4": (lambda: band_limited(7, 300, 300, 6.0), {"NumOctaves": 4, "NumScaleLevels": 4}),   # 16 levels, derivative steps to 22
    "many": (lambda: band_limited(6, 480, 640, 2.5), {"Threshold": 1e-5}),     # thousands of keypoints, two histogram sweeps
}
_MIRROR = {}


def mirror(name):
    """(image, keyword arguments, desc, loc, aux) of a case."""
    if name not in _MIRROR:
        build, kw = CASES[name]
        img = build()
        out = km.extract(img, **kw)
        for a in out:
            a.setflags(write=False)
        _MIRROR[name] = (img, kw) + out
    return _MIRROR[name]


def blob(amplitude, sigma=4.0):
    """A dark Gaussian blob centred on pixel (64, 64) of a 128 x 128 field of gray 200."""
    yy, xx = np.mgrid[0:128, 0:128]
    return np.round(200.0 - amplitude * np.exp(-((xx - 64) ** 2 + (yy - 64) ** 2) / (2.0 * sigma ** 2))).astype(np.uint8)


def oriented_patch():
    """129 x 129: band-limited noise plus a few blobs, without symmetry (test_surf_mirror's patch)."""
    img = sc.band_limited(11, 129, 129, 3.0, contrast=0.8).astype(np.float64)
    yy, xx = np.mgrid[0:129, 0:129]
    for cx, cy, s, a in ((50, 60, 4.0, 70.0), (80, 45, 5.0, -60.0), (70, 85, 3.5, 60.0)):
        img -= a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


# the 2 x 1 synth scene of the stitch tests: 640 x 480 views, f = 900, neighbours 30 % of a field of view apart, finest_px = 3
SCENE = {"w": 640, "h": 480, "f": 900.0, "apart": 0.3, "finest_px": 3.0, "seed": 7}


def scene(synth, device):
    """(views as the renderer returns them, cameras) of SCENE on `device`."""
    s = SCENE
    cams = synth.grid_cameras(2, 1, s["w"], s["h"], s["f"], 2 * np.arctan(s["w"] / (2 * s["f"])) * s["apart"],
                              2 * np.arctan(s["h"] / (2 * s["f"])) * s["apart"], 1.0, s["seed"])
    return [synth.render_view(cams[i], s["h"], s["w"], s["seed"], device, finest_px=s["finest_px"]) for i in range(2)], cams
