"""One 64 x 4K render of the bench scene (8 x 8 views of 3840 x 2160, f = 8000, 5 bands, tile 2048) per projection mode:
'miller' against 'spherical' (the same tables, kernels and host footprints) and 'fisheye' / 'panini' against 'stereographic' (the
R_ref family: coverage kernel, rays evaluated in place).  Alternating series in one process, ms per call, median (range).
DESIGN.md, "Projection contract" records the result; nothing is asserted."""
import sys, time
import numpy as np, torch
sys.path.insert(0, ".")
import apsamd
from importlib import import_module
synth = import_module(apsamd.__name__ + ".synth")
pl = import_module(apsamd.__name__ + ".pipeline")
rp = import_module(apsamd.__name__ + ".renderPanorama")
capi = apsamd._capi
W, H, f = 3840, 2160, 8000.0
imgs, cams = synth.make_scene(8, 8, W, H, f, 0.4, device="cuda", finest_px=16.0)
inp = pl.default_input(bands=5)
sizes = [(H, W, 3)] * 64
opts = {"anglePower": 2, "blending": "multiband", "pyrLevels": 5, "pyrSigma": 1.0, "tile": (2048, 2048), "cropBorder": False}
MODES = tuple(sys.argv[1:]) or ("spherical", "miller", "stereographic", "fisheye", "panini")  # argv: a subset


def sync():
    capi.check(capi.lib.aps_synchronize()); torch.cuda.synchronize()


def render(mode):
    sync(); t0 = time.perf_counter()
    pano, _ = rp.renderPanorama(inp, imgs, sizes, cams, mode, 27, opts, device_out=True)
    sync()
    return 1e3 * (time.perf_counter() - t0), tuple(pano.shape[:2])


shape = {}
for m in MODES:  # warm-up: workspaces, tables
    for _ in range(2):
        _, shape[m] = render(m)
t = {m: [] for m in MODES}
for rep in range(7):
    for m in MODES:
        t[m].append(render(m)[0])
for m in MODES:
    v = np.array(t[m])
    print(f"{m:14s} canvas {shape[m][1]} x {shape[m][0]} ({shape[m][0] * shape[m][1] / 1e6:.1f} MPix): "
          f"{np.median(v):.2f} ms ({v.min():.2f}-{v.max():.2f}), {np.median(v) / (shape[m][0] * shape[m][1] / 1e6):.4f} ms/MPix", flush=True)
