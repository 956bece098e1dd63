"""The cost of multibandWeights = 'maxweight': the bench scene (8 x 8 views of 3840 x 2160, f = 8000, spherical, tile 2048) rendered
with bands 3 and 5 in both modes.  Alternating series in one process: the render stage in ms per call, median (range), and in a
series of its own under aps_profile_* the warp kernel (site render_warp), the shrinks and the collapse.  DESIGN.md, "Max-weight
multiband contract" records the result; nothing is asserted."""
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
sizes = [(H, W, 3)] * 64
CASES = [(b, w) for b in (3, 5) for w in ("tent", "maxweight")]
SITES = ("render_warp", "render_pyr_down", "render_collapse")


def sync():
    capi.check(capi.lib.aps_synchronize()); torch.cuda.synchronize()


def render(bands, weights):
    inp = pl.default_input(bands=bands)
    opts = {"anglePower": 2, "blending": "multiband", "multibandWeights": weights, "pyrLevels": bands, "pyrSigma": 1.0,
            "tile": (2048, 2048), "cropBorder": False}
    sync(); t0 = time.perf_counter()
    rp.renderPanorama(inp, imgs, sizes, cams, "spherical", 27, opts, device_out=True)
    sync()
    return 1e3 * (time.perf_counter() - t0)


for c in CASES:  # warm-up: workspaces, tables
    for _ in range(2):
        render(*c)
t = {c: [] for c in CASES}
for rep in range(7):
    for c in CASES:
        t[c].append(render(*c))
k = {c: {s: [] for s in SITES} for c in CASES}
capi.profile_enable(True)
for rep in range(5):
    for c in CASES:
        capi.profile_reset()
        render(*c)
        for s in SITES:
            k[c][s].append(capi.profile_get(s)[0])
capi.profile_enable(False)
for c in CASES:
    v = np.array(t[c])
    sites = ", ".join(f"{s} {np.median(k[c][s]):.2f}" for s in SITES)
    print(f"bands {c[0]} {c[1]:9s}: render {np.median(v):.2f} ms ({v.min():.2f}-{v.max():.2f}); kernels (ms): {sites}", flush=True)
