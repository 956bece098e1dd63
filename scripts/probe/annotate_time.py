"""Cost of the annotated panorama on a bench-sized resident canvas (21123 x 11632, 737 MB) with 64 image-sized outlines:
aps_annotate_panorama out of place (copy + drawing) and in place (drawing alone: host binning, one upload, one launch) beside a
plain device-to-device copy of the same canvas, alternating in one process.  Wall times end in a device synchronise; the
library's own event brackets give the kernel ("annotate_tiles") and the copy ("annotate_copy") in a separate pass.

    python scripts/probe/annotate_time.py [repeats]
"""
import ctypes as C
import statistics
import sys
import time
from importlib import import_module

import numpy as np
import torch

sys.path.insert(0, ".")
import apsamd

rp = import_module(apsamd.__name__ + ".renderPanorama")
capi = apsamd._capi
REP = int(sys.argv[1]) if len(sys.argv) > 1 else 9
H, W, N = 11632, 21123, 64
assert apsamd.lib.aps_device_count() > 0, "needs a gfx950 device"

# 8 x 8 grid of slightly turned, slightly sheared 4000 x 3000 outlines that overlap their neighbours, as the warped views do
rng = np.random.default_rng(3)
polys = np.zeros((N, 4, 2))
for k in range(N):
    cx, cy = 1700 + (k % 8) * 2500 + rng.uniform(-60, 60), 1300 + (k // 8) * 1290 + rng.uniform(-40, 40)
    a = rng.uniform(-0.08, 0.08)
    base = np.array([[-2000, -1500], [2000, -1500], [2050, 1500], [-1950, 1450]], float)
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    polys[k] = base @ rot.T + [cx, cy]
centers = polys.mean(1)
colors = rp.vivid_palette(N)
perimeter = sum(np.hypot(*(polys[k, (e + 1) % 4] - polys[k, e])) for k in range(N) for e in range(4))

src = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
dst = torch.empty_like(src)
torch.cuda.synchronize()


def annotate(s, d):
    n = C.c_int(0)
    capi.check(capi.lib.aps_annotate_panorama(capi.ptr(s), H, W, capi.ptr(polys), capi.ptr(centers), capi.ptr(colors), N, 2,
                                              capi.ptr(d), C.byref(n)))
    capi.check(capi.lib.aps_synchronize())
    assert n.value == N


def copy():
    dst.copy_(src)
    torch.cuda.synchronize()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


work = src.clone()
torch.cuda.synchronize()
for _ in range(2):  # warm up every shape
    copy(), annotate(src, dst), annotate(work, work)
t_copy, t_out, t_in = [], [], []
for _ in range(REP):  # alternating
    t_copy.append(timed(copy))
    t_out.append(timed(lambda: annotate(src, dst)))
    t_in.append(timed(lambda: annotate(work, work)))
changed = int((dst != src).any(2).sum().item())
capi.profile_enable(True)
capi.profile_reset()
annotate(src, dst)
prof = capi.profile_all()
capi.profile_enable(False)
fmt = lambda v: f"median {statistics.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f})"  # noqa: E731
print(f"canvas {W} x {H} ({H * W * 3 / 1e6:.0f} MB), {N} outlines, perimeter {perimeter:.0f} px, {changed} pixels drawn, {REP} repeats")
print(f"plain device-to-device copy        : {fmt(t_copy)}")
print(f"aps_annotate_panorama, out of place: {fmt(t_out)}")
print(f"aps_annotate_panorama, in place    : {fmt(t_in)}")
print("event brackets: " + ", ".join(f"{k} = {v[0]:.3f} ms" for k, v in prof.items() if k.startswith("annotate")))
