"""Cost of a match plot of two resident 3840 x 2160 views with 2000 synthetic matches: imageProcessing.montage_pair (two strided
copies), aps_draw_marks in place on the montage (host binning, one upload, one launch), and the whole
imageMatching.showMatchedFeatures, beside the copies alone of the path a user has without them - both views device-to-host,
one host-made montage host-to-device (the host's drawing not counted) - alternating in one process.  Wall times end in a
device synchronise; the library's own event brackets give the kernel ("mark_tiles") and the copies ("montage_pair") in a
separate pass.

    python scripts/probe/marks_time.py [repeats]
"""
import statistics
import sys
import time
from importlib import import_module

import numpy as np
import torch

sys.path.insert(0, ".")
import apsamd

im = import_module(apsamd.__name__ + ".imageMatching")
ip = import_module(apsamd.__name__ + ".imageProcessing")
capi = apsamd._capi
REP = int(sys.argv[1]) if len(sys.argv) > 1 else 9
H, W, N = 2160, 3840, 2000
assert apsamd.lib.aps_device_count() > 0, "needs a gfx950 device"

rng = np.random.default_rng(3)
# matches of two views that overlap by about half, as neighbours of a panorama do: the same scene points, shifted and jittered
p1 = np.stack([rng.uniform(W / 2, W, N), rng.uniform(1, H, N)], axis=1)
p2 = p1 - [W / 2, 0] + rng.normal(0, 6, (N, 2))
marks = im.match_plot_marks(p1, p2, W)
I1 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
I2 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
canvas = ip.montage_pair(I1, I2)
host_montage = torch.empty((H, 2 * W, 3), dtype=torch.uint8).pin_memory()
host_1, host_2 = torch.empty((H, W, 3), dtype=torch.uint8).pin_memory(), torch.empty((H, W, 3), dtype=torch.uint8).pin_memory()
dev_montage = torch.empty_like(canvas)
torch.cuda.synchronize()


def sync():
    capi.check(capi.lib.aps_synchronize())
    torch.cuda.synchronize()


def montage():
    ip.montage_pair(I1, I2)
    sync()


def draw():
    capi.check(capi.lib.aps_draw_marks(capi.ptr(canvas), H, 2 * W, capi.ptr(marks), len(marks), capi.ptr(canvas), None))
    sync()


def whole():
    im.showMatchedFeatures(I1, I2, p1, p2)
    sync()


def download_path():
    host_1.copy_(I1)
    host_2.copy_(I2)
    dev_montage.copy_(host_montage)
    sync()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


legs = [("montage_pair (two resident 4K views)", montage), ("aps_draw_marks, in place", draw),
        ("showMatchedFeatures, whole", whole), ("copies of the download path", download_path)]
for _ in range(2):  # warm up every shape
    for _, fn in legs:
        fn()
times = {name: [] for name, _ in legs}
for _ in range(REP):  # alternating
    for name, fn in legs:
        times[name].append(timed(fn))
plain = ip.montage_pair(I1, I2)
changed = int((canvas != plain).any(2).sum().item())
capi.profile_enable(True)
capi.profile_reset()
whole()
prof = capi.profile_all()
capi.profile_enable(False)
fmt = lambda v: f"median {statistics.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f})"  # noqa: E731
print(f"two {W} x {H} views, montage {2 * W} x {H} ({H * 2 * W * 3 / 1e6:.0f} MB), {N} matches = {len(marks)} marks, {changed} pixels drawn, "
      f"{REP} repeats")
for name, _ in legs:
    print(f"{name:38s}: {fmt(times[name])}")
print("event brackets: " + ", ".join(f"{k} = {v[0]:.3f} ms" for k, v in prof.items() if k.startswith(("mark", "montage"))))
