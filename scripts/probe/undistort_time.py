"""Cost of undistortImage on one resident 2160 x 3840 x 3 view (barrel coefficients at f = 3000, 'same' view) beside the yardstick
that moves the same bytes with a comparable per-pixel f64 chain: aps_image_warp_u8, bilinear, identity homography, same view.
Both in one process, alternating series of CALLS calls each; a series is timed by the host clock and ends in a device synchronise
(each entry also synchronises its own stream before it returns).  The spread the yardstick shows against itself in this run is
the range of its own series.  Bytes: one read and one write of the image.

    python scripts/probe/undistort_time.py [series] [calls per series]
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

ip = import_module(apsamd.__name__ + ".imageProcessing")
capi = apsamd._capi
SERIES = int(sys.argv[1]) if len(sys.argv) > 1 else 7
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
H, W, F = 2160, 3840, 3000.0
HBM_ACHIEVABLE = 6.3e12  # bytes per second, a streaming kernel's ceiling on this device
assert apsamd.lib.aps_device_count() > 0, "needs a gfx950 device"

lens = ip.cameraIntrinsics((F, F, (W + 1) / 2 + 1.3, (H + 1) / 2 - 0.7), (-0.25, 0.08), (1e-3, -5e-4))
img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
out_w = torch.empty_like(img)
eye = np.eye(3)
torch.cuda.synchronize()


def sync():
    capi.check(capi.lib.aps_synchronize())
    torch.cuda.synchronize()


def undistort():
    return ip.undistortImage(img, lens, "same")[0]


def warp():
    capi.check(capi.lib.aps_image_warp_u8(capi.ptr(img), H, W, 3, capi.ptr(eye), H, W, 1.0, 1.0, 1.0, 1.0, 0, capi.APS_WARP_BILINEAR,
                                          capi.ptr(out_w)))


def series(fn):
    sync()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / CALLS


legs = [("undistortImage, barrel, 'same'", undistort), ("aps_image_warp_u8, bilinear, identity", warp)]
for _, fn in legs:  # warm up both shapes
    for _ in range(5):
        fn()
assert torch.equal(out_w[:-1, :-1], img[:-1, :-1]), "the yardstick's identity warp is not a copy"  # (its last row and column are fill)
valid = float((undistort() != 0).any(2).float().mean().item())
times = {name: [] for name, _ in legs}
for _ in range(SERIES):  # alternating
    for name, fn in legs:
        times[name].append(series(fn))
capi.profile_enable(True)
capi.profile_reset()
for _ in range(CALLS):
    undistort()
kernel_ms, launches = capi.profile_get("undistort_image_u8")
capi.profile_enable(False)
nbytes = 2 * H * W * 3
print(f"one resident {H} x {W} x 3 view ({H * W * 3 / 1e6:.1f} MB), f = {F:.0f}, {SERIES} alternating series of {CALLS} calls; "
      f"{100 * valid:.1f} % of the output pixels are not black")
for name, _ in legs:
    v = times[name]
    med = statistics.median(v)
    print(f"{name:38s}: median {med:.4f} ms per call (min {min(v):.4f}, max {max(v):.4f}); {nbytes / (med * 1e-3) / 1e12:.3f} TB/s of one read "
          f"and one write = {100 * nbytes / (med * 1e-3) / HBM_ACHIEVABLE:.1f} % of {HBM_ACHIEVABLE / 1e12:.1f} TB/s")
k = kernel_ms / max(launches, 1)
print(f"event bracket undistort_image_u8: {k:.4f} ms per launch over {launches} launches; {nbytes / (k * 1e-3) / 1e12:.3f} TB/s = "
      f"{100 * nbytes / (k * 1e-3) / HBM_ACHIEVABLE:.1f} % of {HBM_ACHIEVABLE / 1e12:.1f} TB/s")
