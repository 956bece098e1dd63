"""Per-kernel time (aps_profile_*) of SURF and of SIFT on one 3840 x 2160 synthetic view.  Prints one line per launch site."""
import sys
from importlib import import_module

import numpy as np

sys.path.insert(0, ".")
import apsamd  # noqa: E402

fm = import_module(apsamd.__name__ + ".featureMatching")
synth = import_module(apsamd.__name__ + ".synth")
capi = apsamd._capi
W, H, f = 3840, 2160, 4000.0
cam = synth.grid_cameras(1, 1, W, H, f, 0.1, 0.1, 0.0, 5)[0]
img = synth.render_view(cam, H, W, 5, "cuda", finest_px=8.0)
import torch  # noqa: E402

torch.cuda.synchronize()
for det, fn in (("SURF", fm.surf_extract), ("SIFT", fm.sift_extract)):
    fn({"detector": det}, img, device_out=True)  # warm-up: workspaces, code objects
    capi.profile_enable(True)
    capi.profile_reset()
    reps = 5
    for _ in range(reps):
        d, _ = fn({"detector": det}, img, device_out=True)
    capi.check(capi.lib.aps_synchronize())
    prof = {k: v for k, v in capi.profile_all().items() if v[1]}
    capi.profile_enable(False)
    total = sum(v[0] for v in prof.values()) / reps
    print(f"{det}: {int(d.shape[0])} features, {total:.3f} ms in profiled kernels per view")
    for k, (ms, n) in sorted(prof.items()):
        print(f"  {k:20s} {ms / reps:8.3f} ms  ({n // reps} launches)")
