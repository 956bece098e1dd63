"""Per-kernel time (aps_profile_*) of FAST/FREAK on one 3840 x 2160 synthetic view.  Prints one line per launch site."""
import sys
from importlib import import_module

sys.path.insert(0, ".")
import apsamd  # noqa: E402

fm = import_module(apsamd.__name__ + ".featureMatching")
synth = import_module(apsamd.__name__ + ".synth")
capi = apsamd._capi
W, H, f = 3840, 2160, 4000.0
cam = synth.grid_cameras(1, 1, W, H, f, 0.1, 0.1, 0.0, 5)[0]
img = synth.render_view(cam, H, W, 5, "cuda", finest_px=1.0)
import torch  # noqa: E402

torch.cuda.synchronize()
inp = {"detector": "FAST", "MinContrast": 0.08}  # (the synthetic world is smooth: the default 0.2 finds next to nothing)
fm.fast_extract(inp, img, device_out=True)  # warm-up: workspaces, code objects
capi.profile_enable(True)
capi.profile_reset()
reps = 5
for _ in range(reps):
    d, _ = fm.fast_extract(inp, img, device_out=True)
capi.check(capi.lib.aps_synchronize())
prof = {k: v for k, v in capi.profile_all().items() if v[1]}
capi.profile_enable(False)
total = sum(v[0] for v in prof.values()) / reps
print(f"FAST: {len(d)} features, {total:.3f} ms in profiled kernels per view")
for k, (ms, n) in sorted(prof.items()):
    print(f"  {k:20s} {ms / reps:8.3f} ms  ({n // reps} launches)")
