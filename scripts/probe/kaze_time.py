"""Per-kernel time (aps_profile_*) of KAZE next to SURF and SIFT on one 3840 x 2160 synthetic view: one line per launch site,
and for KAZE's plane kernels the achieved bandwidth against their counted bytes (4 bytes per plane element read or written,
halos not counted)."""
import math
import sys
from importlib import import_module

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

# planes read + written per launch of a KAZE plane kernel site (DESIGN.md "KAZE contract")
O, S = 3, 4
NL = O * S
sig = [1.6 * math.pow(2.0, i / S) for i in range(NL)]
fed_steps = sum(int(math.ceil(math.sqrt(3.0 * (0.5 * sig[i + 1] ** 2 - 0.5 * sig[i] ** 2) / 0.25 + 0.25) - 0.5 - 1.0e-8) + 0.5)
                for i in range(NL - 1))
PLANES = {"kaze_blur0": 2, "kaze_smooth": 3 * NL, "kaze_deriv": 3 * NL, "kaze_response": 3 * NL, "kaze_fed": 3 * fed_steps}

for det, fn in (("KAZE", fm.kaze_extract), ("SURF", fm.surf_extract), ("SIFT", fm.sift_extract)):
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
        line = f"  {k:20s} {ms / reps:8.3f} ms  ({n // reps} brackets)"
        if det == "KAZE" and k in PLANES:
            gb = PLANES[k] * W * H * 4 / 1e9
            line += f"  {gb:6.2f} GB counted -> {gb / (ms / reps / 1e3) / 1e3:5.2f} TB/s"
        print(line)
    if det == "KAZE":
        print(f"  ({fed_steps} diffusion steps in {NL - 1} cycles; workspace {(5 + 3 * NL) * W * H * 4 / 1e9:.2f} GB of planes)")

# The selection keys and Upright (DESIGN.md "KAZE selection and Upright") against the call without keys, alternated in one process:
# SERIES rounds, each variant once per round.  Per variant the wall time of a resident call (library stream drained) and the
# profiled time of the sites that differ, as median (min-max) over the rounds.  The call without keys runs the parent's launches:
# the only comparison that matters is against that row.
import statistics  # noqa: E402
import time  # noqa: E402

VARIANTS = (("no keys", {}), ("NumStrongest=2000", {"NumStrongest": 2000}), ("NumUniform=2000", {"NumUniform": 2000}),
            ("Upright", {"Upright": True}), ("NumUniform=2000 + Upright", {"NumUniform": 2000, "Upright": True}))
SITES = ("kaze_keypoint", "kaze_select", "kaze_detect")
SERIES = 7
for _, keys in VARIANTS:
    fm.kaze_extract(dict(keys, detector="KAZE"), img, device_out=True)  # warm-up
wall = {name: [] for name, _ in VARIANTS}
site = {name: {s: [] for s in SITES} for name, _ in VARIANTS}
rows = {}
for _ in range(SERIES):
    for name, keys in VARIANTS:
        inp = dict(keys, detector="KAZE")
        capi.check(capi.lib.aps_synchronize())
        t0 = time.perf_counter()
        d, _ = fm.kaze_extract(inp, img, device_out=True)   # (drains the library's stream before it returns)
        wall[name].append((time.perf_counter() - t0) * 1e3)
        rows[name] = int(d.shape[0])
        capi.profile_enable(True)
        capi.profile_reset()
        fm.kaze_extract(inp, img, device_out=True)
        capi.check(capi.lib.aps_synchronize())
        prof = capi.profile_all()
        capi.profile_enable(False)
        for s in SITES:
            site[name][s].append(prof.get(s, (0.0, 0))[0])
fmt = lambda v: f"{statistics.median(v):7.3f} ({min(v):.3f}-{max(v):.3f})"  # noqa: E731
print(f"KAZE keys, {SERIES} alternating rounds, ms as median (min-max):")
for name, _ in VARIANTS:
    print(f"  {name:26s} {rows[name]:6d} rows  wall {fmt(wall[name])}  " + "  ".join(f"{s} {fmt(site[name][s])}" for s in SITES))
