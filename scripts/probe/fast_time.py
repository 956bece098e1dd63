"""Per-kernel time (aps_profile_*) of FAST/FREAK on one 3840 x 2160 synthetic view, at one or more values of NumLevels
(default: 1 and 8, the single level next to the pyramid).  Prints one line per launch site and, per NumLevels, the total of
each of --repeats groups of --reps extractions, whose spread is the noise of the figure.

    python scripts/probe/fast_time.py [--levels 1 8] [--scale 1.2] [--reps 5] [--repeats 3]
"""
import argparse
import sys
from importlib import import_module

sys.path.insert(0, ".")
import apsamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, nargs="+", default=[1, 8])
ap.add_argument("--scale", type=float, default=1.2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

fm = import_module(apsamd.__name__ + ".featureMatching")
synth = import_module(apsamd.__name__ + ".synth")
capi = apsamd._capi
W, H, f = 3840, 2160, 4000.0
cam = synth.grid_cameras(1, 1, W, H, f, 0.1, 0.1, 0.0, 5)[0]
img = synth.render_view(cam, H, W, 5, "cuda", finest_px=1.0)
import torch  # noqa: E402

torch.cuda.synchronize()
totals = {}
for nl in args.levels:
    # (the synthetic world is smooth: the default MinContrast 0.2 finds next to nothing)
    inp = {"detector": "FAST", "MinContrast": 0.08, "NumLevels": nl, "ScaleFactor": args.scale}
    fm.fast_extract(inp, img, device_out=True)  # warm-up: workspaces, code objects
    groups = []
    for _ in range(args.repeats):
        capi.profile_enable(True)
        capi.profile_reset()
        for _ in range(args.reps):
            d, _ = fm.fast_extract(inp, img, device_out=True)
        capi.check(capi.lib.aps_synchronize())
        prof = {k: v for k, v in capi.profile_all().items() if v[1]}
        capi.profile_enable(False)
        groups.append(sum(v[0] for v in prof.values()) / args.reps)
    totals[nl] = sorted(groups)[len(groups) // 2]
    print(f"FAST NumLevels={nl}: {len(d)} features, {totals[nl]:.3f} ms in profiled kernels per view "
          f"(groups of {args.reps}: {' '.join('%.3f' % g for g in groups)})")
    for k, (ms, n) in sorted(prof.items()):  # (the last group)
        print(f"  {k:20s} {ms / args.reps:8.3f} ms  ({n // args.reps} launches)")
if len(totals) > 1:
    base = totals[args.levels[0]]
    for nl in args.levels[1:]:
        print(f"NumLevels={nl} / NumLevels={args.levels[0]}: {totals[nl] / base:.2f}")
