"""Per-kernel time (aps_profile_*) of FAST/FREAK on one 3840 x 2160 synthetic view, at one or more values of NumLevels
(default: 1 and 8, the single level next to the pyramid) and, with --strongest N, of the same values with NumStrongest = N.
Prints one line per launch site and, per row, the total of each of --repeats groups of --reps extractions, whose spread is the
noise of the figure.  The groups of the rows alternate, so drift of the device shows as spread and not as a difference of rows.

    python scripts/probe/fast_time.py [--levels 1 8] [--scale 1.2] [--reps 5] [--repeats 5] [--strongest 5000]
"""
import argparse
import statistics
import sys
from importlib import import_module

sys.path.insert(0, ".")
import apsamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, nargs="+", default=[1, 8])
ap.add_argument("--scale", type=float, default=1.2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--strongest", type=int, default=None, help="also time every NumLevels with NumStrongest = N")
args = ap.parse_args()

fm = import_module(apsamd.__name__ + ".featureMatching")
synth = import_module(apsamd.__name__ + ".synth")
capi = apsamd._capi
W, H, f = 3840, 2160, 4000.0
cam = synth.grid_cameras(1, 1, W, H, f, 0.1, 0.1, 0.0, 5)[0]
img = synth.render_view(cam, H, W, 5, "cuda", finest_px=1.0)
import torch  # noqa: E402

torch.cuda.synchronize()
rows = [(nl, None) for nl in args.levels] + ([(nl, args.strongest) for nl in args.levels] if args.strongest is not None else [])


def inputs(nl, strongest):
    # (the synthetic world is smooth: the default MinContrast 0.2 finds next to nothing)
    inp = {"detector": "FAST", "MinContrast": 0.08, "NumLevels": nl, "ScaleFactor": args.scale}
    return inp if strongest is None else {**inp, "NumStrongest": strongest}


for row in rows:
    fm.fast_extract(inputs(*row), img, device_out=True)  # warm-up: workspaces, code objects
groups, last, found = {row: [] for row in rows}, {}, {}
for _ in range(args.repeats):
    for row in rows:
        capi.profile_enable(True)
        capi.profile_reset()
        for _ in range(args.reps):
            d, _ = fm.fast_extract(inputs(*row), img, device_out=True)
        capi.check(capi.lib.aps_synchronize())
        last[row] = {k: v for k, v in capi.profile_all().items() if v[1]}
        capi.profile_enable(False)
        found[row] = len(d)
        groups[row].append(sum(v[0] for v in last[row].values()) / args.reps)
totals = {}
for row in rows:
    nl, strongest = row
    g = groups[row]
    totals[row] = statistics.median(g)
    name = f"NumLevels={nl}" + ("" if strongest is None else f" NumStrongest={strongest}")
    print(f"FAST {name}: {found[row]} features, {totals[row]:.3f} ms in profiled kernels per view, range {min(g):.3f} .. {max(g):.3f} "
          f"(groups of {args.reps}: {' '.join('%.3f' % v for v in g)})")
    for k, (ms, n) in sorted(last[row].items()):  # (the last group)
        print(f"  {k:20s} {ms / args.reps:8.3f} ms  ({n // args.reps} launches)")
base = totals[rows[0]]
for row in rows[1:]:
    print(f"{row} / {rows[0]}: {totals[row] / base:.2f}")
