"""Per-kernel time (aps_profile_*) of FAST/FREAK on one 3840 x 2160 synthetic view, at one or more values of NumLevels
(default: 1 and 8, the single level next to the pyramid) and, with --strongest N, of the same values with NumStrongest = N.
Prints one line per launch site and, per row, the total of each of --repeats groups of --reps extractions, whose spread is the
noise of the figure.  The groups of the rows alternate, so drift of the device shows as spread and not as a difference of rows.
With --orb every row is timed a second time with DescriptorMethod = 'ORB' (orb_keypoint_kernel beside freak_keypoint_kernel), and
with --match the batched pairwise Hamming matcher is timed on the rows of two such views at 64 bytes (FREAK) and at 32 (ORB): the
same keypoints, host clock around calls that end in a synchronise, alternating groups again.
With --corner harris every row is timed once more with CornerMethod = 'Harris' (launch site harris_detect: harris_detect_kernel and
harris_gate_kernel, beside fast_detect: fast_detect_kernel, fast_smax_kernel and fast_gate_kernel).

    python scripts/probe/fast_time.py [--levels 1 8] [--scale 1.2] [--reps 5] [--repeats 5] [--strongest 5000] [--orb] [--match]
                                      [--corner harris]
"""
import argparse
import statistics
import sys
import time
from importlib import import_module

sys.path.insert(0, ".")
import apsamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, nargs="+", default=[1, 8])
ap.add_argument("--scale", type=float, default=1.2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--strongest", type=int, default=None, help="also time every NumLevels with NumStrongest = N")
ap.add_argument("--orb", action="store_true", help="also time every row with DescriptorMethod = 'ORB'")
ap.add_argument("--match", action="store_true", help="time batched pairwise matching of two views' rows at 64 and 32 bytes")
ap.add_argument("--corner", choices=["harris"], default=None, help="also time every row with CornerMethod = 'Harris'")
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
rows = [row + (m,) for row in rows for m in (("FREAK", "ORB") if args.orb else ("FREAK",))]
rows = [row + (c,) for row in rows for c in (("FAST", "Harris") if args.corner else ("FAST",))]


def inputs(nl, strongest, method="FREAK", corner="FAST"):
    # (the synthetic world is smooth: the default MinContrast 0.2 finds next to nothing)
    inp = {"detector": "FAST", "MinContrast": 0.08, "NumLevels": nl, "ScaleFactor": args.scale}
    if method != "FREAK":
        inp["DescriptorMethod"] = method
    if corner != "FAST":
        inp["CornerMethod"] = corner
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
    nl, strongest, method, corner = row
    g = groups[row]
    totals[row] = statistics.median(g)
    name = f"NumLevels={nl}" + ("" if strongest is None else f" NumStrongest={strongest}")
    print(f"{corner}/{method} {name}: {found[row]} features, {totals[row]:.3f} ms in profiled kernels per view, range {min(g):.3f} .. {max(g):.3f} "
          f"(groups of {args.reps}: {' '.join('%.3f' % v for v in g)})")
    for k, (ms, n) in sorted(last[row].items()):  # (the last group)
        print(f"  {k:20s} {ms / args.reps:8.3f} ms  ({n // args.reps} launches)")
base = totals[rows[0]]
for row in rows[1:]:
    print(f"{row} / {rows[0]}: {totals[row] / base:.2f}")

if args.match:
    # two overlapping views; the rows of both descriptors are those of the same keypoints
    cams = synth.grid_cameras(2, 1, W, H, f, 0.1, 0.0, 0.0, 5)
    pair = [synth.render_view(c, H, W, 5, "cuda", finest_px=1.0) for c in cams]
    torch.cuda.synchronize()
    sets = {m: [fm.fast_extract(inputs(args.levels[0], None, m), v, device_out=True)[0] for v in pair] for m in ("FREAK", "ORB")}
    capi.check(capi.lib.aps_synchronize())
    times, n_match = {m: [] for m in sets}, {}
    for m in sets:
        fm.match_pairwise_binary_csr(sets[m], 0.6, 20.0, True)  # warm-up
    for _ in range(args.repeats):
        for m in sets:
            capi.check(capi.lib.aps_synchronize())
            t0 = time.perf_counter()
            for _ in range(args.reps):
                ptr, ii, jj, _ = fm.match_pairwise_binary_csr(sets[m], 0.6, 20.0, True)
            capi.check(capi.lib.aps_synchronize())
            times[m].append((time.perf_counter() - t0) * 1e3 / args.reps)
            n_match[m] = len(ii)
    for m in sets:
        g = times[m]
        print(f"match {m} ({sets[m][0].Features.shape[1]} bytes, {len(sets[m][0])} x {len(sets[m][1])} rows, {n_match[m]} matches): "
              f"{statistics.median(g):.3f} ms per call, range {min(g):.3f} .. {max(g):.3f} ({' '.join('%.3f' % v for v in g)})")
    print(f"match ORB / FREAK: {statistics.median(times['ORB']) / statistics.median(times['FREAK']):.2f}")
