"""Time of one 3840 x 2160 synthetic view's extraction for three calls per detector (SIFT, SURF, FAST): no key, NumStrongest = N and
NumUniform = N (DESIGN.md "Uniform-N selection"), at several N.  Per row it prints the rows returned, the time in profiled kernels
(aps_profile_*, event-bracketed launch sites) and the host time of the call - a clock around extractions that end in a synchronise,
which includes the sorts and scans (no launch site of their own) and the read-backs.  Each figure is the median of --repeats groups
of --reps extractions with the range of the groups; the rows' groups alternate, so drift of the device shows as spread and not as
a difference of rows.

    python scripts/probe/uniform_time.py [--n 2000 5000] [--grid 8 8] [--reps 5] [--repeats 5] [--detectors SIFT SURF FAST] [--levels 8]
"""
import argparse
import statistics
import sys
import time
from importlib import import_module

sys.path.insert(0, ".")
import apsamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[2000, 5000])
ap.add_argument("--grid", type=int, nargs=2, default=[8, 8])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--detectors", nargs="+", default=["SIFT", "SURF", "FAST"])
ap.add_argument("--levels", type=int, default=8, help="NumLevels of the FAST rows")
ap.add_argument("--finest-px", type=float, default=16.0)
ap.add_argument("--focal", type=float, default=8000.0)
args = ap.parse_args()

fm = import_module(apsamd.__name__ + ".featureMatching")
pl = import_module(apsamd.__name__ + ".pipeline")
synth = import_module(apsamd.__name__ + ".synth")
capi = apsamd._capi
views, _ = synth.make_scene(2, 1, 3840, 2160, args.focal, 0.4, seed=5, device="cuda", finest_px=args.finest_px)
import torch  # noqa: E402

torch.cuda.synchronize()
img = views[0]


def inputs(det, key, N):
    inp = pl.default_input(detector=det)
    if det == "FAST":
        inp = {**inp, "NumLevels": args.levels}
    if key == "NumUniform":
        inp = {**inp, "UniformGrid": tuple(args.grid)}
    return inp if key is None else {**inp, key: N}


def sync():
    capi.check(capi.lib.aps_synchronize())
    torch.cuda.synchronize()


def n_rows(d):
    return d.NumFeatures if hasattr(d, "NumFeatures") else len(d)


for det in args.detectors:
    rows = [(None, None)] + [(key, N) for N in args.n for key in ("NumStrongest", "NumUniform")]
    for key, N in rows:
        fm.extract_features(inputs(det, key, N), img, device_out=True)  # warm-up: workspaces, code objects
    sync()
    groups, host, found = {r: [] for r in rows}, {r: [] for r in rows}, {}
    for _ in range(args.repeats):
        for r in rows:
            inp = inputs(det, *r)
            capi.profile_enable(True)
            capi.profile_reset()
            for _ in range(args.reps):
                d, _ = fm.extract_features(inp, img, device_out=True)
            sync()
            groups[r].append(sum(v[0] for v in capi.profile_all().values() if v[1]) / args.reps)
            capi.profile_enable(False)
            found[r] = n_rows(d)
            t0 = time.perf_counter()   # (profiling off: the events of the launch sites are not in the host time)
            for _ in range(args.reps):
                fm.extract_features(inp, img, device_out=True)
            sync()
            host[r].append((time.perf_counter() - t0) * 1e3 / args.reps)
    for r in rows:
        g, hs = groups[r], host[r]
        name = "no key" if r[0] is None else f"{r[0]}={r[1]}"
        print(f"{det} {name}: {found[r]} rows, {statistics.median(g):.3f} ms in profiled kernels per view, range {min(g):.3f} .. {max(g):.3f}; "
              f"host time of the call {statistics.median(hs):.3f} ms, range {min(hs):.3f} .. {max(hs):.3f}", flush=True)
