"""Time of SIFT and SURF with NumStrongest (DESIGN.md "Strongest-N for SIFT and SURF") on 3840 x 2160 synthetic views, at several N
against the same views without the key.  Per detector and N it prints
  * the per-kernel time (aps_profile_*) of one view's extraction, one line per launch site, and the host time of the call (a clock
    around extractions that end in a synchronise: it includes the sort and the scans, which have no launch site of their own, and
    the read-backs); the total of each of --repeats groups of --reps extractions, whose spread is the noise of the figure - the
    groups of the rows alternate, so drift of the device shows as spread and not as a difference of rows;
  * the host time of match_pairs_csr over all pairs of 8 such views (4 x 2 grid, 40 % overlap).

--finest-px and --focal are the synthetic world's texture scale and the views' focal length (defaults: bench.py's 16 and 8000, about
20 k SIFT rows per view; --finest-px 1 gives a view with over 200 k rows, more than the wrapper's first capacity of H W / 64).

    python scripts/probe/strongest_time.py [--n 1000 5000 10000] [--reps 5] [--repeats 5] [--detectors SIFT SURF] [--finest-px 16]
"""
import argparse
import statistics
import sys
import time
from importlib import import_module

sys.path.insert(0, ".")
import apsamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[1000, 5000, 10000])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--detectors", nargs="+", default=["SIFT", "SURF"])
ap.add_argument("--finest-px", type=float, default=16.0)
ap.add_argument("--focal", type=float, default=8000.0)
args = ap.parse_args()

fm = import_module(apsamd.__name__ + ".featureMatching")
pl = import_module(apsamd.__name__ + ".pipeline")
synth = import_module(apsamd.__name__ + ".synth")
capi = apsamd._capi
W, H, f = 3840, 2160, args.focal
views, _ = synth.make_scene(4, 2, W, H, f, 0.4, seed=5, device="cuda", finest_px=args.finest_px)
import torch  # noqa: E402

torch.cuda.synchronize()
img = views[0]


def inputs(det, N):
    inp = pl.default_input(detector=det)
    return inp if N is None else {**inp, "NumStrongest": N}


def sync():
    capi.check(capi.lib.aps_synchronize())
    torch.cuda.synchronize()


for det in args.detectors:
    rows = [None] + list(args.n)
    for N in rows:
        fm.extract_features(inputs(det, N), img, device_out=True)  # warm-up: workspaces, code objects
    sync()
    groups, host, last, found = {N: [] for N in rows}, {N: [] for N in rows}, {}, {}
    for _ in range(args.repeats):
        for N in rows:
            capi.profile_enable(True)
            capi.profile_reset()
            for _ in range(args.reps):
                d, _ = fm.extract_features(inputs(det, N), img, device_out=True)
            sync()
            last[N] = {k: v for k, v in capi.profile_all().items() if v[1]}
            capi.profile_enable(False)
            found[N] = len(d)
            groups[N].append(sum(v[0] for v in last[N].values()) / args.reps)
            t0 = time.perf_counter()   # (profiling off: the events of the launch sites are not in the host time)
            for _ in range(args.reps):
                fm.extract_features(inputs(det, N), img, device_out=True)
            sync()
            host[N].append((time.perf_counter() - t0) * 1e3 / args.reps)
    for N in rows:
        g, hs = groups[N], host[N]
        name = "no NumStrongest" if N is None else f"NumStrongest={N}"
        print(f"{det} {name}: {found[N]} rows, {statistics.median(g):.3f} ms in profiled kernels per view, range {min(g):.3f} .. {max(g):.3f}; "
              f"host time of the call {statistics.median(hs):.3f} ms, range {min(hs):.3f} .. {max(hs):.3f}")
        for k, (ms, n) in sorted(last[N].items()):  # (the last group)
            print(f"  {k:20s} {ms / args.reps:8.3f} ms  ({n / args.reps:g} launches)")
    # matching: all pairs of the 8 views
    order = fm.pair_order(len(views))
    for N in rows:
        inp = inputs(det, N)
        descs = [fm.extract_features(inp, v, device_out=True)[0] for v in views]
        sync()
        fm.match_pairs_csr(descs, order, inp["Ratiothreshold"], inp["Matchingthreshold"], True)  # warm-up
        sync()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            m = fm.match_pairs_csr(descs, order, inp["Ratiothreshold"], inp["Matchingthreshold"], True)
            sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        name = "no NumStrongest" if N is None else f"NumStrongest={N}"
        print(f"{det} {name}: match_pairs_csr over {len(order)} pairs of {len(views)} views, rows per view "
              f"{min(len(d) for d in descs)} .. {max(len(d) for d in descs)}, {int(m[0][-1])} matches: "
              f"{statistics.median(ts):.2f} ms, range {min(ts):.2f} .. {max(ts):.2f}")
