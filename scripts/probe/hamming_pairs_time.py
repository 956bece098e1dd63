"""The batched Hamming matcher against the per-pair loop it replaces, on the FAST descriptors of a few 3840 x 2160 synthetic
views (a 3 x 2 grid, neighbours overlapping).  Both forms get the same resident sets; each is warmed up once and then timed
alternately over `reps` rounds with a host clock around calls that end in a device synchronise.  The lists are compared before
anything is timed.  Prints the wall times (median, min, max), the batched call's per-kernel times (aps_profile_*) and the
counts behind the claim: pairs, per-pair launch / synchronise / copy round trips, matches the host uniqueness loop walked.

    python scripts/probe/hamming_pairs_time.py [--levels 8] [--strongest 5000] [--batched-only]

--levels and --strongest set NumLevels and NumStrongest of the extraction (the sets grow with the pyramid and are cut by the
selection); --batched-only leaves the per-pair loop out (it is quadratic in rows too, and has nothing to add to such a figure)."""
import argparse
import statistics
import sys
import time
from importlib import import_module

import numpy as np

sys.path.insert(0, ".")
import apsamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, default=1)
ap.add_argument("--strongest", type=int, default=None)
ap.add_argument("--batched-only", action="store_true")
args = ap.parse_args()

fm = import_module(apsamd.__name__ + ".featureMatching")
synth = import_module(apsamd.__name__ + ".synth")
capi = apsamd._capi
import torch  # noqa: E402

W, H, f = 3840, 2160, 4000.0
RATIO, THR = 0.6, 20.0
cams = synth.grid_cameras(3, 2, W, H, f, 2 * np.arctan(W / (2 * f)) * 0.5, 2 * np.arctan(H / (2 * f)) * 0.5, 0.0, 5)
inp = {"detector": "FAST", "MinContrast": 0.08, "NumLevels": args.levels}  # (the synthetic world is smooth: the default 0.2 finds next to nothing)
if args.strongest is not None:
    inp["NumStrongest"] = args.strongest
descs = []
for cam in cams:
    img = synth.render_view(cam, H, W, 5, "cuda", finest_px=1.0)
    torch.cuda.synchronize()
    descs.append(fm.fast_extract(inp, img, device_out=True)[0])
n = len(descs)
pairs = fm.pair_order(n)


def per_pair():
    """The loop as it stood: one matchFeaturesScratch (search, synchronise, three copies, host filter) per pair."""
    out = [0]
    lists = []
    for (i, j) in pairs:
        m, d = fm.matchFeaturesScratch(descs[i], descs[j], MatchThreshold=THR, MaxRatio=RATIO, Unique=True)
        lists.append((m, d))
        out.append(out[-1] + len(m))
    return out, lists


def batched():
    return fm.match_pairwise_binary_csr(descs, RATIO, THR, True)


got = batched()   # warm-up of both, and the comparison
if args.batched_only:
    ptr0 = got[0].tolist()
else:
    ptr0, lists = per_pair()
    assert got[0].tolist() == ptr0
    assert np.array_equal(got[1], np.concatenate([m[:, 0] for m, _ in lists])) and np.array_equal(got[2], np.concatenate([m[:, 1] for m, _ in lists]))
    assert np.array_equal(got[3].view(np.uint32), np.concatenate([d for _, d in lists]).view(np.uint32))
reps = 7
t_loop, t_batch = [], []
for _ in range(reps):
    if not args.batched_only:
        t0 = time.perf_counter()
        per_pair()
        t_loop.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    batched()
    t_batch.append((time.perf_counter() - t0) * 1e3)
capi.profile_enable(True)
capi.profile_reset()
batched()
capi.check(capi.lib.aps_synchronize())
prof = {k: v for k, v in capi.profile_all().items() if v[1]}
capi.profile_enable(False)
rows = [len(d) for d in descs]
print(f"{n} views {W} x {H}, FAST features {rows}, {len(pairs)} pairs, {ptr0[-1]} matches (MaxRatio {RATIO}, MatchThreshold {THR})")
fmt = lambda t: f"median {statistics.median(t):9.2f} ms  min {min(t):9.2f}  max {max(t):9.2f}  ({reps} rounds, alternating)"  # noqa: E731
if not args.batched_only:
    print(f"per-pair loop : {fmt(t_loop)}   {len(pairs)} search launches, synchronises and 3-array copies; host uniqueness loop over {ptr0[-1]}+ rows")
print(f"batched call  : {fmt(t_batch)}   one launch chain, one read-back")
for k, (ms, cnt) in sorted(prof.items()):
    print(f"  {k:24s} {ms:8.3f} ms  ({cnt} launches)")
