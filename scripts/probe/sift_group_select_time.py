"""Time of the feature extraction with a per-view selection on the bench scene: 64 resident 3840 x 2160 synthetic views (bench.py's
8 x 8 grid) through pipeline.sift_many with NumStrongest = N and with NumUniform = N on the default grid.  After --warmup passes per
row, --series series of --passes passes each; a pass is timed on the host clock from the call to the return of sift_many, which
ends with every worker's stream synchronised.  Prints, per row, the median ms per pass of every series, and the median and min-max
of those.  The series of the two rows alternate, so drift of the device shows as spread and not as a difference of rows.

The script uses public entries only, so the same file run from a checkout of another commit times that commit: before the grouped
selection (aps_sift_extract_batch_strongest / _uniform) the same calls take the per-view path.

    python scripts/probe/sift_group_select_time.py [--n 5000] [--grid 8x8] [--series 3] [--passes 7] [--warmup 2]
"""
import argparse
import json
import statistics
import sys
import time
from importlib import import_module

import numpy as np

sys.path.insert(0, ".")
import apsamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=5000)
ap.add_argument("--grid", default="8x8", help="views of the scene, columns x rows")
ap.add_argument("--size", default="3840x2160")
ap.add_argument("--series", type=int, default=3)
ap.add_argument("--passes", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

import torch  # noqa: E402

synth = import_module(apsamd.__name__ + ".synth")
pl = import_module(apsamd.__name__ + ".pipeline")
capi = apsamd._capi
nx, ny = (int(v) for v in args.grid.lower().split("x"))
w, h = (int(v) for v in args.size.lower().split("x"))
OVERLAP, FINEST_PX, FOCAL = 0.4, 16.0, 8000.0   # bench.py's scene
f = FOCAL * w / 3840
cams = synth.grid_cameras(nx, ny, w, h, f, 2 * np.arctan(w / (2 * f)) * (1 - OVERLAP), 2 * np.arctan(h / (2 * f)) * (1 - OVERLAP), 1.0, 12345)
views = [synth.render_view(c, h, w, 12345, "cuda", finest_px=FINEST_PX) for c in cams]
torch.cuda.synchronize()
rows = {"NumStrongest": pl.default_input(NumStrongest=args.n), "NumUniform": pl.default_input(NumUniform=args.n)}


def one_pass(inp):
    capi.check(capi.lib.aps_synchronize())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = pl.sift_many(inp, views)
    capi.check(capi.lib.aps_synchronize())
    ms = (time.perf_counter() - t0) * 1e3
    return ms, [int(d.shape[0]) for d, _ in out]


found = {}
for name, inp in rows.items():
    for _ in range(args.warmup):   # code objects, workspaces, the worker pools
        _, found[name] = one_pass(inp)
series = {name: [] for name in rows}
for _ in range(args.series):
    for name, inp in rows.items():
        series[name].append(statistics.median(one_pass(inp)[0] for _ in range(args.passes)))
for name in rows:
    s = series[name]
    n_rows = found[name]
    print(json.dumps({"row": f"{name}={args.n}", "views": len(views), "size": [w, h], "rows_per_view": [min(n_rows), max(n_rows)],
                      "median_ms_per_pass": round(statistics.median(s), 3), "min_ms": round(min(s), 3), "max_ms": round(max(s), 3),
                      "series_ms": [round(v, 3) for v in s], "passes_per_series": args.passes, "warmup_passes": args.warmup}))
