"""Time of SURF and FAST feature extraction in groups of views against the per-view route of another checkout, on 64 resident
3840 x 2160 synthetic views (bench.py's 8 x 8 grid of cameras, over a dense texture by default: on bench.py's own world SURF finds
a handful of rows per view and FAST none) through pipeline.sift_many.  Rows: SURF at defaults, SURF with NumStrongest = --n
(5000), FAST with NumLevels = 3 (MinContrast 0.08: the synthetic world is smooth).  Routes of a row: `per-view` =
the yardstick, pipeline.sift_many of the package under --baseline (a checkout of the parent commit, built; without it, this
checkout with a group size of 0, which is NOT the yardstick and is labelled so); `VxW` = this checkout with groups of V views on
W workers.  After --warmup passes per route, --series series of --passes passes each; a pass is timed on the host clock from the
call to the return of sift_many, which ends with every worker's stream synchronised.  The series of a row's routes alternate
(round-robin), so drift of the device shows as spread and not as a difference of routes.  Every route keeps its own worker pool
for the whole run, so no pass pays for a pool's start.  Prints, per row and route, the median ms per pass of every series, and
one JSON line with all of them.

    python scripts/probe/feature_groups_time.py --baseline ../parent [--settings 4x2 8x3 16x4 ...] [--rows surf fast3] [--grid 8x8]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time
from importlib import import_module

import numpy as np

sys.path.insert(0, ".")
import apsamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--baseline", default=None, help="root of a built checkout of the parent commit: its per-view route is the yardstick")
ap.add_argument("--settings", nargs="+", default=["%dx%d" % (v, w) for v in (4, 8, 16) for w in (2, 3, 4)], help="views x workers")
ap.add_argument("--rows", nargs="+", default=["surf", "surf-strongest", "fast3"])
ap.add_argument("--grid", default="8x8", help="views of the scene, columns x rows")
ap.add_argument("--size", default="3840x2160")
ap.add_argument("--finest-px", type=float, default=1.0, help="finest texture period of the synthetic world (bench.py: 16, where SURF "
                "finds a handful of rows per view and FAST none)")
ap.add_argument("--focal", type=float, default=4000.0, help="focal length at 3840 px width (bench.py: 8000)")
ap.add_argument("--n", type=int, default=5000, help="NumStrongest of the surf-strongest row")
ap.add_argument("--series", type=int, default=3)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

import torch  # noqa: E402

synth = import_module(apsamd.__name__ + ".synth")
pl = import_module(apsamd.__name__ + ".pipeline")
capi = apsamd._capi
base_pl, base_capi = None, None
if args.baseline:
    # the other checkout's package under a name of its own: its modules, its library, its worker pools
    pkg_dir = os.path.join(os.path.abspath(args.baseline), apsamd.__name__)
    spec = importlib.util.spec_from_file_location("aps_baseline", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    base = importlib.util.module_from_spec(spec)
    sys.modules["aps_baseline"] = base
    spec.loader.exec_module(base)
    base_pl, base_capi = import_module("aps_baseline.pipeline"), import_module("aps_baseline._capi")
    assert os.path.samefile(os.path.dirname(base_capi.LIB_PATH), os.path.join(pkg_dir, "lib")), base_capi.LIB_PATH

nx, ny = (int(v) for v in args.grid.lower().split("x"))
w, h = (int(v) for v in args.size.lower().split("x"))
OVERLAP = 0.4   # bench.py's grid of cameras over the dense texture of strongest_time.py's second table (--finest-px 1 --focal 4000)
f = args.focal * w / 3840
cams = synth.grid_cameras(nx, ny, w, h, f, 2 * np.arctan(w / (2 * f)) * (1 - OVERLAP), 2 * np.arctan(h / (2 * f)) * (1 - OVERLAP), 1.0, 12345)
views = [synth.render_view(c, h, w, 12345, "cuda", finest_px=args.finest_px) for c in cams]
torch.cuda.synchronize()
ROWS = {"surf": {"detector": "SURF"}, "surf-strongest": {"detector": "SURF", "NumStrongest": args.n},
        "fast3": {"detector": "FAST", "NumLevels": 3, "MinContrast": 0.08}}
PER_VIEW = "per-view" if base_pl else "per-view (this checkout: not the yardstick)"
pools = {}   # (detector, route) -> this checkout's group pool of that route


def one_pass(inp, route):
    det = inp["detector"]
    if route == PER_VIEW and base_pl:
        run, sync = base_pl.sift_many, base_capi
    else:
        v, k = (0, 1) if route == PER_VIEW else (int(x) for x in route.split("x"))
        setattr(pl, det + "_GROUP_VIEWS", v)
        setattr(pl, det + "_GROUP_WORKERS", k)
        if (det, route) in pools:
            pl._GROUP_POOLS[det] = pools[det, route]
        else:
            pl._GROUP_POOLS.pop(det, None)
        run, sync = pl.sift_many, capi
    sync.check(sync.lib.aps_synchronize())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(pl.default_input(**inp), views)
    sync.check(sync.lib.aps_synchronize())
    ms = (time.perf_counter() - t0) * 1e3
    if det in pl._GROUP_POOLS and run is pl.sift_many:
        pools[det, route] = pl._GROUP_POOLS[det]
    return ms, [len(p) for _, p in out]


result = {}
for row in args.rows:
    inp, routes = ROWS[row], [PER_VIEW] + list(args.settings)
    found = {}
    for route in routes:
        for _ in range(args.warmup):   # code objects, workspaces, the worker pools
            found[route] = one_pass(inp, route)[1]
    assert all(found[r] == found[PER_VIEW] for r in routes), "the routes disagree on the rows per view"
    series = {r: [] for r in routes}
    for _ in range(args.series):
        for route in routes:
            series[route].append(statistics.median(one_pass(inp, route)[0] for _ in range(args.passes)))
    print(f"{row}: {len(views)} views of {w} x {h}, {sum(found[PER_VIEW])} rows in all; ms per extraction pass, median of {args.passes} passes per series")
    for route in routes:
        s = series[route]
        print(f"  {route:12s} median {statistics.median(s):8.2f}  range {min(s):8.2f} .. {max(s):8.2f}  ({' '.join('%.2f' % v for v in s)})")
    result[row] = series
print(json.dumps({"feature_groups_time": result}))
