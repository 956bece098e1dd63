"""GPU: parallel.stitch_distributed without intrinsics.  The cameras are estimated per connected component on the rank that
owns the component and broadcast; the result must be the single-process driver's (pipeline.stitch), must not depend on the
number of ranks, and planar sets must render through the planar compositor.  With intrinsics nothing new may run.
Multi-rank runs: fresh children from torch.multiprocessing's spawn context, gloo, both ranks on GPU 0 (at most the test
process and two children alive); a child that fails ends the test."""
import os
import socket
import sys
from importlib import import_module

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, F = 640, 480, 900.0
CAMERA_FIELDS = ("K", "R", "f", "noRotation", "H2refined")
BA_NOT_COMPARED = ("owner", "seconds")  # who estimated the component and how long it took


def _mods(pkg):
    return {k: import_module(pkg.__name__ + "." + k) for k in ("synth", "pipeline", "parallel")}


_SCENES = {}


def _scenario(mode, synth):
    """(views on the device, input, tile, RANSAC seed) - each scene the smallest that reaches its branch; rendered once per
    process and never written to."""
    if mode not in _SCENES:
        _SCENES[mode] = _render_scenario(mode, synth)
    return _SCENES[mode]


def _render_scenario(mode, synth):
    import torch

    pl = import_module(synth.__name__.rsplit(".", 1)[0] + ".pipeline")
    if mode == "pair":  # the 2 x 1 scene of tests/test_surf_pipeline_gpu.py, with SIFT
        from test_surf_pipeline_gpu import _scene

        views, _ = _scene({"synth": synth})
        out = views, pl.default_input(), (512, 512), 0
    elif mode == "grid":  # one component of six: tiles sharded
        cams = synth.grid_cameras(3, 2, W, H, F, 2 * np.arctan(W / (2 * F)) * 0.6, 2 * np.arctan(H / (2 * F)) * 0.6, 1.0, 7)
        out = [synth.render_view(c, H, W, 7, "cuda", finest_px=6.0) for c in cams], pl.default_input(bands=3), (256, 256), 0
    elif mode == "worlds":  # components of 4, 4 and 6: estimation and render sharded by component
        from test_components_gpu import _worlds

        out = _worlds(synth)[0], pl.default_input(bands=3), (256, 256), 0
    elif mode == "planar":  # the 3 x 2 grid of DESIGN.md "Planar sets"
        views, _ = synth.make_scene(3, 2, W, H, F, overlap=0.35, seed=31, device="cuda", finest_px=3.0, gains=True)
        out = views, pl.default_input(bands=2, forcePlanarScan=True, planarBundleAdjustment=True), (1024, 1024), 1
    else:
        raise ValueError(mode)
    torch.cuda.synchronize()
    return out


def _record(info):
    """What the runs are compared on, as host data (it crosses a process boundary)."""
    return {"pairs": [tuple(p) for p in info["pairs"]], "models": [np.asarray(m, np.float64).copy() for m in info["models"]],
            "members": [list(c["members"]) for c in info["components"]], "refs": [int(c["ref"]) for c in info["components"]],
            "cameras": [None if c is None else {k: np.asarray(c[k], np.float64).copy() for k in CAMERA_FIELDS if k in c}
                        for c in info["cameras"]],
            "ba": [dict(d) for d in info.get("ba", [])], "times": dict(info["times"]),
            "panos": [p.cpu().numpy() for p in info["panoramas"]]}


def _distributed(mods, mode, world=1, rank=0, **kw):
    import torch

    views, inp, tile, seed = _scenario(mode, mods["synth"])
    par = mods["parallel"]
    n = len(views)
    local = {i: views[i] for i in par.shard_indices(n, world, rank)}
    _, info = par.stitch_distributed(inp, local, n, None, tile, seed, pano_root=0, **kw)
    torch.cuda.synchronize()
    return info


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, q, mode):
    try:
        sys.path.insert(0, ROOT)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["APS_DEVICE"] = "0"
        import torch
        import torch.distributed as dist

        torch.cuda.set_device(0)
        if mode == "counts":
            os.environ["APS_PARALLEL_FORCE_COLLECTIVES"] = "1"
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import apsamd

        mods = _mods(apsamd)
        if mode == "counts":
            out = _count_collectives(mods)
        else:
            info = _distributed(mods, mode, world, rank)
            out = _record(info) if rank == 0 else None  # (pano_root = 0: the other rank holds only what it rendered itself)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", out if rank == 0 else None))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, traceback.format_exc(), None))
        raise


def _spawn(world, mode):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q, mode)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    for _ in procs:
        res.append(q.get(timeout=600))
        if res[-1][1] != "ok":
            break  # the other rank is waiting for this one in a collective: do not wait for it
    for p in procs:
        if any(r[1] != "ok" for r in res):
            p.terminate()
        p.join(timeout=120)
    assert all(r[1] == "ok" for r in res), [r[1] for r in res if r[1] != "ok"]
    return next(r[2] for r in res if r[0] == 0)


_ONE_RANK = {}


def _one_rank(gpu, mode):
    """The one-rank run of a scene (this process, no process group), computed once and shared."""
    if mode not in _ONE_RANK:
        _ONE_RANK[mode] = _record(_distributed(_mods(gpu), mode))
    return _ONE_RANK[mode]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _assert_same_matching(a, b, what):
    msg = "RANSAC differs between %s: not the camera estimation" % what
    assert a["pairs"] == b["pairs"], msg
    assert len(a["models"]) == len(b["models"])
    for x, y in zip(a["models"], b["models"]):
        assert np.array_equal(_bits(x), _bits(y)), msg


def _assert_same_cameras(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), k
        if x is not None:
            assert sorted(x) == sorted(y), k
            for f in x:
                assert np.array_equal(_bits(x[f]), _bits(y[f])), (k, f)


def _assert_same_value(x, y, where):
    if isinstance(x, float) or isinstance(y, float):
        assert x is not None and y is not None and np.array_equal(_bits(x), _bits(y)), where
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), where
        for u, v in zip(x, y):
            _assert_same_value(u, v, where)
    else:
        assert x == y, where


def _assert_same_panoramas(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and np.array_equal(x, y)


def test_one_rank_equals_the_single_process_driver(gpu):
    mods = _mods(gpu)
    pl, par = mods["pipeline"], mods["parallel"]
    views, inp, tile, _ = _scenario("pair", mods["synth"])
    pano, info = par.stitch_distributed(inp, dict(enumerate(views)), 2, None, (512, 512))
    panos, i2 = pl.stitch(inp, views, tile=(512, 512))
    got = _record(info)
    _assert_same_matching(got, {"pairs": i2["result"]["pairs"], "models": i2["result"]["models"]}, "the two drivers")
    assert len(got["pairs"]) == 1 and len(info["ba"]) == len(i2["ba"]) == 1 and len(panos) == 1
    for k in range(2):
        for f in ("K", "R"):
            assert np.array_equal(_bits(info["cameras"][k][f]), _bits(i2["cameras"][k][f])), (k, f)
    for key in ("focals", "rmse_init", "rmse_final", "evaluations"):
        _assert_same_value(info["ba"][0][key], i2["ba"][0][key], key)
    assert info["ba"][0]["evaluations"] > 0 and info["ba"][0]["owner"] == 0 and info["ba"][0]["members"] == [0, 1]
    assert "bundle_adjustment" in info["times"] and "host_cameras" not in info["times"]
    assert tuple(pano.shape) == tuple(panos[0].shape) and np.array_equal(pano.cpu().numpy(), panos[0].cpu().numpy())


@pytest.mark.parametrize("mode", ["grid", "worlds"])
def test_two_ranks_equal_one_rank(gpu, mode):
    one = _one_rank(gpu, mode)
    two = _spawn(2, mode)
    _assert_same_matching(one, two, "one and two ranks")
    assert len(one["pairs"]) >= 5
    assert one["members"] == two["members"] and one["refs"] == two["refs"]
    assert len(one["panos"]) == (3 if mode == "worlds" else 1)
    _assert_same_cameras(one["cameras"], two["cameras"])
    assert len(one["ba"]) == len(two["ba"]) == len(one["panos"])
    for a, b in zip(one["ba"], two["ba"]):
        assert sorted(a) == sorted(b)
        for key in a:
            if key not in BA_NOT_COMPARED:
                _assert_same_value(a[key], b[key], key)
        assert a["evaluations"] > 0
    _assert_same_panoramas(one["panos"], two["panos"])
    assert {d["owner"] for d in one["ba"]} == {0}
    if mode == "worlds":
        assert {d["owner"] for d in two["ba"]} == {0, 1}
    print("%s: times['bundle_adjustment'] one rank %.3f s, two ranks on one GPU %.3f s; per component (members, s, evaluations) "
          "one rank %s, two ranks %s" % (mode, one["times"]["bundle_adjustment"], two["times"]["bundle_adjustment"],
                                         [(len(d["members"]), round(d["seconds"], 3), d["evaluations"]) for d in one["ba"]],
                                         [(len(d["members"]), round(d["seconds"], 3), d["evaluations"], d["owner"]) for d in two["ba"]]))


def test_three_worlds_equal_each_world_alone(gpu):
    """Every component's cameras and panorama from the three-worlds run equal those of stitch_distributed on that world's
    views alone (one rank, no intrinsics).  The figures are printed for every world before anything is asserted.
    It holds because the RANSAC draws of a pair are keyed by its position among the candidate pairs of its own connected set
    of the candidate graph (parallel.candidate_keys), not by its position in the whole collection: keyed that way, 3 of the
    23 verified models of this scene differed in bits between the two runs, focals by up to 8e-4 relative, rotations by up
    to 0.012 deg and 1-3 % of the panorama bytes."""
    import torch

    mods = _mods(gpu)
    par = mods["parallel"]
    views, inp, tile, seed = _scenario("worlds", mods["synth"])
    allw = _one_rank(gpu, "worlds")
    assert sorted(len(m) for m in allw["members"]) == [4, 4, 6]
    alone = []
    for ci, members in enumerate(allw["members"]):
        sub = {q: views[k] for q, k in enumerate(members)}
        pano, ia = par.stitch_distributed(inp, sub, len(members), None, tile, seed, pano_root=0)
        torch.cuda.synchronize()
        ra = _record(ia)
        alone.append((ia["n_components"], ra))
        loc = {k: q for q, k in enumerate(members)}
        big = {(loc[i], loc[j]): m for (i, j), m in zip(allw["pairs"], allw["models"]) if i in loc and j in loc}
        small = dict(zip(ra["pairs"], ra["models"]))
        differ = [ij for ij in sorted(big) if ij not in small or not np.array_equal(_bits(big[ij]), _bits(small[ij]))]
        df = max(abs(float(allw["cameras"][k]["f"]) / float(ra["cameras"][q]["f"]) - 1) for q, k in enumerate(members))
        dr = max(float(np.degrees(np.arccos(np.clip((np.trace(allw["cameras"][k]["R"] @ ra["cameras"][q]["R"].T) - 1) / 2, -1, 1))))
                 for q, k in enumerate(members))
        a, b = allw["panos"][ci], ra["panos"][0]
        px = ("shape %s against %s" % (a.shape, b.shape) if a.shape != b.shape else
              "%.2f %% of the bytes differ, by %d at most" % (100.0 * float((a != b).mean()), int(np.abs(a.astype(int) - b).max())))
        print("world %d (%d views): %d of %d RANSAC models differ in bits; focal differs by %.2e (relative), rotations by "
              "%.2e deg at most; panorama: %s" % (ci, len(members), len(differ), len(big), df, dr, px))
    for ci, members in enumerate(allw["members"]):
        ncomp, ra = alone[ci]
        assert ncomp == 1 and ra["members"] == [list(range(len(members)))] and ra["refs"] == [allw["refs"][ci]]
        _assert_same_cameras([allw["cameras"][k] for k in members], ra["cameras"])
        _assert_same_panoramas([allw["panos"][ci]], ra["panos"])
        assert (ra["panos"][0].max(axis=2) > 0).mean() > 0.5


def test_planar_set_one_rank_equals_the_single_process_driver(gpu):
    import torch

    mods = _mods(gpu)
    views, inp, tile, seed = _scenario("planar", mods["synth"])
    panos, i2 = mods["pipeline"].stitch(inp, views, tile=tile, seed=seed)
    torch.cuda.synchronize()
    one = _one_rank(gpu, "planar")
    _assert_same_matching(one, {"pairs": i2["result"]["pairs"], "models": i2["result"]["models"]}, "the two drivers")
    assert len(panos) == 1 and one["members"] == [list(range(6))]
    st = one["ba"][0]
    assert st["noRotation"] == 1 and st["evaluations"] > 0 and st["rmse_final"] <= st["rmse_init"]
    assert all(int(c["noRotation"]) == 1 and "H2refined" in c for c in one["cameras"])
    _assert_same_cameras(one["cameras"], [{k: c[k] for k in CAMERA_FIELDS if k in c} for c in i2["cameras"]])
    _assert_same_panoramas(one["panos"], [panos[0].cpu().numpy()])


def test_planar_set_two_ranks_equal_one_rank(gpu):
    one = _one_rank(gpu, "planar")
    two = _spawn(2, "planar")
    _assert_same_matching(one, two, "one and two ranks")
    _assert_same_cameras(one["cameras"], two["cameras"])
    for a, b in zip(one["ba"], two["ba"]):
        for key in a:
            if key not in BA_NOT_COMPARED:
                _assert_same_value(a[key], b[key], key)
    _assert_same_panoramas(one["panos"], two["panos"])


def test_planar_cameras_passed_back_render_the_same_bytes(gpu):
    """cameras = the estimated planar cameras: no estimation, the planar compositor, the same panorama."""
    import torch

    mods = _mods(gpu)
    views, inp, tile, seed = _scenario("planar", mods["synth"])
    one = _one_rank(gpu, "planar")
    cams = [{k: (int(v) if k == "noRotation" else float(v) if k == "f" else v) for k, v in c.items()} for c in one["cameras"]]
    back, ib = mods["parallel"].stitch_distributed(inp, dict(enumerate(views)), 6, None, tile, seed, cams, pano_root=0)
    torch.cuda.synchronize()
    assert "ba" not in ib and "bundle_adjustment" not in ib["times"]
    _assert_same_panoramas(one["panos"], [back.cpu().numpy()])


def test_second_pass_estimates_from_the_second_pass(gpu):
    """resizeImage and resizeImagePanoramaCluster with three worlds of three sizes (tests/test_components_gpu.py): the images
    are resized per component and matched again, and the estimate must use THAT pass's keypoints, inliers and image sizes:
    the cameras and panoramas are those of a plain run on images resized that way beforehand."""
    import torch
    from test_components_gpu import _worlds_of_three_sizes

    mods = _mods(gpu)
    pl, par = mods["pipeline"], mods["parallel"]
    originals, _, _ = _worlds_of_three_sizes(mods["synth"])
    torch.cuda.synchronize()
    n = len(originals)
    hw_o = [(int(v.shape[0]), int(v.shape[1])) for v in originals]
    inp = pl.default_input(bands=3, resizeImage=1, resizeImagePanoramaCluster=1, heightLimit=480, widthLimit=480)
    first = pl.resize_per_component(inp, dict(enumerate(originals)), np.zeros(n, np.int64), hw_o)
    _, info = par.stitch_distributed(inp, first, n, None, (256, 256), 0, None, pano_root=0,
                                     local_originals=dict(enumerate(originals)))
    torch.cuda.synchronize()
    assert info["second_pass"] is True and info["n_components"] == 3 and len(info["ba"]) == 3
    assert list(info["n_features"]) != list(info["n_features_first_pass"])
    pre = pl.resize_per_component(inp, dict(enumerate(originals)), np.asarray(info["labels"]), hw_o)
    assert len({tuple(v.shape) for v in pre.values()}) == 3  # every world kept its own aspect
    _, plain = par.stitch_distributed(pl.default_input(bands=3), pre, n, None, (256, 256), 0, None, pano_root=0)
    torch.cuda.synchronize()
    assert plain["second_pass"] is False
    got, want = _record(info), _record(plain)
    _assert_same_matching(got, want, "the second pass and the plain run")
    assert got["members"] == want["members"] and got["refs"] == want["refs"]
    _assert_same_cameras(got["cameras"], want["cameras"])
    _assert_same_panoramas(got["panos"], want["panos"])


def _count_collectives(mods):
    """In a gloo group of one with APS_PARALLEL_FORCE_COLLECTIVES=1 (every collective of the multi-rank driver runs): calls of
    allgather_ragged and _broadcast, and the keys of _match_pass' result, with and without intrinsics on the 3 x 2 grid."""
    import torch

    par, synth = mods["parallel"], mods["synth"]
    assert par._multi(1)
    cams = synth.grid_cameras(3, 2, W, H, F, 2 * np.arctan(W / (2 * F)) * 0.6, 2 * np.arctan(H / (2 * F)) * 0.6, 1.0, 7)
    views, inp, tile, seed = _scenario("grid", synth)
    calls = {"allgather_ragged": 0, "_broadcast": 0, "_match_pass": 0}
    keys = []
    real = {k: getattr(par, k) for k in calls}

    def wrap(name):
        def f(*a, **kw):
            calls[name] += 1
            out = real[name](*a, **kw)
            if name == "_match_pass":
                keys.append(sorted(out))
            return out
        return f

    for k in calls:
        setattr(par, k, wrap(k))
    out = {}
    try:
        for tag, Ks in (("Ks", [c["K"] for c in cams]), ("estimated", None)):
            for k in calls:
                calls[k] = 0
            del keys[:]
            _, info = par.stitch_distributed(inp, dict(enumerate(views)), 6, Ks, tile, seed, pano_root=0)
            torch.cuda.synchronize()
            out[tag] = {"calls": dict(calls), "keys": list(keys[-1]), "ncomp": len(info["components"]), "ba": "ba" in info,
                        "times": sorted(info["times"])}
    finally:
        for k in calls:
            setattr(par, k, real[k])
    return out


def test_nothing_new_runs_with_intrinsics(gpu):
    """The parent commit's driver, read off its code for this run (pairwise matcher, one match pass, pano_root = 0, no gain
    compensation): allgather_ragged once per match pass (the match lists), _broadcast once per component (the panorama's
    shape in _deliver_panorama; the owner is the root).  With Ks exactly that; without, one more of each."""
    got = _spawn(1, "counts")
    k, e = got["Ks"], got["estimated"]
    assert k["ncomp"] == e["ncomp"] == 1 and k["calls"]["_match_pass"] == e["calls"]["_match_pass"] == 1
    assert k["calls"]["allgather_ragged"] == 1 and k["calls"]["_broadcast"] == 1
    assert "inliers" not in k["keys"] and "keypoints" not in k["keys"] and not k["ba"]
    assert "host_cameras" in k["times"] and "bundle_adjustment" not in k["times"]
    # the wrappers do count what the new path calls: the inlier all-gather and one broadcast per component
    assert e["calls"]["allgather_ragged"] == 2 and e["calls"]["_broadcast"] == 2
    assert "inliers" in e["keys"] and "keypoints" in e["keys"] and e["ba"]
    assert "bundle_adjustment" in e["times"] and "host_cameras" not in e["times"]
