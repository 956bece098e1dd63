"""The KAZE selection keys and Upright through the routes that hand `input` on: the whole stitch with and without intrinsics,
matching and RANSAC on the frozen pair, the pipeline's extraction dispatch on the worker threads and the distributed driver."""
from importlib import import_module

import numpy as np
import pytest

import kaze_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(gpu):
    return {k: import_module(gpu.__name__ + "." + k) for k in ("featureMatching", "imageMatching", "pipeline", "parallel", "synth")}


def _scene(mods):
    """kaze_cases.SCENE (test_kaze_pipeline_gpu._scene): about 1400 keypoints per view without a selection."""
    import torch

    views, cams = kc.scene(mods["synth"], "cuda")
    torch.cuda.synchronize()
    return views, [c["K"] for c in cams]


def test_stitch_end_to_end_with_uniform_rows_and_upright(mods):
    """info['n_features'] is the length of every view's keypoint list (info['keypoints'] with showKeypointsPlot): 300 of the views'
    1400 rows."""
    pl = mods["pipeline"]
    views, Ks = _scene(mods)
    inp = pl.default_input(detector="KAZE", resizeImage=0, NumUniform=300, Upright=True)
    for kw in ({"Ks": Ks}, {}):
        panos, info = pl.stitch(inp, views, tile=(512, 512), **kw)
        assert info["n_features"] == [300, 300], info["n_features"]
        assert info["n_components"] == 1 and len(panos) == 1 and sorted(info["components"][0]["members"]) == [0, 1]
        pano = panos[0].cpu().numpy() if hasattr(panos[0], "cpu") else np.asarray(panos[0])
        assert (pano.max(axis=2) > 0).mean() > 0.5
        assert ("ba" in info) == (not kw)
    plain = pl.stitch(pl.default_input(detector="KAZE", resizeImage=0), views, Ks=Ks, tile=(512, 512))[1]
    assert min(plain["n_features"]) > 1000, "without the keys the views keep all their rows"


def test_ransac_recovers_the_known_homography_from_upright_rows(mods):
    """test_kaze_pipeline_gpu.test_ransac_recovers_the_known_homography with Upright = True, through match_and_verify: the four image
    corners within 5.5 px of PAIR_H's (the maxDistance that test uses)."""
    fm, pl = mods["featureMatching"], mods["pipeline"]
    A, B = kc.pair()
    inp = pl.default_input(detector="KAZE", Upright=True, maxDistance=5.5, inliersConfidence=99.9, maxIter=500)
    feats = [fm.kaze_extract(inp, x) for x in (A, B)]
    oriented = [fm.kaze_extract(pl.default_input(detector="KAZE"), x) for x in (A, B)]
    assert [len(f[0]) for f in feats] == [len(f[0]) for f in oriented] == [1090, 1082]
    assert not np.array_equal(feats[0][0], oriented[0][0])
    res = pl.match_and_verify(inp, [f[0] for f in feats], [f[1] for f in feats], seed=1)
    assert [tuple(p) for p in res["pairs"]] == [(0, 1)]
    H = np.asarray(res["models"][0], np.float64)   # j -> i on 1-based [x y 1] columns: B's corners onto A's
    corners = np.array([[1, 1], [320, 1], [1, 240], [320, 240]], np.float64)
    want = np.concatenate([corners - 1.0, np.ones((4, 1))], 1) @ np.linalg.inv(kc.PAIR_H).T
    want = want[:, :2] / want[:, 2:] + 1.0
    got = np.concatenate([corners, np.ones((4, 1))], 1) @ H.T
    err = np.hypot(*(got[:, :2] / got[:, 2:] - want).T)
    print("upright: %d putative matches, %d inliers, corner errors %s" % (int(res["putative"][0, 1]), len(res["inliers"][0]), np.round(err, 3)))
    assert err.max() <= 5.5, err


def test_sift_submit_dispatches_the_keys_on_the_worker_threads(mods):
    import torch

    fm, pl = mods["featureMatching"], mods["pipeline"]
    views = [kc.band_limited(20 + k, 200, 260, 2.5, channels=3) for k in range(4)]
    for keys in ({"NumStrongest": 60}, {"NumUniform": 60, "UniformGrid": (4, 6), "Upright": True}):
        inp = pl.default_input(detector="KAZE", **keys)
        for fu, v in zip(pl.sift_submit(inp, views), views):
            d, p = fu.result()
            d0, p0 = fm.kaze_extract(inp, v)
            assert d.shape == (60, 64) and np.array_equal(d.view(np.uint8), d0.view(np.uint8)) and np.array_equal(p.view(np.uint8), p0.view(np.uint8))
            assert len(fm.kaze_extract(pl.default_input(detector="KAZE"), v)[0]) > 60
        resident = [torch.from_numpy(v).cuda() for v in views[:2]]
        descs, kps = pl.extract_features(inp, resident)
        for d, v in zip(descs, views):
            assert tuple(d.shape) == (60, 128) and np.array_equal(d[:, :64].cpu().numpy().view(np.uint8), fm.kaze_extract(inp, v)[0].view(np.uint8))


def test_one_rank_distributed_run_with_numstrongest_equals_the_single_process_driver(mods):
    pl, par = mods["pipeline"], mods["parallel"]
    views, Ks = _scene(mods)
    inp = pl.default_input(detector="KAZE", resizeImage=0, NumStrongest=200)
    pano, info = par.stitch_distributed(inp, dict(enumerate(views)), 2, Ks, (512, 512))
    panos, i2 = pl.stitch(inp, views, Ks=Ks, tile=(512, 512))
    assert info["n_components"] == 1 and i2["n_components"] == 1 and len(panos) == 1
    assert list(info["n_features"]) == [200, 200] and i2["n_features"] == [200, 200]
    assert tuple(pano.shape) == tuple(panos[0].shape) and np.array_equal(pano.cpu().numpy(), panos[0].cpu().numpy())
