"""KAZE through the operators behind feature extraction: the matchers on 64-wide rows, RANSAC on the frozen pair, the whole
stitch with and without intrinsics, the pipeline's extraction dispatch on the worker threads and the distributed driver."""
from importlib import import_module

import numpy as np
import pytest

import kaze_cases as kc

pytestmark = pytest.mark.gpu
KAZE = {"detector": "KAZE"}


@pytest.fixture(scope="module")
def mods(gpu):
    return {k: import_module(gpu.__name__ + "." + k) for k in ("featureMatching", "imageMatching", "pipeline", "parallel", "synth")}


@pytest.fixture(scope="module")
def pair_features(mods):
    """Device features of the frozen pair (host arrays), computed once."""
    fm = mods["featureMatching"]
    A, B = kc.pair()
    return fm.kaze_extract(KAZE, A), fm.kaze_extract(KAZE, B)


def pad128(d):
    out = np.zeros((len(d), 128), np.float32)
    out[:, :64] = d
    return out


def test_matchers_take_64_wide_rows_as_the_same_rows_zero_padded(mods, pair_features):
    import torch

    fm = mods["featureMatching"]
    (dA, _), (dB, _) = pair_features
    assert dA.shape[1] == 64 and dB.shape[1] == 64
    m, met = fm.matchFeaturesScratch(dA, dB, MatchThreshold=1.5, MaxRatio=0.6, ZeroPad=True)
    mp, metp = fm.matchFeaturesScratch(pad128(dA), pad128(dB), MatchThreshold=1.5, MaxRatio=0.6)
    assert len(m) > 100 and np.array_equal(m, mp) and np.array_equal(met.view(np.uint32), metp.view(np.uint32))
    # resident, as kaze_extract hands them out: the [:, :64] view of the padded buffer, and the padded buffer itself
    A, B = kc.pair()
    res = [fm.kaze_extract(KAZE, torch.from_numpy(np.array(x)).cuda(), device_out=True)[0] for x in (A, B)]
    assert res[0].shape[1] == 64 and res[0].stride(0) == 128 and np.array_equal(res[0].cpu().numpy().view(np.uint32), dA.view(np.uint32))
    full = [fm.kaze_extract(KAZE, torch.from_numpy(np.array(x)).cuda(), device_out=True, padded=True)[0] for x in (A, B)]
    assert full[0].shape[1] == 128 and not bool(full[0][:, 64:].any())
    want = fm.match_pairs_csr([pad128(dA), pad128(dB)], [(0, 1)], 0.6, 1.5, True)
    assert int(want[0][-1]) == len(m)
    for sets in (res, full, [dA, dB]):
        got = fm.match_pairs_csr(sets, [(0, 1)], 0.6, 1.5, True)
        assert all(np.array_equal(np.asarray(g), np.asarray(w_)) for g, w_ in zip(got, want))
        gotp = fm.match_pairwise_csr(sets, 0.6, 1.5, True)
        assert all(np.array_equal(np.asarray(g), np.asarray(w_)) for g, w_ in zip(gotp, want))
    g64 = fm.featureMatchingGlobal({"Ratiothreshold": 0.6, "k": 4}, [dA, dB], 2)
    g128 = fm.featureMatchingGlobal({"Ratiothreshold": 0.6, "k": 4}, [pad128(dA), pad128(dB)], 2)
    assert g64[0][1] is not None and len(g64[0][1]) > 100 and np.array_equal(g64[0][1], g128[0][1])


def test_ransac_recovers_the_known_homography(mods, pair_features):
    """Exhaustive matches of the frozen pair -> estimateTransformationRANSAC (projective, maxDistance 5.5): all four image
    corners within 5.5 px of the known homography's, inliers above imageMatching.m:150's 8 + 0.3 * nf."""
    fm, im = mods["featureMatching"], mods["imageMatching"]
    (dA, lA), (dB, lB) = pair_features
    m, _ = fm.matchFeaturesScratch(dA, dB, MatchThreshold=1.5, MaxRatio=0.6, ZeroPad=True)
    nf = len(m)
    p1, p2 = lA[m[:, 0] - 1], lB[m[:, 1] - 1]
    inp = {"maxDistance": 5.5, "inliersConfidence": 99.9, "maxIter": 500}
    samples = im.draw_samples([nf], 500, seed=1)[0]
    H, mask, found = im.estimateTransformationRANSAC(p1, p2, "projective", inp, sample_idx=samples)
    assert found and int(mask.sum()) > 8 + 0.3 * nf, (nf, int(mask.sum()))
    H = np.asarray(H, np.float64)   # maps matchedPoints1 -> matchedPoints2 (1-based [x y 1] columns)
    corners = np.array([[1, 1], [320, 1], [1, 240], [320, 240]], np.float64)
    want = np.concatenate([corners - 1.0, np.ones((4, 1))], 1) @ kc.PAIR_H.T
    want = want[:, :2] / want[:, 2:] + 1.0
    got = np.concatenate([corners, np.ones((4, 1))], 1) @ H.T
    err = np.hypot(*(got[:, :2] / got[:, 2:] - want).T)
    assert err.max() <= 5.5, err


def _scene(mods):
    """kaze_cases.SCENE: 2 x 1 synth views of 640 x 480, f = 900, finest_px = 3, neighbours 30 % of a field of view apart (70 %
    overlap).  On the CPU rendering of that scene the mirror finds 1411 and 1393 keypoints at the default Threshold, 754 ratio
    matches at 0.6 of which 753 lie within 5.5 px of the cameras' homography, against the 8 + 0.3 * 754 = 234.2 that
    imageMatching.m:150 asks for.  Matcher and RANSAC thresholds are the defaults."""
    import torch

    views, cams = kc.scene(mods["synth"], "cuda")
    torch.cuda.synchronize()
    return views, [c["K"] for c in cams]


def test_stitch_end_to_end_with_and_without_intrinsics(mods):
    pl = mods["pipeline"]
    views, Ks = _scene(mods)
    inp = pl.default_input(detector="KAZE", resizeImage=0)
    panos, info = pl.stitch(inp, views, Ks=Ks, tile=(512, 512))
    assert info["n_components"] == 1 and len(panos) == 1 and sorted(info["components"][0]["members"]) == [0, 1]
    pano = panos[0].cpu().numpy() if hasattr(panos[0], "cpu") else np.asarray(panos[0])
    assert (pano.max(axis=2) > 0).mean() > 0.5
    panos2, info2 = pl.stitch(inp, views, tile=(512, 512))
    assert len(panos2) == 1 and "ba" in info2 and len(info2["ba"]) == 1
    assert sorted(info2["components"][0]["members"]) == [0, 1]
    pano2 = panos2[0].cpu().numpy() if hasattr(panos2[0], "cpu") else np.asarray(panos2[0])
    assert (pano2.max(axis=2) > 0).mean() > 0.5
    st = info2["ba"][0]
    assert np.isfinite(st["f_init"]) and st["f_init"] > 0 and len(st["focals"]) == 2
    assert all(np.isfinite(f) and f > 0 for f in st["focals"])


def test_sift_submit_dispatches_kaze_on_the_worker_threads(mods):
    fm, pl = mods["featureMatching"], mods["pipeline"]
    views = [kc.band_limited(20 + k, 200, 260, 2.5, channels=3) for k in range(4)]
    inp = pl.default_input(detector="KAZE")
    futs = pl.sift_submit(inp, views)
    for v, fu in zip(views, futs):
        d, p = fu.result()
        d0, p0 = fm.kaze_extract(inp, v)
        assert d.shape == d0.shape and d.shape[1] == 64 and len(d) > 50
        assert np.array_equal(d.view(np.uint8), d0.view(np.uint8)) and np.array_equal(p.view(np.uint8), p0.view(np.uint8))


def test_one_rank_distributed_run_equals_the_single_process_driver(mods):
    """parallel.stitch_distributed takes the detector (float rows, unlike the binary detectors): one rank, known intrinsics,
    the panorama of pipeline.stitch byte for byte."""
    pl, par = mods["pipeline"], mods["parallel"]
    views, Ks = _scene(mods)
    inp = pl.default_input(detector="KAZE", resizeImage=0)
    pano, info = par.stitch_distributed(inp, dict(enumerate(views)), 2, Ks, (512, 512))
    panos, i2 = pl.stitch(inp, views, Ks=Ks, tile=(512, 512))
    assert info["n_components"] == 1 and i2["n_components"] == 1 and len(panos) == 1
    assert len(info["n_features"]) == 2 and min(info["n_features"]) > 100
    assert tuple(pano.shape) == tuple(panos[0].shape) and np.array_equal(pano.cpu().numpy(), panos[0].cpu().numpy())
