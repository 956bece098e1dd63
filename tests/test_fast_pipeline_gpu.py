"""FAST/FREAK through the operators behind feature extraction: the binary branch of matchFeaturesScratch, the pairwise and
the global matcher against NumPy restatements of the reference (tests/fast_cases.py), and the whole stitch.

The scene: three 240 x 320 views of the procedural world, neighbours 30 % of a field of view apart, rendered on the CPU so the
device sees the bytes the CPU check saw.  The world is smooth: detectFASTFeatures' default MinContrast = 0.2 finds nothing,
MinContrast = 0.08 gives 227 / 220 / 220 keypoints (mirror).  With Matchingthreshold = 20 percent (matchFeaturesScratch.m:32
suggests 10 or more) and the default ratio 0.6, the mirror plus the NumPy matcher alone give 80 / 44 / 82 matches on the pairs
(0,1) / (0,2) / (1,2), every one within 5.5 px of the known homography - against the 8 + 0.3 * nf = 32 / 21.2 / 32.6 inliers
imageMatching.m:150 asks for."""
from importlib import import_module

import numpy as np
import pytest

import fast_cases as fc
import fast_mirror as fmir

INP = {"detector": "FAST", "MinContrast": 0.08}
THR, RATIO = 20.0, 0.6


@pytest.fixture(scope="module")
def mirror_sets():
    views, _ = fc.scene()
    return [fmir.extract(v, fc.tables(), MinContrast=0.08) for v in views]


def test_cpu_check_of_the_scene(mirror_sets):
    """Device-free: the mirror and the NumPy matcher alone yield enough correct matches for RANSAC."""
    _, cams = fc.scene()
    assert [len(s[0]) for s in mirror_sets] == [227, 220, 220]
    counts = []
    for (i, j) in [(0, 1), (0, 2), (1, 2)]:
        m, _ = fc.match_binary(mirror_sets[i][0], mirror_sets[j][0], RATIO, THR)
        Hm = cams[j]["K"] @ cams[j]["R"] @ cams[i]["R"].T @ np.linalg.inv(cams[i]["K"])
        p = np.concatenate([mirror_sets[i][1][m[:, 0] - 1], np.ones((len(m), 1))], 1) @ Hm.T
        q = mirror_sets[j][1][m[:, 1] - 1]
        good = int((np.hypot(p[:, 0] / p[:, 2] - q[:, 0], p[:, 1] / p[:, 2] - q[:, 1]) <= 5.5).sum())
        assert good > 8 + 0.3 * len(m)
        counts.append((len(m), good))
    assert counts == [(80, 80), (44, 44), (82, 82)]


@pytest.fixture(scope="module")
def mods(gpu):
    return {k: import_module(gpu.__name__ + "." + k) for k in ("featureMatching", "pipeline")}


@pytest.fixture(scope="module")
def sets(mods, mirror_sets):
    """Device features of the three views (host binaryFeatures), computed once; they equal the mirror's."""
    fm = mods["featureMatching"]
    out = [fm.getFeaturePoints(INP, v) for v in fc.scene()[0]]
    for (f, pts), (md, mloc, _) in zip(out, mirror_sets):
        assert np.array_equal(f.Features, md) and np.array_equal(pts, mloc)
    return out


@pytest.mark.gpu
def test_matchFeaturesScratch_binary_branch_equals_the_numpy_restatement(mods, sets):
    import torch

    fm = mods["featureMatching"]
    A, B = sets[0][0], sets[1][0]
    want_m, want_d = fc.match_binary(A.Features, B.Features, RATIO, THR)
    assert len(want_m) == 80
    for method in ("Exhaustive", "Approximate"):
        m, d = fm.matchFeaturesScratch(A, B, Method=method, MatchThreshold=THR, MaxRatio=RATIO)
        assert m.dtype == np.uint32 and d.dtype == np.float32
        assert np.array_equal(m, want_m) and np.array_equal(d.view(np.uint32), want_d.view(np.uint32))
    # other thresholds, no uniqueness, one candidate only (second = nBits), resident sets, unpacked bits
    for (ratio, thr, uniq) in ((0.8, 30.0, True), (1.0, 100.0, False), (0.6, 10.0, True)):
        m, d = fm.matchFeaturesScratch(A, B, MatchThreshold=thr, MaxRatio=ratio, Unique=uniq)
        wm, wd = fc.match_binary(A.Features, B.Features, ratio, thr, uniq)
        assert np.array_equal(m, wm) and np.array_equal(d, wd), (ratio, thr, uniq)
    one = fm.binaryFeatures(B.Features[:1])
    m, d = fm.matchFeaturesScratch(A, one, MatchThreshold=100.0, MaxRatio=1.0)
    wm, wd = fc.match_binary(A.Features, B.Features[:1], 1.0, 100.0)
    assert np.array_equal(m, wm) and np.array_equal(d, wd) and len(m) == 1
    rA, rB = [fm.binaryFeatures(torch.from_numpy(x.Features).cuda()) for x in (A, B)]
    torch.cuda.synchronize()
    m, d = fm.matchFeaturesScratch(rA, rB, MatchThreshold=THR, MaxRatio=RATIO)
    assert np.array_equal(m, want_m) and np.array_equal(d, want_d)
    bits = [np.unpackbits(x.Features[:60], axis=1, bitorder="big").astype(bool) for x in (A, B)]
    m, d = fm.matchFeaturesScratch(bits[0], bits[1], MatchThreshold=THR, MaxRatio=RATIO)
    wm, wd = fc.match_binary(A.Features[:60], B.Features[:60], RATIO, THR)
    assert np.array_equal(m, wm) and np.array_equal(d, wd)


@pytest.mark.gpu
def test_featureMatchingPairwise_equals_the_per_pair_results(mods, sets):
    fm = mods["featureMatching"]
    descs = [s[0] for s in sets]
    got = fm.featureMatchingPairwise({"Matchingthreshold": THR, "Ratiothreshold": RATIO}, descs, 3)
    for i in range(3):
        for j in range(3):
            if i < j:
                wm, _ = fc.match_binary(descs[i].Features, descs[j].Features, RATIO, THR)
                assert got[i][j].dtype == np.float64 and np.array_equal(got[i][j], wm.astype(np.float64))
            else:
                assert got[i][j] is None
    assert [len(got[0][1]), len(got[0][2]), len(got[1][2])] == [80, 44, 82]


@pytest.mark.gpu
@pytest.mark.parametrize("bf", [0, 1])
def test_featureMatchingGlobal_binary_branch_equals_the_numpy_restatement(mods, sets, bf):
    fm = mods["featureMatching"]
    descs = [s[0] for s in sets]
    got = fm.featureMatchingGlobal({"Ratiothreshold": 0.8, "k": 4, "BFMatch": bf}, descs, 3)
    want = fc.global_binary([d.Features for d in descs], 0.8, 4)
    assert sum(len(v) for v in want.values()) > 100
    for i in range(3):
        for j in range(3):
            if (i, j) in want:
                assert np.array_equal(got[i][j], want[(i, j)]), (i, j)
            else:
                assert got[i][j] is None


@pytest.mark.gpu
def test_stitch_end_to_end_with_fast(mods):
    pl = mods["pipeline"]
    views, cams = fc.scene()
    inp = pl.default_input(detector="FAST", MinContrast=0.08, Matchingthreshold=THR, resizeImage=0)
    panos, info = pl.stitch(inp, views, Ks=[c["K"] for c in cams], tile=(512, 512))
    assert info["n_features"] == [227, 220, 220]
    assert info["n_components"] == 1 and len(panos) == 1 and sorted(info["components"][0]["members"]) == [0, 1, 2]
    assert [int(info["putative"][i, j]) for (i, j) in ((0, 1), (0, 2), (1, 2))] == [80, 44, 82]
    pano = panos[0].cpu().numpy() if hasattr(panos[0], "cpu") else np.asarray(panos[0])
    assert pano.ndim == 3 and (pano.max(axis=2) > 0).mean() > 0.5
