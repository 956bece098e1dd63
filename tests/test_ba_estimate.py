"""CPU: camera estimation without known intrinsics (bundleAdjustment.py) - the focal estimates of
initializeCameraMatrices.m, the spanning tree and rotation chaining, the rotation-consistency verdict, the Brown-Lowe
prior, the per-camera step caps, and the whole incremental bundle adjustment driven by the oracle's normal-equation
blocks (oracle/ba_oracle.c) on synthetic correspondences."""
from importlib import import_module

import numpy as np
import pytest

import oracle

W, H = 640, 480


@pytest.fixture(scope="module")
def ba(aps):
    return import_module(aps.__name__ + ".bundleAdjustment")


def _rot(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def _K(f, w=W, h=H):
    return np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]])


def _grid_cams(nx, ny, f, yaw_step=18.0, pitch_step=14.0, rng=None):
    cams = []
    for r in range(ny):
        for c in range(nx):
            R = _rot("x", (r - (ny - 1) / 2) * pitch_step) @ _rot("y", (c - (nx - 1) / 2) * yaw_step)
            if rng is not None:
                R = _rot("z", rng.normal(0, 1.0)) @ R
            cams.append({"f": f, "R": R, "K": _K(f)})
    return cams


def _homography(ci, cj):  # j -> i
    return ci["K"] @ ci["R"] @ cj["R"].T @ np.linalg.inv(cj["K"])


def _correspondences(cams, n_pts=4000, outliers=0.0, noise=0.3, seed=0, min_matches=30):
    """World directions seen by every camera; pairs with enough common points become verified pairs."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_pts, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = len(cams)
    kps, vis = [], []
    for c in cams:
        x = (c["K"] @ c["R"] @ d.T).T
        z = x[:, 2]
        u = x[:, :2] / np.where(np.abs(z) < 1e-9, 1e-9, z)[:, None]
        ok = (z > 0) & (u[:, 0] > 1) & (u[:, 0] < W - 1) & (u[:, 1] > 1) & (u[:, 1] < H - 1)
        kps.append(u + rng.normal(0, noise, u.shape))
        vis.append(ok)
    nm = np.zeros((n, n))
    matches = [[None] * n for _ in range(n)]
    tforms = [[None] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            common = np.nonzero(vis[i] & vis[j])[0]
            if len(common) < min_matches:
                continue
            M = np.stack([common + 1, common + 1], 1)
            k = int(outliers * len(M))
            if k:  # wrong partners: a point of j that is not the one seen in i
                bad = rng.choice(len(M), k, replace=False)
                M[bad, 1] = rng.choice(np.nonzero(vis[j])[0], k) + 1
            matches[i][j] = M
            nm[i, j] = len(M)
            tforms[i][j] = _homography(cams[i], cams[j])
            tforms[j][i] = np.linalg.inv(tforms[i][j])
    return kps, matches, nm, tforms


def _angle(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))


def _align_err(truth, est):
    A = [np.asarray(t["R"]).T @ np.asarray(e["R"]) for t, e in zip(truth, est)]
    U, _, Vt = np.linalg.svd(np.mean(A, 0))
    M = U @ Vt
    return [_angle(a @ M.T) for a in A]


# ---- focal estimation --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f", [700.0, 1500.0])
def test_focal_estimates_recover_f(ba, f):
    cams = _grid_cams(3, 2, f, yaw_step=15, pitch_step=10, rng=np.random.default_rng(1))
    pairs = [{"i": i, "j": j, "Hij": _homography(cams[i], cams[j])} for i in range(6) for j in range(i + 1, 6)]
    sizes = np.array([[H, W, 3]] * 6, np.float64)
    for p in pairs[:4]:
        Hc = ba.centerNormalizeH(p["Hij"], W, H, W, H)
        assert abs(np.linalg.det(Hc) - 1) < 1e-12
    fs = ba.focalShumSzeliski(pairs, sizes)
    fw = ba.focalWConstraint(pairs, sizes)
    assert abs(fs / f - 1) < 1e-6, fs
    assert abs(fw / f - 1) < 1e-6, fw
    for method, want in (("shumSzeliskiOneHPaper", fs), ("wConstraint", fw)):
        K, R, fUsed, H2, noRot = ba.initializeKRf({"focalEstimateMethod": method}, pairs, sizes, 6, 0, _tf(pairs, 6),
                                                  _nm(pairs, 6))
        assert fUsed == want and K[3][0, 0] == want and K[3][0, 2] == W / 2 and K[3][1, 2] == H / 2


def _tf(pairs, n):
    T = [[None] * n for _ in range(n)]
    for p in pairs:
        T[p["i"]][p["j"]] = p["Hij"]
        T[p["j"]][p["i"]] = np.linalg.inv(p["Hij"])
    return T


def _nm(pairs, n, w=None):
    G = np.zeros((n, n))
    for k, p in enumerate(pairs):
        G[p["i"], p["j"]] = 100 + k if w is None else w[k]
    return G


def test_focal_fallback_on_degenerate_homographies(ba):
    """Pure translations (a planar scan) carry no focal: both methods give none, and initializeKRf falls back to
    0.8 max(H, W)."""
    T = np.array([[1, 0, 120.0], [0, 1, 3.0], [0, 0, 1]])
    pairs = [{"i": 0, "j": 1, "Hij": T}, {"i": 1, "j": 2, "Hij": T}]
    sizes = np.array([[H, W, 3]] * 3, np.float64)
    assert np.isnan(ba.focalsHomographyShumsz(ba.centerNormalizeH(T, W, H, W, H)))
    assert ba.focalShumSzeliski(pairs, sizes) is None and ba.focalWConstraint(pairs, sizes) is None
    for method in ("shumSzeliskiOneHPaper", "wConstraint"):
        _, _, f, _, _ = ba.initializeKRf({"focalEstimateMethod": method}, pairs, sizes, 3, 1, _tf(pairs, 3), _nm(pairs, 3))
        assert f == 0.8 * W
    with pytest.raises(ValueError):
        ba.initializeKRf({"focalEstimateMethod": "none"}, pairs, sizes, 3, 1, _tf(pairs, 3), _nm(pairs, 3))


# ---- spanning tree, rotation chaining, consistency -------------------------------------------------------------------------

def test_spanning_tree_and_rotation_chaining(ba):
    f = 900.0
    cams = _grid_cams(4, 2, f, rng=np.random.default_rng(2))
    n = len(cams)
    pairs = [{"i": i, "j": j, "Hij": _homography(cams[i], cams[j])} for i in range(n) for j in range(i + 1, n)
             if abs(i % 4 - j % 4) <= 1 and abs(i // 4 - j // 4) <= 1]
    rng = np.random.default_rng(3)
    w = rng.integers(50, 500, len(pairs)).astype(float)
    G = _nm(pairs, n, w)
    tree = ba.maximumSpanningTree(G)
    assert np.array_equal(tree, tree.T) and (np.triu(tree, 1) > 0).sum() == n - 1
    # a maximum spanning tree: no non-tree edge outweighs the lightest edge of the tree path it closes
    import itertools
    adj = {k: [m for m in range(n) if tree[k, m] > 0] for k in range(n)}

    def path(a, b, seen=()):
        if a == b:
            return [a]
        for m in adj[a]:
            if m not in seen:
                p = path(m, b, seen + (a,))
                if p:
                    return [a] + p
        return None

    for (i, j) in itertools.combinations(range(n), 2):
        if G[i, j] > 0 and tree[i, j] == 0:
            p = path(i, j)
            assert min(tree[a, b] for a, b in zip(p, p[1:])) >= G[i, j]
    sizes = np.array([[H, W, 3]] * n, np.float64)
    seed = 5
    K, R, fUsed, H2, noRot = ba.initializeKRf({}, pairs, sizes, n, seed, _tf(pairs, n), G)
    assert abs(fUsed / f - 1) < 1e-6 and not noRot
    assert np.array_equal(R[seed], np.eye(3))
    assert max(_align_err(cams, [{"R": r} for r in R])) < 1e-5
    assert all(np.array_equal(h, np.eye(3)) for h in H2)  # rotational: no chained homographies


def _planar_scan(n=6, scale=8.0, tilt=1.0, f=600.0):
    """A translating camera (no rotation) over a scene with strong parallax: each pair's homography is that of its own
    dominant plane, H(j -> i) = K (I + (C_j - C_i) n') K^-1 with the depth of camera j left out, so the pairs do not
    compose (as independent RANSAC fits of such a scene do not).  With tilt = 0 they do compose (a fronto-parallel plane
    scanned sideways)."""
    K = _K(f)
    nrm = np.array([0.0, tilt, 1.0]) / np.hypot(tilt, 1.0)
    C = [np.array([k * 0.3 * scale, (k % 2) * 0.2 * scale, 0.0]) for k in range(n)]
    pairs = []
    for i in range(n):
        for j in range(i + 1, n):
            Hm = K @ (np.eye(3) + np.outer(C[j] - C[i], nrm)) @ np.linalg.inv(K)
            pairs.append({"i": i, "j": j, "Hij": Hm / Hm[2, 2]})
    return pairs


def test_rotation_consistency_flags_a_planar_scan_and_passes_a_rotation(ba):
    """The reference's verdict (median > 0.6 deg AND max > 100 deg) after the spanning-tree chaining of initializeKRf.
    Measured: the rotational set 0 deg; the translated planar set median 43.8, max 173.1 deg (flagged); a milder scan
    (fronto-parallel, translations of up to 6 plane distances) median 27.0, max 45.0 deg (not flagged: the rule needs
    both, and consistent planar homographies rarely reach 100 deg)."""
    sizes = np.array([[H, W, 3]] * 6, np.float64)
    cams = _grid_cams(3, 2, 800.0, rng=np.random.default_rng(4))
    pairs = [{"i": i, "j": j, "Hij": _homography(cams[i], cams[j])} for i in range(6) for j in range(i + 1, 6)]
    _, R, f, _, noRot = ba.initializeKRf({}, pairs, sizes, 6, 0, _tf(pairs, 6), _nm(pairs, 6))
    flag, mean, med, mx = ba.rotationConsistency(pairs, sizes, R, f)
    assert not noRot and not flag and mx < 1e-4
    pairs = _planar_scan()
    _, R, f, H2, noRot = ba.initializeKRf({}, pairs, sizes, 6, 0, _tf(pairs, 6), _nm(pairs, 6))
    flag, mean, med, mx = ba.rotationConsistency(pairs, sizes, R, f)
    assert noRot and flag and med > 0.6 and mx > 100, (med, mx)
    assert not all(np.array_equal(h, np.eye(3)) for h in H2)  # planar: the chained homographies are built
    pairs = _planar_scan(scale=4.0, tilt=0.0)
    _, R, f, _, noRot = ba.initializeKRf({}, pairs, sizes, 6, 0, _tf(pairs, 6), _nm(pairs, 6))
    assert not noRot


def test_planar_chained_homographies(ba):
    """H2seed chains the pairs' homographies over the tree from the seed: on a consistent set every view's chain equals
    its direct homography to the seed."""
    pairs = _planar_scan(scale=2.0, tilt=0.0)
    n, seed = 6, 2
    sizes = np.array([[H, W, 3]] * n, np.float64)
    T = _tf(pairs, n)
    _, _, _, H2, _ = ba.initializeKRf({"forcePlanarScan": True}, pairs, sizes, n, seed, T, _nm(pairs, n))
    assert np.array_equal(H2[seed], np.eye(3))
    for k in range(n):
        if k != seed:
            want = T[seed][k] / T[seed][k][2, 2]
            assert np.allclose(H2[k], want, rtol=1e-9, atol=1e-9) and H2[k][2, 2] == 1.0


# ---- prior and step caps ---------------------------------------------------------------------------------------------------

def test_brown_lowe_prior_by_hand(ba):
    camList = [0, 1, 3, 4, 7]
    seed = 3
    fs = {0: 800.0, 1: 820.0, 3: 780.0, 4: 790.0, 7: 810.0}
    cams = [{"f": fs.get(k, 1.0), "R": np.eye(3), "cx": 1.0, "cy": 1.0} for k in range(8)]
    _, pmap = ba.buildDeltaVector(cams, camList, seed)
    lf, lm = 123.0, 50.0
    C = ba.buildBrownLowePrior(camList, seed, cams, {"FocalSmoothnessWeight": lf, "FocalMeanWeight": lm}, pmap)
    P = 4 * 4 + 1
    assert C.shape == (P, P)
    fbar = np.mean(list(fs.values()))
    sf2, st2 = max(1.0, fbar / 20) ** 2, (np.pi / 16) ** 2
    want = np.zeros((P, P))
    fcol = {0: 3, 1: 7, 3: 8, 4: 12, 7: 16}  # camera 3 is the seed: one column (8)
    for k, s in ((0, 0), (1, 4), (4, 9), (7, 13)):
        want[s:s + 3, s:s + 3] = np.eye(3) / st2
    for c in fcol.values():
        want[c, c] = 1 / sf2
    # smoothness: list neighbours at most two apart in camList AND in camera index: (0,1) (0,3)? no (|0-3| = 3), (1,3), (1,4)?
    # |1-4| = 3 no, (3,4), (3,7)? no, (4,7)? no
    for a, b in ((0, 1), (1, 3), (3, 4)):
        fa, fb = fcol[a], fcol[b]
        want[fa, fa] += lf
        want[fb, fb] += lf
        want[fa, fb] -= lf
        want[fb, fa] -= lf
    n = 5
    for a in fcol.values():
        for b in fcol.values():
            want[a, b] += lm * (n - 1) / n if a == b else -lm / n
    assert np.allclose(C, want, rtol=1e-12, atol=1e-12)
    assert np.array_equal(C, C.T)


def test_step_cap(ba):
    cams = [{"f": 1000.0, "R": np.eye(3), "cx": 0, "cy": 0}, {"f": 500.0, "R": np.eye(3), "cx": 0, "cy": 0}]
    _, pmap = ba.buildDeltaVector(cams, [0, 1], 0)
    d = np.array([30.0, 0.3, -0.4, 0.0, -50.0])  # seed df, then camera 1: |dth| = 0.5 rad, df
    out = ba.capPerCameraStep(d, pmap, cams, np.deg2rad(5), 0.01)
    assert out[0] == 10.0 and out[4] == -5.0
    assert abs(np.linalg.norm(out[1:4]) - np.deg2rad(5)) < 1e-15 and np.allclose(out[1:4] / np.linalg.norm(out[1:4]), d[1:4] / 0.5)
    small = np.array([-3.0, 0.01, 0.0, 0.02, 2.0])
    assert np.array_equal(ba.capPerCameraStep(small, pmap, cams, np.deg2rad(5), 0.01), small)


def test_subsample_seed_saturates_like_matlab(ba):
    """uint32 arithmetic saturates in MATLAB: for principal points of a few hundred pixels the seed is 1."""
    c = {"K": _K(800.0)}
    assert ba.randpermSeed(c, c) == 1
    tiny = {"K": np.array([[1, 0, 0.002], [0, 1, 0.0], [0, 0, 1]])}  # round(1e3 * 0.002) = 2: nothing saturates
    assert ba.randpermSeed(tiny, tiny) == (1664525 * 2 + 1013904223 * 2) % (2 ** 31 - 1)
    M = np.stack([np.arange(1, 1001), np.arange(1, 1001)], 1)
    a = ba.subsampleMatches(M, c, c, 300)
    assert a.shape == (300, 2) and len(np.unique(a[:, 0])) == 300
    assert np.array_equal(a, ba.subsampleMatches(M, c, c, 300))  # the same subset on every call
    assert ba.subsampleMatches(M[:200], c, c, 300) is not None and len(ba.subsampleMatches(M[:200], c, c, 300)) == 200


# ---- the whole incremental driver on the oracle's blocks ------------------------------------------------------------------

def _host_evaluator(ba):
    return lambda m, k, both: ba.HostEvaluator(m, k, both, blocks=lambda *a: oracle.ba_pair_blocks(*a))


@pytest.mark.parametrize("n_cams", [6, 8])
def test_incremental_bundle_adjustment_on_oracle_blocks(ba, n_cams):
    f = 750.0
    rng = np.random.default_rng(40 + n_cams)
    truth = _grid_cams(n_cams // 2, 2, f, yaw_step=20, pitch_step=16, rng=rng)
    kps, matches, nm, _ = _correspondences(truth, n_pts=3000, outliers=0.10, seed=n_cams)
    # the homographies the RANSAC would hand over: from perturbed cameras (f off by 1 %, rotations by ~1 deg)
    pert = [{"f": f * 1.01, "K": _K(f * 1.01), "R": _rot("y", rng.normal(0, 0.7)) @ _rot("x", rng.normal(0, 0.7)) @ c["R"]}
            for c in truth]
    n = len(truth)
    tforms = [[None] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            if i != j and (nm[min(i, j), max(i, j)] > 0):
                tforms[i][j] = _homography(pert[i], pert[j])
    history = []
    inp = {"maxIterLM": 40, "lambda": 1e-3, "sigmaHuber": 2.0, "focalEstimateMethod": "shumSzeliskiOneHPaper",
           "residualOneDirection": False, "MaxMatches": 300}
    sizes = np.array([[H, W, 3]] * n, np.float64)
    cams, seed, st = ba.bundleAdjustmentRKf(inp, nm, matches, kps, sizes, tforms, evaluator=_host_evaluator(ba),
                                            history=history)
    assert st["noRotation"] == 0 and st["camList"] == list(range(n))
    assert history and all(e1 < e0 for (e0, e1) in history)  # every accepted step lowers the energy
    assert st["evaluations"] > 2 * len(history)
    assert st["rmse_final"] < st["rmse_init"]
    ferr = max(abs(c["f"] / f - 1) for c in cams)
    rerr = max(_align_err(truth, cams))
    print("n=%d: f_init %.1f, f %s, rot err %.3f deg, rmse %.3f -> %.3f, %d evaluations" % (
        n, st["f_init"], [round(c["f"], 1) for c in cams], rerr, st["rmse_init"], st["rmse_final"], st["evaluations"]))
    assert abs(st["f_init"] / f - 1.01) < 1e-6  # the perturbed homographies' focal
    # The seed's one focal column carries the dthx Jacobian column, as in the reference (the blocks' leading column,
    # oracle-pinned), and the prior couples every focal to it: the focal stays near its estimate (with f off by 4 % it
    # stayed at 780 of 750) and the rotations absorb the rest.  Measured here: rotation error 0.21 / 0.31 deg (6 / 8
    # views) from 0.6-1 deg, Huber-weighted RMSE 6.6 -> 5.3 / 5.9 -> 5.1 px with 10 % outliers, 680 / 476 evaluations.
    assert ferr < 0.05, ferr
    rinit = max(_align_err(truth, pert))
    assert rerr < rinit, (rerr, rinit)
    for c in cams:
        assert abs(np.linalg.det(c["R"]) - 1) < 1e-12 and np.allclose(c["R"] @ c["R"].T, np.eye(3), atol=1e-12)


def test_planar_set_keeps_the_chained_homographies(ba):
    """forcePlanarScan: no LM at all, noRotation = 1 on every camera and H2refined = H2seed."""
    truth = _grid_cams(3, 1, 700.0)
    kps, matches, nm, tforms = _correspondences(truth, n_pts=1500, seed=5)
    inp = {"forcePlanarScan": True}
    sizes = np.array([[H, W, 3]] * 3, np.float64)
    calls = []
    cams, seed, st = ba.bundleAdjustmentRKf(inp, nm, matches, kps, sizes, tforms, evaluator=lambda *a: calls.append(a))
    assert not calls and st["evaluations"] == 0
    assert all(c["noRotation"] == 1 and c["H2refined"] is c["H2seed"] for c in cams)
    assert np.allclose(cams[seed]["H2refined"], np.eye(3))
