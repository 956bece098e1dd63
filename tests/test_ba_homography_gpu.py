"""GPU: the data term of the homography bundle adjustment (aps_ba_h_normal_eqns) against its numpy mirror
hNormalEqnsMirror bit for bit, its argument checks, planar-scan stitching with the refinement end to end against the
synthetic world, and a report on the 64 x 4K bench scene."""
import time
from importlib import import_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba(gpu):
    return import_module(gpu.__name__ + ".bundleAdjustment")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _problem(rng, n, huber):
    """n random absolute homographies (H(3,3) = 1), a random subset of the pairs with 0, 1, < 64, > 64 (not multiples of
    64) matches, points consistent with the homographies up to noise plus a share of gross errors, so that a Huber
    threshold is active on part of the matches."""
    G = []
    for _ in range(n):
        M = np.eye(3) + np.diag([1, 1, 0.0]) @ rng.normal(0, 0.05, (3, 3))
        M[:2, 2] = rng.normal(0, 50, 2)
        M[2, :2] = rng.normal(0, 3e-5, 2)
        G.append(M / M[2, 2])
    cand = [(i, j) for i in range(n) for j in range(i + 1, n)]
    npairs = min(len(cand), 3 * n)
    pairs = [cand[k] for k in sorted(rng.choice(len(cand), npairs, replace=False))]
    counts = ([130, 1, 0, 63, 64, 65, 200, 300] + [int(c) for c in rng.integers(1, 300, max(0, npairs - 8))])[:npairs]
    plist = []
    for (i, j), m in zip(pairs, counts):
        ui = rng.uniform(0, 640, (m, 2))
        x = np.c_[ui, np.ones(m)] @ G[i].T
        y = np.c_[x[:, :2] / x[:, 2:], np.ones(m)] @ np.linalg.inv(G[j]).T
        uj = y[:, :2] / y[:, 2:] + rng.normal(0, 0.7 * max(huber, 1.0), (m, 2))
        k = m // 5
        uj[:k] += rng.uniform(-40, 40, (k, 2))
        plist.append({"i": i, "j": j, "Ui": ui, "Uj": uj})
    return np.stack(G), plist


@pytest.mark.parametrize("n", [2, 3, 7, 20, 64])
def test_h_normal_eqns_equal_the_mirror(ba, n):
    """H, g and the three sums bit for bit, for the seed first, in the middle and last, Huber on part of the matches and
    off (0); the energy-only call returns the same sums; H is symmetric."""
    rng = np.random.default_rng(500 + n)
    for huber in (2.0, 0.0):
        G, plist = _problem(rng, n, huber)
        dev = ba.DeviceEvaluatorH(plist, n)
        host = ba.HostEvaluatorH(plist, n)
        for seed in sorted({0, n // 2, n - 1}):
            Gs = G.copy()
            Gs[seed] = np.eye(3)
            Hd, gd, sd = dev(Gs, seed, huber, True)
            Hm, gm, sm = host(Gs, seed, huber, True)
            assert Hd.shape == (8 * (n - 1),) * 2 and np.array_equal(_bits(Hd), _bits(Hm))
            assert np.array_equal(_bits(gd), _bits(gm)) and np.array_equal(_bits(sd), _bits(sm))
            assert np.array_equal(Hd, Hd.T) and sd[2] == sum(len(q["Ui"]) for q in plist)
            if huber > 0 and n > 2:
                _, _, s_off = host(Gs, seed, 0.0, False)
                assert s_off[0] > sd[0]  # Huber active on some matches
            H0, g0, s0 = dev(Gs, seed, huber, False)
            assert H0 is None and g0 is None and np.array_equal(_bits(s0), _bits(sd))


def test_h_normal_eqns_bad_arguments(ba, gpu):
    capi = gpu._capi
    rng = np.random.default_rng(9)
    G, plist = _problem(rng, 4, 1.0)
    dev = ba.DeviceEvaluatorH(plist, 4)
    h = dev.problem._h
    Gc = np.ascontiguousarray(G.reshape(4, 9))
    P = 24
    Hb, gb, st = np.zeros((P, P)), np.zeros(P), np.zeros(3)
    ok = capi.lib.aps_ba_h_normal_eqns(h, capi.ptr(Gc), 4, 0, 1.0, 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st))
    assert ok == capi.APS_OK
    cases = [
        (None, capi.ptr(Gc), 4, 0, 1.0, 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st)),  # NULL handle
        (h, None, 4, 0, 1.0, 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st)),  # NULL G
        (h, capi.ptr(Gc), 4, 0, 1.0, 1, None, capi.ptr(gb), capi.ptr(st)),  # NULL H with want_H
        (h, capi.ptr(Gc), 4, 0, 1.0, 1, capi.ptr(Hb), capi.ptr(gb), None),  # NULL stats
        (h, capi.ptr(Gc), 4, -1, 1.0, 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st)),  # seed out of range
        (h, capi.ptr(Gc), 4, 4, 1.0, 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st)),
        (h, capi.ptr(Gc), 4, 0, float("nan"), 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st)),  # non-finite huber
        (h, capi.ptr(Gc), 4, 0, float("inf"), 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st)),
        (h, capi.ptr(Gc), 5, 0, 1.0, 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st)),  # wrong n_cams
        (h, capi.ptr(Gc), 3, 0, 1.0, 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st)),
    ]
    for args in cases:
        assert capi.lib.aps_ba_h_normal_eqns(*args) == capi.APS_E_ARG, args
    Gd = torch.tensor(Gc, device="cuda")  # G in device memory
    assert capi.lib.aps_ba_h_normal_eqns(h, Gd.data_ptr(), 4, 0, 1.0, 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st)) == capi.APS_E_ARG
    Gbad = Gc.copy()
    Gbad[2, 8] = 2.0  # H(3,3) != 1
    assert capi.lib.aps_ba_h_normal_eqns(h, capi.ptr(Gbad), 4, 0, 1.0, 1, capi.ptr(Hb), capi.ptr(gb), capi.ptr(st)) == capi.APS_E_ARG
    # a negative huber clamps to 0 (max(0, opts.Huber)): the same bits as huber = 0
    s_neg, s_zero = np.zeros(3), np.zeros(3)
    assert capi.lib.aps_ba_h_normal_eqns(h, capi.ptr(Gc), 4, 0, -3.0, 0, None, None, capi.ptr(s_neg)) == capi.APS_OK
    assert capi.lib.aps_ba_h_normal_eqns(h, capi.ptr(Gc), 4, 0, 0.0, 0, None, None, capi.ptr(s_zero)) == capi.APS_OK
    assert np.array_equal(_bits(s_neg), _bits(s_zero))


def _corner_err(Ha, Hb, w, h):
    c = np.array([[1, 1, 1], [w, 1, 1], [1, h, 1], [w, h, 1.0]]).T
    a, b = Ha @ c, Hb @ c
    return float(np.max(np.linalg.norm(a[:2] / a[2] - b[:2] / b[2], axis=0)))


def test_planar_scan_refinement_end_to_end(gpu):
    """3 x 2 views at 640 x 480, f = 900, overlap 0.35, sensor noise and gains, forcePlanarScan with
    planarBundleAdjustment: one panorama, the transfer RMSE drops, and every view's H2refined is closer to the true
    homography to the seed, K R_seed R_k' K^-1 in synth's convention (principal point (W/2, H/2), pixel (1, 1) the
    top-left pixel centre), than its chained H2seed (max corner transfer error).  The same call without the key keeps
    H2refined = H2seed (no LM evaluation): its homographies are the chained ones the refinement started from.
    Measured on the MI355X: RMSE 0.272 -> 0.249 px in 9 evaluations (step stop), max corner error 0.39 px refined
    against 1.63 px chained (per view 0.39 / 0.13 / 0.07 / 0.24 / 0.24 against 0.56 / 0.39 / 1.63 / 0.41 / 0.26).
    With overlap 0.5 the chained homographies of this clean scene are already at 0.05-0.2 px and the refinement does
    not improve every view; on 4 x 3 grids it improves 5-8 of 11 views.  Bounds (BOUNDS_E2E): 3x the
    measured RMSE and corner error."""
    synth = import_module(gpu.__name__ + ".synth")
    pl = import_module(gpu.__name__ + ".pipeline")
    w, h, f = 640, 480, 900.0
    imgs, cams = synth.make_scene(3, 2, w, h, f, overlap=0.35, seed=31, device="cuda", finest_px=3.0, gains=True)
    imgs = [im.cpu().numpy() for im in imgs]
    inp = pl.default_input(bands=2, forcePlanarScan=True, planarBundleAdjustment=True)
    t0 = time.perf_counter()
    panos, info = pl.stitch(inp, imgs, tile=(1024, 1024), seed=1, device_out=False)
    wall = time.perf_counter() - t0
    assert len(panos) == 1 and len(info["ba"]) == 1
    st = info["ba"][0]
    comp = info["components"][0]
    members, ref, est = comp["members"], comp["ref"], comp["cameras"]
    assert len(members) == 6 and st["noRotation"] == 1 and st["evaluations"] > 0
    K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]])
    Rs = np.asarray(cams[members[ref]]["R"])
    e_ref, e_seed = [], []
    for q, k in enumerate(members):
        if q == ref:
            assert np.array_equal(est[q]["H2refined"], np.eye(3))
            continue
        T = K @ Rs @ np.asarray(cams[k]["R"]).T @ np.linalg.inv(K)
        T = T / T[2, 2]
        e_ref.append(_corner_err(np.asarray(est[q]["H2refined"]), T, w, h))
    # the chained homographies of the same run: the call without the key
    inp0 = pl.default_input(bands=2, forcePlanarScan=True)
    panos0, info0 = pl.stitch(inp0, imgs, tile=(1024, 1024), seed=1, device_out=False)
    comp0 = info0["components"][0]
    assert comp0["members"] == members and comp0["ref"] == ref and info0["ba"][0]["evaluations"] == 0
    for q, k in enumerate(members):
        c0 = comp0["cameras"][q]
        if q != ref:
            T = K @ Rs @ np.asarray(cams[k]["R"]).T @ np.linalg.inv(K)
            e_seed.append(_corner_err(np.asarray(c0["H2refined"]), T / T[2, 2], w, h))
    print("planar 3x2: rmse %.4f -> %.4f px, %d evaluations (%s), corner error refined %s vs chained %s px, stitch %.2f s"
          % (st["rmse_init"], st["rmse_final"], st["evaluations"], st["lm_stop"], np.round(e_ref, 3).tolist(),
             np.round(e_seed, 3).tolist(), wall))
    assert st["rmse_final"] < st["rmse_init"]
    assert all(a < b for a, b in zip(e_ref, e_seed)), (e_ref, e_seed)
    assert st["rmse_final"] < BOUNDS_E2E["rmse_px"] and max(e_ref) < BOUNDS_E2E["corner_px"]
    pano = np.asarray(panos[0])
    assert pano.dtype == np.uint8 and pano.ndim == 3 and (pano > 0).mean() > 0.5


BOUNDS_E2E = {"rmse_px": 0.75, "corner_px": 1.2}


def test_bench_scene_planar_refinement_report(gpu, ba):
    """The 64 x 4K bench scene with forcePlanarScan and planarBundleAdjustment: the refinement's wall time, LM evaluations
    and the device time per aps_ba_h_normal_eqns (Prof names ba_h_blocks / ba_h_assemble); then one evaluation at the
    final homographies on the device problem and through the numpy mirror, which must agree bit for bit.  No speed bound.
    Measured on the MI355X: 0.14 s, 23 LM evaluations (step stop), 63.7 us of device time per call (blocks 10.8 +
    assembly 52.9), one evaluation 0.24 ms on the device problem against 81.9 ms through the mirror (P = 504).  The
    weighted energy drops 36976 -> 31819; the unweighted RMSE is 2.1e7 px before and 2.8e7 px after: a few matches
    whose transfer through the chained homographies of this rotational f = 8000 scene lands near the horizon of the
    seed's plane dominate it, and Huber caps their weighted residuals."""
    synth = import_module(gpu.__name__ + ".synth")
    pl = import_module(gpu.__name__ + ".pipeline")
    capi = gpu._capi
    w, h, f, ov, seed, finest = 3840, 2160, 8000.0, 0.40, 12345, 16.0
    cams = synth.grid_cameras(8, 8, w, h, f, 2 * np.arctan(w / (2 * f)) * (1 - ov), 2 * np.arctan(h / (2 * f)) * (1 - ov), 1.0, seed)
    imgs = [synth.render_view(cams[i], h, w, seed, "cuda", finest_px=finest) for i in range(64)]
    torch.cuda.synchronize()
    inp = pl.default_input(bands=5, forcePlanarScan=True, planarBundleAdjustment=True)
    descs, kps = pl.extract_features(inp, imgs)
    res = pl.match_and_verify(inp, descs, kps, 0)
    ncomp, labels = pl.connected_components(res["numMatches"])
    assert ncomp == 1
    capi.profile_enable(True)
    capi.profile_reset()
    ba_info = []
    t0 = time.perf_counter()
    comps = pl.recognize_panoramas(64, res["pairs"], res["models"], res["numMatches"], None, labels, None, keypoints=kps,
                                   inliers=res["inliers"], image_sizes=[(h, w)] * 64, input=inp, ba_info=ba_info)
    wall = time.perf_counter() - t0
    tb, nb = capi.profile_get("ba_h_blocks")
    ta, na = capi.profile_get("ba_h_assemble")
    capi.profile_enable(False)
    st = ba_info[0]
    assert len(comps) == 1 and len(comps[0]["members"]) == 64 and st["noRotation"] == 1
    # the LM lowers the Huber-weighted energy; the unweighted RMSE of the chained start can be dominated by a few huge
    # transfers, and need not drop
    assert na == st["evaluations"] and st["E_final"] <= st["E_init"]
    # one evaluation at the final homographies: device problem against the mirror
    members, ref, est = comps[0]["members"], comps[0]["ref"], comps[0]["cameras"]
    loc = {k: q for q, k in enumerate(members)}
    plist = []
    for p, (i, j) in enumerate(res["pairs"]):
        a, b = sorted((loc[i], loc[j]))
        M = np.asarray(res["inliers"][p], np.int64)
        if loc[i] > loc[j]:
            M = M[:, ::-1]
        Ui = np.asarray(kps[members[a]].cpu() if torch.is_tensor(kps[members[a]]) else kps[members[a]], np.float64)[M[:, 0] - 1]
        Uj = np.asarray(kps[members[b]].cpu() if torch.is_tensor(kps[members[b]]) else kps[members[b]], np.float64)[M[:, 1] - 1]
        Ui, Uj = ba.subsampleMatchesH(Ui, Uj, a, b, inp["MaxMatches"])
        plist.append({"i": a, "j": b, "Ui": Ui, "Uj": Uj})
    G = np.stack([np.asarray(c["H2refined"]) for c in est])
    dev = ba.DeviceEvaluatorH(plist, 64)
    host = ba.HostEvaluatorH(plist, 64)
    dev(G, ref, inp["sigmaHuber"], True)  # warm
    t0 = time.perf_counter()
    Hd, gd, sd = dev(G, ref, inp["sigmaHuber"], True)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    Hh, gh, sh = host(G, ref, inp["sigmaHuber"], True)
    t_host = time.perf_counter() - t0
    assert np.array_equal(_bits(Hd), _bits(Hh)) and np.array_equal(_bits(gd), _bits(gh)) and np.array_equal(_bits(sd), _bits(sh))
    print("bench scene planar: refinement %.3f s, E %.6g -> %.6g, rmse %.6g -> %.6g px, %d LM evaluations (%s), device %.1f us per "
          "aps_ba_h_normal_eqns (blocks %.1f + assembly %.1f), one evaluation %.2f ms on the device problem vs %.2f ms "
          "through the mirror, P = %d" % (
              wall, st["E_init"], st["E_final"], st["rmse_init"], st["rmse_final"], st["evaluations"], st["lm_stop"],
              1e3 * (tb + ta) / max(na, 1),
              1e3 * tb / max(nb, 1), 1e3 * ta / max(na, 1), 1e3 * t_dev, 1e3 * t_host, Hd.shape[0]))
