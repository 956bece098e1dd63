"""GPU: the resident bundle-adjustment problem (aps_ba_problem_create / aps_ba_normal_eqns) against the host mirror
accumulateNormalEqnsBlock bit for bit, its argument checks, and stitching without known intrinsics end to end (focal
estimation + bundle adjustment), checked against the synthetic world."""
import time
from importlib import import_module

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba(gpu):
    return import_module(gpu.__name__ + ".bundleAdjustment")


def _rand_rot(rng, scale):
    w = rng.normal(0, scale, 3)
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / a
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def _problem(rng, n, density=0.5, empty=0):
    """n cameras about one centre, random keypoints, random 1-based match lists on a random subset of the pairs (some of
    them empty)."""
    cams = []
    for _ in range(n):
        f = float(rng.uniform(600, 1200))
        cams.append({"f": f, "cx": 320.0, "cy": 240.0, "R": _rand_rot(rng, 0.3),
                     "K": np.array([[f, 0, 320.0], [0, f, 240.0], [0, 0, 1]])})
    kps = [rng.uniform(0, 640, (300, 2)) for _ in range(n)]
    matches = [[None] * n for _ in range(n)]
    cand = [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < density]
    for q, (i, j) in enumerate(cand):
        m = 0 if q < empty else int(rng.integers(1, 200))
        matches[i][j] = np.stack([rng.integers(1, 301, m), rng.integers(1, 301, m)], 1)
    return cams, kps, matches


def _mirror(ba, Phi, pmap, cams, camList, seed, matches, kps, sigma, both):
    return ba.accumulateNormalEqnsBlock(Phi, pmap, cams, camList, seed, matches, kps, None, sigma, {"OneDirection": not both},
                                        blocks=lambda *a: oracle.ba_pair_blocks(*a))


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


@pytest.mark.parametrize("n,sub,both", [(3, "all", True), (7, "all", False), (12, "contiguous", True),
                                        (20, "noncontiguous", True), (33, "noncontiguous", False), (64, "all", True)])
def test_normal_eqns_equal_the_host_mirror(ba, n, sub, both):
    """H, g, E and rmse bit for bit; pairs outside camList and pairs without matches take no part.  (A block entry is never
    -0.0: the blocks' sums start at +0.0; the assembly still writes a lone off-diagonal block as 0.0 + x, as the mirror
    does.)"""
    rng = np.random.default_rng(1000 + n)
    cams, kps, matches = _problem(rng, n, density=min(1.0, 8.0 / n), empty=2)
    dev = ba.DeviceEvaluator(matches, kps, both)
    if sub == "all":
        camList = list(range(n))
    elif sub == "contiguous":
        camList = list(range(2, n - 3))
    else:
        camList = sorted(rng.choice(n, max(2, (2 * n) // 3), replace=False).tolist())
    for seed in (camList[0], camList[len(camList) // 2]):
        Phi, pmap = ba.buildDeltaVector(cams, camList, seed)
        Phi[:] = rng.normal(0, 1e-3, len(Phi)) * np.array([1 if e % 4 != 3 else 1e3 for e in range(len(Phi))])
        sigma = float(rng.uniform(1.0, 4.0))
        H, g, E, rmse = dev(Phi, pmap, cams, camList, seed, sigma, True)
        Hm, gm, Em, rm = _mirror(ba, Phi, pmap, cams, camList, seed, matches, kps, sigma, both)
        assert H.shape == Hm.shape and np.array_equal(_bits(H), _bits(Hm))
        assert np.array_equal(_bits(g), _bits(gm)) and _bits(E) == _bits(Em) and _bits(rmse) == _bits(rm)
        assert E > 0 and np.array_equal(H, H.T)
        # energy only: no H, the same bits
        H0, g0, E0, r0 = dev(Phi, pmap, cams, camList, seed, sigma, False)
        assert H0 is None and g0 is None and _bits(E0) == _bits(E) and _bits(r0) == _bits(rmse)


def test_normal_eqns_without_live_pairs(ba):
    """Only empty pairs (or none among camList): H and g are zero, E = rmse = 0, as the mirror returns."""
    rng = np.random.default_rng(7)
    cams, kps, matches = _problem(rng, 4, density=1.0, empty=6)
    dev = ba.DeviceEvaluator(matches, kps, True)
    Phi, pmap = ba.buildDeltaVector(cams, [0, 1, 3], 1)
    H, g, E, rmse = dev(Phi, pmap, cams, [0, 1, 3], 1, 2.0, True)
    Hm, gm, Em, rm = _mirror(ba, Phi, pmap, cams, [0, 1, 3], 1, matches, kps, 2.0, True)
    assert np.array_equal(_bits(H), _bits(Hm)) and np.array_equal(_bits(g), _bits(gm)) and E == Em == 0.0 and rmse == rm == 0.0


def test_bad_arguments(ba, gpu):
    capi = gpu._capi
    rng = np.random.default_rng(8)
    cams, kps, matches = _problem(rng, 5, density=1.0)
    prob = ba.DeviceEvaluator(matches, kps, True).problem
    base = ba.pack_cameras(cams)
    cs = np.array([0, 4, 8, -1, 9], np.int32)
    npar = np.array([4, 4, 1, 0, 4], np.int32)
    prob.normal_eqns(base, base, cs, npar, 13, 2.0)  # well formed
    cases = [
        (cs, npar, 14, 2.0),                                              # wrong P for the column map
        (cs, npar, 12, 2.0),                                              # columns beyond P
        (np.array([0, 3, 8, -1, 9], np.int32), npar, 13, 2.0),            # overlapping col_start
        (cs, npar, 13, 0.0),                                              # sigma <= 0
        (cs, npar, 13, -1.0),
        (cs, np.array([4, 4, 2, 0, 4], np.int32), 13, 2.0),               # n_params not 1 / 4
    ]
    for c, p, P, s in cases:
        with pytest.raises(capi.ApsError) as e:
            prob.normal_eqns(base, base, c, p, P, s)
        assert e.value.code == capi.APS_E_ARG, (P, s, e.value)
    st = np.zeros(2)
    z = np.zeros(5 * 12)
    i5 = np.zeros(5, np.int32)
    with pytest.raises(capi.ApsError) as e:  # NULL handle
        capi.check(capi.lib.aps_ba_normal_eqns(None, capi.ptr(z), capi.ptr(z), capi.ptr(i5), capi.ptr(i5), 1, 2.0, 1, 0, None,
                                               None, capi.ptr(st)))
    assert e.value.code == capi.APS_E_ARG
    with pytest.raises(capi.ApsError) as e:  # unsorted pairs
        ba.BaProblem(np.zeros((2, 2)), np.zeros((2, 2)), [0, 1, 2], [(1, 2), (0, 1)], 3)
    assert e.value.code == capi.APS_E_ARG
    with pytest.raises(capi.ApsError) as e:  # i >= j
        ba.BaProblem(np.zeros((1, 2)), np.zeros((1, 2)), [0, 1], [(2, 1)], 3)
    assert e.value.code == capi.APS_E_ARG


# ---- end to end: no intrinsics given ---------------------------------------------------------------------------------------

W, H, SEED, FINEST = 1024, 768, 321, 5.0


def _so3(M):
    U, _, Vt = np.linalg.svd(M)
    R = U @ Vt
    return R if np.linalg.det(R) > 0 else U @ np.diag([1, 1, -1.0]) @ Vt


def _angle_deg(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))


@pytest.mark.parametrize("F", [1100.0, 800.0])
def test_stitch_without_intrinsics_shows_the_world(gpu, F):
    """4 x 2 views at 1024 x 768, pl.stitch with neither Ks nor cameras.  Measured on the MI355X (F = 1100 / 800):
    focal error 7e-5 / 4.4e-4 relative, rotation error 0.0048 / 0.0136 deg after the one aligning rotation, RMSE
    0.192 -> 0.179 / 0.230 -> 0.214 px, 344 / 201 LM evaluations, PSNR 55.7 / 53.0 dB.  Bounds (BOUNDS) are at least 3x
    those: focal 2e-3, rotation 0.05 deg, PSNR 48 dB (a 3x larger mean squared error than measured)."""
    synth = import_module(gpu.__name__ + ".synth")
    pl = import_module(gpu.__name__ + ".pipeline")
    rp = import_module(gpu.__name__ + ".renderPanorama")
    imgs, cams = synth.make_scene(4, 2, W, H, F, overlap=0.45, seed=SEED, device="cuda", finest_px=FINEST)
    inp = pl.default_input(bands=3)
    panos, info = pl.stitch(inp, imgs, tile=(1024, 1024), seed=1)
    assert len(panos) == 1 and info["n_components"] == 1
    assert "bundle_adjustment" in info["times"] and len(info["ba"]) == 1
    st = info["ba"][0]
    comp = info["components"][0]
    members, est = comp["members"], comp["cameras"]
    assert len(members) == 8 and st["noRotation"] == 0
    ferr = max(abs(c["f"] / F - 1) for c in est)
    A_k = [np.asarray(cams[k]["R"]).T @ np.asarray(e["R"]) for k, e in zip(members, est)]
    A = _so3(np.mean(A_k, axis=0))
    rerr = max(_angle_deg(a @ A.T) for a in A_k)
    opts = {"anglePower": 2, "blending": "multiband", "pyrLevels": 3, "pyrSigma": inp["MBBsigma"], "canvasColor": "black",
            "tile": (1024, 1024), "cropBorder": False}
    pano, _, cov, geo = rp.renderPanorama(inp, [imgs[k] for k in members], [(H, W, 3)] * len(members), est, "spherical",
                                          comp["ref"], opts, return_covered=True, device_out=True)
    pano, cov = pano.cpu().numpy().astype(np.float64), cov.cpu().numpy() > 0
    ys, xs = np.mgrid[0:geo["H"], 0:geo["W"]]
    a, b = geo["o0"] + xs / geo["fPan"], geo["o1"] + ys / geo["fPan"]
    d = np.stack([np.cos(b) * np.sin(a), np.sin(b), np.cos(b) * np.cos(a)], -1) @ A.T
    truth = synth.world_color(torch.tensor(d, dtype=torch.float32, device="cuda"), F, SEED, finest_px=FINEST)
    truth = (truth * 255.0).cpu().numpy().astype(np.float64)
    from scipy import ndimage

    inside = ndimage.binary_erosion(cov, structure=np.ones((15, 15), bool))
    assert inside.sum() > 0.5 * cov.sum() > 0
    diff = np.abs(pano - truth)[inside]
    psnr = 10 * np.log10(255.0 ** 2 / float((diff ** 2).mean()))
    print("F=%g: f %s (init %.2f), max rotation error %.4f deg, rmse %.4f -> %.4f, %d evaluations, PSNR %.2f dB, BA %.3f s" % (
        F, [round(c["f"], 2) for c in est], st["f_init"], rerr, st["rmse_init"], st["rmse_final"], st["evaluations"], psnr,
        info["times"]["bundle_adjustment"]))
    assert st["rmse_final"] <= st["rmse_init"]
    assert ferr < BOUNDS["f_rel"], ferr
    assert rerr < BOUNDS["rot_deg"], rerr
    assert psnr > BOUNDS["psnr_db"], psnr


BOUNDS = {"f_rel": 2e-3, "rot_deg": 0.05, "psnr_db": 48.0}


def test_planar_scan_takes_the_chained_homographies(gpu):
    """forcePlanarScan: the cameras come back with noRotation = 1 and H2refined = H2seed, and the planar-scan renderer
    composes them."""
    synth = import_module(gpu.__name__ + ".synth")
    pl = import_module(gpu.__name__ + ".pipeline")
    imgs, _ = synth.make_scene(3, 1, 640, 480, 700.0, overlap=0.5, seed=77, device="cpu", finest_px=4.0)
    imgs = [np.asarray(im) for im in imgs]
    inp = pl.default_input(bands=2, forcePlanarScan=True)
    panos, info = pl.stitch(inp, imgs, tile=(1024, 1024), seed=1, device_out=False)
    assert len(panos) == 1 and info["ba"][0]["noRotation"] == 1 and info["ba"][0]["evaluations"] == 0
    cams = info["components"][0]["cameras"]
    assert all(c["noRotation"] == 1 and np.asarray(c["H2refined"]).shape == (3, 3) for c in cams)
    ref = info["components"][0]["ref"]
    assert np.allclose(cams[ref]["H2refined"], np.eye(3))
    pano = np.asarray(panos[0])
    assert pano.dtype == np.uint8 and pano.ndim == 3 and pano.shape[1] > 640 and (pano > 0).mean() > 0.5


def test_bench_scene_estimation_speed(gpu, ba):
    """The 64 x 4K bench scene: the estimation once (after features and matching), with its wall time, LM evaluations and
    the device time per aps_ba_normal_eqns call; then one evaluation at the final cameras through the device problem and
    through the host mirror (device blocks + the host assembly loop), which must agree bit for bit.
    Measured on the MI355X: 9.6 s, 8793 LM evaluations, 64 us of device time per call (blocks 20 + assembly 44), one
    evaluation 0.74 ms on the device problem against 12.2 ms through the host mirror (P = 253).  The scene's f = 8000
    lies outside the reference's focal clamp [100, 5000] (applyIncrements), so the estimate there ends at f = 5000
    (RMSE 27.7 -> 13.4 px): this test reports speed, not accuracy."""
    synth = import_module(gpu.__name__ + ".synth")
    pl = import_module(gpu.__name__ + ".pipeline")
    capi = gpu._capi
    w, h, f, ov, seed, finest = 3840, 2160, 8000.0, 0.40, 12345, 16.0
    cams = synth.grid_cameras(8, 8, w, h, f, 2 * np.arctan(w / (2 * f)) * (1 - ov), 2 * np.arctan(h / (2 * f)) * (1 - ov), 1.0, seed)
    imgs = [synth.render_view(cams[i], h, w, seed, "cuda", finest_px=finest) for i in range(64)]
    torch.cuda.synchronize()
    inp = pl.default_input(bands=5)
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
    tb, nb = capi.profile_get("ba_normal_blocks")
    ta, na = capi.profile_get("ba_normal_assemble")
    capi.profile_enable(False)
    st = ba_info[0]
    assert len(comps) == 1 and len(comps[0]["members"]) == 64 and st["noRotation"] == 0
    assert na == st["evaluations"] + 1 and st["rmse_final"] <= st["rmse_init"]
    # one evaluation, device problem against the host mirror, at the final cameras
    est = comps[0]["cameras"]
    loc = {k: q for q, k in enumerate(comps[0]["members"])}
    matches = [[None] * 64 for _ in range(64)]
    for p, (i, j) in enumerate(res["pairs"]):
        matches[loc[i]][loc[j]] = ba.subsampleMatches(res["inliers"][p], est[loc[i]], est[loc[j]], inp["MaxMatches"])
    kl = [np.asarray(kps[k], np.float64) for k in comps[0]["members"]]
    for c in est:
        c["cx"], c["cy"] = c["K"][0, 2], c["K"][1, 2]
    camList = st["camList"]
    Phi, pmap = ba.buildDeltaVector(est, camList, comps[0]["ref"] if comps[0]["ref"] in camList else camList[0])
    dev = ba.DeviceEvaluator(matches, kl, True)
    host = ba.HostEvaluator(matches, kl, True)
    dev(Phi, pmap, est, camList, pmap[0]["camIdx"], 2.0, True)  # warm
    t0 = time.perf_counter()
    Hd, gd, Ed, rd = dev(Phi, pmap, est, camList, pmap[0]["camIdx"], 2.0, True)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    Hh, gh, Eh, rh = host(Phi, pmap, est, camList, pmap[0]["camIdx"], 2.0, True)
    t_host = time.perf_counter() - t0
    assert np.array_equal(_bits(Hd), _bits(Hh)) and np.array_equal(_bits(gd), _bits(gh)) and _bits(Ed) == _bits(Eh)
    print("bench scene: estimation %.3f s, f %.1f (init %.1f), rmse %.3f -> %.3f px, %d LM evaluations, device %.1f us per "
          "aps_ba_normal_eqns (blocks %.1f + assembly %.1f), one evaluation %.2f ms on the device problem vs %.2f ms through "
          "the host mirror, P = %d" % (
              wall, np.median(st["focals"]), st["f_init"], st["rmse_init"], st["rmse_final"], st["evaluations"],
              1e3 * (tb + ta) / max(na, 1), 1e3 * tb / max(nb, 1), 1e3 * ta / max(na, 1), 1e3 * t_dev, 1e3 * t_host,
              Hd.shape[0]))
