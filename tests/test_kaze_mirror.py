"""CPU tests that pin the NumPy mirror of the KAZE contract (tests/kaze_mirror.py) by analytic cases, so that a device that
equals the mirror bit for bit (tests/test_kaze_gpu.py) computes KAZE and not merely the mirror's mistakes."""
import math

import numpy as np

import kaze_cases as kc
import kaze_mirror as km

f32 = np.float32


def test_level_tables():
    lv = km.levels(3, 4)
    assert lv["n"] == 12 and lv["step"] == [2, 2, 2, 3, 3, 4, 5, 5, 6, 8, 9, 11]
    assert abs(lv["sigma64"][4] - 3.2) < 1e-12 and abs(lv["sigma64"][8] - 6.4) < 1e-12
    assert lv["margin"][1] == math.ceil(5 * 1.6 * 2 ** 0.5) + 2 == 14
    for g, r in ((km.G_BASE, 7), (km.G_ONE, 4)):
        assert len(g) == r + 1 and abs(float(g[0]) + 2.0 * float(g[1:].astype(np.float64).sum()) - 1.0) < 1e-6 and (np.diff(g) < 0).all()


def test_constant_and_axis_ramps_give_exactly_zero_response_and_no_keypoint():
    """A constant plane stays constant through every blur and diffusion step (every pixel sees the same operands), so every
    difference of the Scharr pair is exactly zero.  A ramp along one axis keeps identical rows (columns) through the chain, so
    Ly, Lxy and Lyy (Lx, Lxy and Lxx) are exact zeros and the determinant, Lxx * Lyy - Lxy * Lxy, is 0 * Lxx - 0 = 0 whatever the
    clamped border does to Lxx.  The diagonal ramp x + y is not exact in f32: g / 255 is rounded, so the second differences are
    rounding noise and not zero.  Away from the border's kink (levels 0..6 at the centre of 120 x 120) that noise is bounded by
    1e-9: eps = 6e-8 relative on values below 1 through the blur gives about 3e-7 absolute, a second derivative at step s about
    1e-6 / s^2, the determinant times sigma^4 about 1e-11.  No keypoint in any of them."""
    yy, xx = np.mgrid[0:80, 0:90]
    for g in (np.full((80, 90), 77), xx * 2, yy * 3):
        assert g.max() <= 255
        lv, LX, LY, RR = km.scale_space(g.astype(np.uint8))
        assert all(not r.any() for r in RR)
        assert km.extract(g.astype(np.uint8))[0].shape == (0, 64)
    const = km.scale_space(np.full((80, 90), 77, np.uint8))
    assert all(not p.any() for p in const[1]) and all(not p.any() for p in const[2])
    yy, xx = np.mgrid[0:120, 0:120]
    diag = (xx + yy).astype(np.uint8)
    assert (xx + yy).max() <= 255
    lv, LX, LY, RR = km.scale_space(diag)
    assert max(abs(float(RR[i][60, 60])) for i in range(7)) <= 1e-9
    assert km.extract(diag)[0].shape == (0, 64)


def test_flat_image_falls_back_to_the_stated_contrast_factor():
    assert km.contrast_factor(np.full((40, 50), f32(0.3), f32)) == f32(0.03)
    k = km.contrast_factor(kc.pair()[0].astype(f32) * f32(1.0 / 255.0))
    assert 0.0 < float(k) < 1.0


def test_fed_cycles_cover_their_time_and_are_never_empty():
    """sum tau_j = t_{i+1} - t_i to f64 rounding, and the order of application is a permutation of the natural order."""
    for O in (1, 2, 3, 4):
        for S in (3, 4, 7, 10):
            lv = km.levels(O, S)
            for i in range(lv["n"] - 1):
                T = km.cycle_time(lv, i)
                assert abs(T - (lv["sigma64"][i + 1] ** 2 - lv["sigma64"][i] ** 2) / 2.0) <= 1e-12 * T
                order, natural = km.fed_taus(T)
                assert len(order) >= 1 and sorted(order) == sorted(natural) and min(natural) > 0
                assert abs(math.fsum(order) - T) <= 1e-12 * T, (O, S, i)


def test_one_diffusion_step_on_an_impulse_is_the_five_point_heat_stencil():
    one = np.ones((9, 11), f32)
    for tau in (0.25, 0.125):
        L = np.zeros((9, 11), f32)
        L[4, 5] = 1
        out = km.fed_step(L, one, f32(0.5 * tau))
        want = np.zeros((9, 11), f32)
        want[4, 5] = 1 - 4 * tau
        want[3, 5] = want[5, 5] = want[4, 4] = want[4, 6] = tau
        assert np.array_equal(out, want)
    corner = np.zeros((9, 11), f32)   # no flux through the border: the mass stays
    corner[0, 0] = 1
    out = km.fed_step(corner, one, f32(0.125))
    assert out[0, 0] == 0.5 and out[0, 1] == 0.25 and out[1, 0] == 0.25 and out.sum() == 1


def test_single_dark_blob_gives_keypoints_only_at_its_centre_and_at_its_scale():
    """A dark Gaussian blob, sigma = 4 px, 40 gray levels deep, centred on pixel (64, 64) of a 128 x 128 field.  Nearly all of the
    field is flat, so the contrast factor (the 70th percentile of the gradient) is small, the blob's rim hardly diffuses, and the
    response over the levels follows the derivative step: round(sigma_i) is 2, 2, 2, 3, 3, 4, 5, 5, ... and the response rises
    within a run of one step (sigma^4 grows) and falls where the step grows.  At the default Threshold the mirror therefore finds
    the centre twice, on levels 4 and 7 (responses 1.2456e-3 and 1.4789e-3, scales 3.40 and 5.45), and nothing anywhere else.
    As test_surf_mirror does with its amplitude, the scale check is made where only the best-fitting level is above the
    threshold: Threshold = 1.3e-3, between the two, leaves the level that maximises the mirror's own centre response (scanned
    over all levels: level 7), and its scale lies within one sublevel ratio 2^(1/4) of that level's sigma."""
    img = kc.blob(40.0)
    lv, LX, LY, RR = km.scale_space(img)
    centre = [float(r[64, 64]) for r in RR]
    best = int(np.argmax(centre))
    assert best == 7
    desc, loc, aux = km.extract(img)
    assert len(desc) == 2 and np.hypot(loc[:, 0] - 65.0, loc[:, 1] - 65.0).max() <= 0.5   # 1-based centre
    assert list(aux[:, 3]) == [4.0, 7.0] and (aux[:, 2] > 1e-4).all()
    assert np.abs(np.linalg.norm(desc.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    desc, loc, aux = km.extract(img, Threshold=1.3e-3)
    assert desc.shape == (1, 64) and np.hypot(loc[0, 0] - 65.0, loc[0, 1] - 65.0) <= 0.5
    ratio = float(aux[0, 0]) / lv["sigma64"][best]
    assert 2.0 ** -0.25 <= ratio <= 2.0 ** 0.25, ratio
    assert aux[0, 2] == f32(centre[best])


def test_quarter_turn_of_the_image():
    """np.rot90 is an exact resampling: pixel (y, x) goes to (w-1-x, y).  The diffusion step, the Scharr pair and the detection
    are written symmetrically; the separable blur runs rows first, which a quarter turn makes columns first, so the planes of
    the turned image differ by rounding.  Keypoints map one to one within 1e-3 px (position + scale), the angle turns by 90
    degrees within 1e-3 and the oriented descriptor, expressed in the keypoint's own frame, is equal within 1e-5."""
    img = kc.oriented_patch()
    rot = np.ascontiguousarray(np.rot90(img))
    h, w = img.shape
    d0, l0, a0 = km.extract(img)
    d1, l1, a1 = km.extract(rot)
    assert len(d0) == len(d1) >= 50
    mapped = np.stack([l0[:, 1], w + 1.0 - l0[:, 0]], 1)   # (x, y) 1-based -> (y, w + 1 - x)
    taken = set()
    for k in range(len(d0)):
        dist = np.hypot(*(l1 - mapped[k]).T) + np.abs(a1[:, 0] - a0[k, 0])
        q = int(np.argmin(dist))
        assert dist[q] <= 1e-3 and q not in taken, (k, dist[q])
        taken.add(q)
        assert a1[q, 3] == a0[k, 3] and abs(a1[q, 2] - a0[k, 2]) <= 1e-3 * a0[k, 2]
        # image y points down: the counter-clockwise quarter turn of the picture takes the angle from t to t - 90
        da = (a0[k, 1] - a1[q, 1] - 90.0 + 180.0) % 360.0 - 180.0
        assert abs(da) <= 1e-3, (k, a0[k, 1], a1[q, 1])
        assert np.abs(d1[q] - d0[k]).max() <= 1e-5, (k, np.abs(d1[q] - d0[k]).max())


def test_image_below_the_margin_of_level_one_gives_nothing():
    for shape in ((28, 28), (28, 200), (5, 3)):
        d, l, a = km.extract(np.random.default_rng(3).integers(0, 256, shape).astype(np.uint8))
        assert d.shape == (0, 64) and l.shape == (0, 2) and a.shape == (0, 4)


def test_frozen_pair_verifies_under_the_reference_acceptance_rule():
    """Image A: surf_cases' 240 x 320 band-limited noise; B: A under PAIR_H, bilinear.  Brute-force ratio test at 0.6; a match
    is correct when its transfer error under the known homography is below maxDistance = 5.5 px; imageMatching.m:150 accepts a
    pair with more than 8 + 0.3 * nf inliers.  The pair's texture is surf_cases' unchanged and the Threshold is the default:
    the mirror finds 1090 and 1082 keypoints, 838 ratio matches, all 838 correct, against 259.4."""
    A, B = kc.pair()
    assert A.shape == (240, 320)
    dA, lA, _ = km.extract(A)
    dB, lB, _ = km.extract(B)
    m = kc.ratio_matches(dA, dB, 0.6)
    nf = len(m)
    correct = int((kc.transfer_error(lA[m[:, 0]], lB[m[:, 1]]) < 5.5).sum())
    assert nf >= 50 and correct >= 8 + 0.3 * nf, (nf, correct)
