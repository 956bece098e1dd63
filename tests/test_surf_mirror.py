"""CPU tests that pin the NumPy mirror of the SURF contract (tests/surf_mirror.py) by analytic cases, so that a device
that equals the mirror bit for bit (tests/test_surf_gpu.py) computes SURF and not merely the mirror's mistakes."""
import numpy as np

import surf_cases as sc
import surf_mirror as sm


def test_integral_image_is_cumsum_of_cumsum():
    g = np.random.default_rng(0).integers(0, 256, (37, 53))
    I = sm.integral(g)
    assert I.shape == (38, 54) and not I[0].any() and not I[:, 0].any()
    assert np.array_equal(I[1:, 1:], g.cumsum(0).cumsum(1))
    assert sm.box(I, 3, 9, 5, 20) == g[3:10, 5:21].sum()
    rgb = np.random.default_rng(1).integers(0, 256, (8, 9, 3)).astype(np.uint8)
    gray = sm.gray_plane(rgb)
    assert gray.min() >= 0 and gray.max() <= 255 and np.abs(gray - rgb @ [0.298936021293775, 0.587043074451121, 0.114020904255103]).max() <= 0.5


def test_responses_of_a_constant_and_of_a_linear_ramp_are_exactly_zero():
    yy, xx = np.mgrid[0:80, 0:90]
    for g in (np.full((80, 90), 77), xx + yy):   # (the ramp stays within 0..255)
        assert g.max() <= 255
        I = sm.integral(g)
        for o in (1, 2):
            for lv in range(4):
                S = sm.filter_size(o, lv)
                b = (S - 1) // 2
                ys, xs = np.arange(b, 80 - b)[:, None], np.arange(b, 90 - b)[None, :]
                if ys.size == 0:
                    continue
                det, tr = sm.response(I, ys, xs, S)
                assert not det.any() and not tr.any(), (o, lv)


def test_filter_sizes_and_dropped_octaves():
    assert [[sm.filter_size(o, l) for l in range(4)] for o in (1, 2, 3)] == [[9, 15, 21, 27], [15, 27, 39, 51], [27, 51, 75, 99]]
    assert sm.plan(64, 64) == [1, 2] and sm.plan(240, 320) == [1, 2, 3, 4] and sm.plan(26, 500) == []


def _blob(amplitude):
    yy, xx = np.mgrid[0:128, 0:128]
    return np.round(200.0 - amplitude * np.exp(-((xx - 64) ** 2 + (yy - 64) ** 2) / (2.0 * 4.0 ** 2))).astype(np.uint8)


def test_single_dark_blob_gives_one_keypoint_at_its_centre_and_scale():
    """A dark Gaussian blob, sigma = 4 px, centred on pixel (64, 64) of a 128 x 128 field.  SURF's octaves overlap in scale
    (filter 27 belongs to octaves 1, 2 and 3), so a strong blob is a maximum of more than one octave; the amplitude here (40
    gray levels) leaves only the best-fitting level above MetricThreshold = 1000, and the stronger blob below shows the
    overlap.  Expected scale: the filter side that maximises the mirror's own response at the centre, scanned over every
    valid side (multiples of 3 with an odd lobe: 9, 15, 21, ...), times 1.2 / 9; tolerance: one level spacing of octave 1
    (6 px of filter side = 0.8)."""
    img = _blob(40.0)
    I = sm.integral(sm.gray_plane(img))
    sides = list(range(9, 100, 6))
    dense = [float(sm.response(I, 64, 64, S)[0]) for S in sides]
    best_side = sides[int(np.argmax(dense))]
    assert best_side == 21   # the box approximation's optimum for sigma = 4 (1.2 * 21 / 9 = 2.8)
    desc, loc, aux = sm.extract(img)
    assert desc.shape == (1, 64) and loc.shape == (1, 2)
    assert np.hypot(loc[0, 0] - 65.0, loc[0, 1] - 65.0) <= 0.5   # 1-based centre
    assert abs(aux[0, 0] - 1.2 * best_side / 9.0) <= 1.2 * 6 / 9.0
    assert aux[0, 3] == 1.0 and aux[0, 2] > 1000.0
    assert abs(np.linalg.norm(desc[0].astype(np.float64)) - 1.0) <= 1e-6
    strong = sm.extract(_blob(150.0))
    assert len(strong[0]) == 2 and np.abs(strong[1] - 65.0).max() <= 0.5 and (strong[2][:, 3] == 1.0).all()


def _oriented_patch():
    """129 x 129 (sample grids of every octave map onto themselves under a quarter turn: 128 is a multiple of every
    step): band-limited noise plus a few dark blobs, without symmetry."""
    img = sc.band_limited(11, 129, 129, 3.0, contrast=0.8).astype(np.float64)
    yy, xx = np.mgrid[0:129, 0:129]
    for cx, cy, s, a in ((50, 60, 4.0, 70.0), (80, 45, 5.0, -60.0), (70, 85, 3.5, 60.0)):
        img -= a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def test_quarter_turn_of_the_image():
    """np.rot90 is an exact resampling: pixel (y, x) goes to (w-1-x, y).  Keypoints map one to one; the orientation turns by
    90 degrees (1e-3) and the oriented descriptor, expressed in the keypoint's own frame, is unchanged; the upright descriptor
    (frame = image axes) shows the rotation as a permutation of the 4 x 4 sub-regions with (dx, dy, |dx|, |dy|) ->
    (dy, -dx, |dy|, |dx|).  Tolerance 1e-5 absolute: only summation order differs."""
    img = _oriented_patch()
    rot = np.ascontiguousarray(np.rot90(img))
    h, w = img.shape
    for upright in (False, True):
        d0, l0, a0 = sm.extract(img, upright=upright)
        d1, l1, a1 = sm.extract(rot, upright=upright)
        assert len(d0) == len(d1) >= 5
        # (x, y) 1-based -> (y, w + 1 - x); match by nearest position and scale
        mapped = np.stack([l0[:, 1], w + 1.0 - l0[:, 0]], 1)
        for k in range(len(d0)):
            dist = np.hypot(*(l1 - mapped[k]).T) + np.abs(a1[:, 0] - a0[k, 0])
            q = int(np.argmin(dist))
            assert dist[q] <= 1e-3, (k, dist[q])
            assert a1[q, 3] == a0[k, 3] and abs(a1[q, 2] - a0[k, 2]) <= 1e-3 * a0[k, 2]
            if not upright:
                # image y points down: the counter-clockwise quarter turn of the picture takes the angle from t to t - 90
                da = (a0[k, 1] - a1[q, 1] - 90.0 + 180.0) % 360.0 - 180.0
                assert abs(da) <= 1e-3, (k, a0[k, 1], a1[q, 1])
                assert np.abs(d1[q] - d0[k]).max() <= 1e-5, (k, np.abs(d1[q] - d0[k]).max())
            else:
                # rotated frame: u' = v, v' = -u  ->  sub-region (row r', col c') holds the original's (row c', col 3 - r')
                D0 = d0[k].reshape(4, 4, 4)
                exp = np.zeros_like(D0)
                for r in range(4):
                    for c in range(4):
                        s_dx, s_dy, a_dx, a_dy = D0[c, 3 - r]
                        exp[r, c] = (s_dy, -s_dx, a_dy, a_dx)
                assert np.abs(d1[q].reshape(4, 4, 4) - exp).max() <= 1e-5, (k, np.abs(d1[q].reshape(4, 4, 4) - exp).max())


def test_image_below_the_first_octave_support_gives_nothing():
    for shape in ((26, 26), (26, 200), (5, 3)):
        d, l, a = sm.extract(np.random.default_rng(3).integers(0, 256, shape).astype(np.uint8))
        assert d.shape == (0, 64) and l.shape == (0, 2) and a.shape == (0, 4)


def test_frozen_pair_verifies_under_the_reference_acceptance_rule():
    """Image A: 240 x 320 band-limited noise; B: A under surf_cases.PAIR_H, bilinear.  Brute-force ratio test at 0.6; a match
    is correct when its transfer error under the known homography is below maxDistance = 5.5 px; imageMatching.m:150 accepts
    a pair with more than 8 + 0.3 * nf inliers."""
    A, B = sc.pair()
    assert A.shape == (240, 320)
    dA, lA, _ = sm.extract(A)
    dB, lB, _ = sm.extract(B)
    m = sc.ratio_matches(dA, dB, 0.6)
    nf = len(m)
    correct = int((sc.transfer_error(lA[m[:, 0]], lB[m[:, 1]]) < 5.5).sum())
    assert nf >= 50 and correct >= 8 + 0.3 * nf, (nf, correct)
