"""GPU parity of device SIFT with the oracle across the parameter space: the arms of aps_sift_extract's dispatch that the
default parameter set never enters (sift_param_cases.py names them; test_sift_param_cases.py holds each case to its arm),
and the capacity paths of the C entry and of featureMatching.sift_extract.

Every comparison is exact: locations equal, aux and descriptors equal as uint32 (tolerance 0, as in test_sift_gpu.py - both
sides were written to one evaluation order).  The keypoint-count floors are half the oracle's counts on the CPU
(sift_param_cases.CASES), so that no case passes on an empty or near-empty result."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import sift_param_cases as sc
from util import fetch, place, same_bits, sentinel_buffer

pytestmark = pytest.mark.gpu

DEFAULT = (1.6, 4, 0.00133, 6.0)
INPUT = {"detector": "SIFT", "Sigma": 1.6, "NumLayersInOctave": 4, "ContrastThreshold": 0.00133, "EdgeThreshold": 6}


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


@pytest.fixture(scope="module")
def capi(gpu):
    return gpu._capi


def assert_equals_oracle(got, want):
    """(features, points, aux) against oracle.sift's (desc, loc, aux), bit for bit; aux is optional on the device side."""
    f, pts = got[0], got[1]
    od, ol, oa = want
    assert f.shape == od.shape and f.shape[1:] == (128,)
    assert pts.shape == ol.shape and np.array_equal(pts, ol)
    if len(got) > 2:
        assert np.array_equal(np.ascontiguousarray(got[2]).view(np.uint32), oa.view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(f).view(np.uint32), od.view(np.uint32))


# ---- 1. the parameter matrix ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", sc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id)
def test_parameter_matrix_bit_exact_rgb(fm, case, hw):
    h, w = hw
    want = sc.oracle_sift("rgb", h, w, sc.params(case))
    floor = case.counts[sc.SHAPES.index(hw)]
    assert 2 * len(want[0]) >= floor, (len(want[0]), floor)
    if "descr>63" in case.arms:
        r, _ = sc.descr_radius(want[2])
        assert (r > sc.DESCR_QUEUED_MAX).sum() >= 5, "too few keypoints take the descriptor's plain sweep"
    got = fm.sift_extract(sc.as_input(case), sc.image(h, w), want_aux=True)
    if floor == 0:
        assert got[0].shape == (0, 128) and got[1].shape == (0, 2) and got[2].shape == (0, 4)
    assert_equals_oracle(got, want)


def test_parameter_matrix_gray(fm):
    """One channel through gray_up_kernel (no fused base kernel at this Sigma) and the large-scale arms."""
    case = sc.BY_ID[sc.GRAY_CASE]
    h, w = sc.SHAPES[0]
    want = sc.oracle_sift("gray", h, w, sc.params(case))
    assert 2 * len(want[0]) >= sc.GRAY_COUNT
    assert_equals_oracle(fm.sift_extract(sc.as_input(case), sc.gray_image(h, w), want_aux=True), want)


# ---- 4. the same arms where the octaves run out ---------------------------------------------------------------------------
@pytest.mark.parametrize("hw", list(sc.SMALL_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_large_scales_on_small_images(fm, hw):
    """Sigma = 3.2 on images whose upper octaves are smaller than 2 kBorder (skipped by the sweep, still blurred and
    decimated) and where the descriptor's square is larger than the plane: 37 x 37 has a keypoint whose radius exceeds its
    octave's diagonal, the other two have radii above 63 on planes 36 and 70 rows high."""
    h, w = hw
    case = sc.BY_ID[sc.SMALL_CASE]
    want = sc.oracle_sift("rgb", h, w, sc.params(case))
    assert len(want[0]) >= 5 and 2 * len(want[0]) >= sc.SMALL_SHAPES[hw]
    r, octave = sc.descr_radius(want[2])
    if hw == (37, 37):
        assert (r > sc.octave_diag(h, w, octave)).sum() >= 1
    else:
        assert (r > sc.DESCR_QUEUED_MAX).sum() >= 2
    assert_equals_oracle(fm.sift_extract(sc.as_input(case), sc.image(h, w), want_aux=True), want)


# ---- 3. capacity paths ------------------------------------------------------------------------------------------------------
def _raw(capi, img, prm, cap, where="host"):
    """aps_sift_extract, row-major and tight, into sentinel-filled outputs of `cap` rows.
    Returns (rc, count, desc [cap,128], loc [cap,2], aux [cap,4]) - everything past the count must still be the sentinel."""
    import torch

    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    desc = place(sentinel_buffer(max(cap, 1) * 128, np.float32), where)
    loc = place(sentinel_buffer(2 * max(cap, 1), np.float64), where)
    aux = place(sentinel_buffer(4 * max(cap, 1), np.float32), where)
    cnt = C.c_int64(-1)
    torch.cuda.synchronize()
    rc = capi.lib.aps_sift_extract(capi.ptr(np.ascontiguousarray(img)), h, w, c, capi.APS_IMG_U8_HWC, C.byref(prm), capi.ptr(desc),
                                   capi.APS_ROWMAJOR, 128, capi.ptr(loc), max(cap, 1), capi.ptr(aux), cap, C.byref(cnt))
    capi.check(capi.lib.aps_synchronize())
    return rc, int(cnt.value), fetch(desc).reshape(-1, 128), fetch(loc).reshape(2, -1).T, fetch(aux).reshape(-1, 4)


def _all_sentinel(*arrays):
    return all(same_bits(a.reshape(-1), sentinel_buffer(a.size, a.dtype)) for a in (np.ascontiguousarray(x) for x in arrays))


def test_max_features_too_small_is_an_error_that_writes_nothing(fm, gpu, capi):
    h, w = sc.SHAPES[0]
    img = sc.image(h, w)
    want = sc.oracle_sift("rgb", h, w, DEFAULT)
    assert len(want[0]) > 8
    with pytest.raises(gpu.ApsError, match="max_features") as err:
        fm.sift_extract(dict(INPUT, maxFeatures=8), img)
    assert err.value.code == capi.APS_E_CAP
    for where in ("host", "device"):
        rc, n, desc, loc, aux = _raw(capi, img, capi.aps_sift_params(*DEFAULT, 8), 4096, where)
        assert rc == capi.APS_E_CAP and n == 0
        assert b"max_features" in capi.lib.aps_last_error()
        assert _all_sentinel(desc, loc, aux), "an extraction that failed on max_features wrote into the caller's outputs"
    # the error leaves nothing behind: the next call with default parameters is the oracle's result
    assert_equals_oracle(fm.sift_extract(INPUT, img, want_aux=True), want)


def test_max_features_large_enough_changes_nothing(fm):
    h, w = sc.SHAPES[0]
    want = sc.oracle_sift("rgb", h, w, DEFAULT)
    assert_equals_oracle(fm.sift_extract(dict(INPUT, maxFeatures=100000), sc.image(h, w), want_aux=True), want)


def test_raw_capacity_too_small_reports_the_count_and_the_retry_matches(capi):
    h, w = sc.SHAPES[0]
    img = sc.image(h, w)
    od, ol, oa = sc.oracle_sift("rgb", h, w, DEFAULT)
    prm = capi.aps_sift_params(*DEFAULT, 0)
    rc, n, desc, loc, aux = _raw(capi, img, prm, 8)
    assert rc == capi.APS_E_CAP and n == len(od) > 8
    assert _all_sentinel(desc, loc, aux), "a call that reports APS_E_CAP wrote into outputs that are too small"
    rc, n2, desc, loc, aux = _raw(capi, img, prm, n)
    assert rc == 0 and n2 == n
    assert_equals_oracle((desc, loc, aux), (od, ol, oa))


@pytest.mark.parametrize("mode", ["host", "device_out", "device_points_compact"])
def test_wrapper_grows_its_capacity_and_retries(fm, mode):
    """6367 features on 300 x 400, first capacity max(4096, h w / 64) = 4096: the first call reports APS_E_CAP with the
    count, the wrapper allocates that many rows and calls again."""
    img = sc.dense_image()
    od, ol, oa = sc.oracle_sift("dense", 0, 0, DEFAULT)
    assert len(od) > max(4096, img.shape[0] * img.shape[1] // 64)
    if mode == "host":
        got = fm.sift_extract(INPUT, img, want_aux=True)
    else:
        more = dict(points_device=True, compact=True) if mode == "device_points_compact" else {}
        f, pts, aux = fm.sift_extract(INPUT, img, device_out=True, want_aux=True, **more)
        assert f.is_cuda and (mode == "device_out" or pts.is_cuda)
        if mode == "device_points_compact":
            assert f.shape[0] * f.shape[1] == f.untyped_storage().nbytes() // 4, "compact=True returns a right-sized buffer"
            pts = pts.cpu().numpy()
        got = (f.cpu().numpy(), pts, aux)
    assert_equals_oracle(got, (od, ol, oa))
