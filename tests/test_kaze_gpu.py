"""Device KAZE against the NumPy mirror of the contract (tests/kaze_mirror.py), bit for bit: the keypoint set and order, loc as
uint64, aux scale / metric / level as uint32, descriptors as uint32.  angle_deg alone passes through atan2f and may differ by
1e-3 degrees.  Shapes are the smallest at which each kernel can go wrong (see the table in kaze_cases.CASES)."""
import ctypes as C
import threading
from importlib import import_module

import numpy as np
import pytest

import kaze_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_matches_mirror(d, loc, aux, md, mloc, maux):
    assert d.shape == md.shape and loc.shape == mloc.shape, (d.shape, md.shape)
    assert d.dtype == np.float32 and loc.dtype == np.float64
    assert np.array_equal(np.ascontiguousarray(loc).view(np.uint64), np.ascontiguousarray(mloc).view(np.uint64)), "loc bits / keypoint order"
    for col, what in ((0, "scale"), (2, "metric"), (3, "level")):
        assert np.array_equal(u32(aux[:, col]), u32(maux[:, col])), what
    da = np.abs((aux[:, 1].astype(np.float64) - maux[:, 1].astype(np.float64) + 180.0) % 360.0 - 180.0)
    assert da.size == 0 or da.max() <= 1e-3, da.max()
    assert np.array_equal(u32(d), u32(md)), "descriptor bits (%d rows differ)" % int((u32(d) != u32(md)).any(1).sum())


@pytest.mark.parametrize("name", list(kc.CASES))
def test_device_equals_mirror(fm, name):
    img, kw, md, mloc, maux = kc.mirror(name)
    assert len(md) >= 10, "the case must have keypoints to compare"
    if name == "many":
        assert len(md) >= 2000
    if name == "O4S4":
        assert maux[:, 3].max() >= 10   # (keypoints up to the fourth octave's levels, whose derivative tiles have the widest halos)
    d, loc, aux = fm.kaze_extract(dict(kw, detector="KAZE"), img, want_aux=True)
    assert_matches_mirror(d, loc, aux, md, mloc, maux)


def _raw(gpu, img, cap, ldd, fill=np.float32(-7.5)):
    capi = gpu._capi
    prm = capi.aps_kaze_params(1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_REGION, 0)
    desc = np.full((max(cap, 1), ldd), fill, np.float32)
    loc = np.zeros((2, max(cap, 1)), np.float64)
    aux = np.zeros((max(cap, 1), 4), np.float32)
    cnt = C.c_int64(-1)
    img = np.ascontiguousarray(img)
    rc = capi.lib.aps_kaze_extract(capi.ptr(img), img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, capi.APS_IMG_U8_HWC, C.byref(prm),
                                   capi.ptr(desc), capi.APS_ROWMAJOR, ldd, capi.ptr(loc), max(cap, 1), capi.ptr(aux), cap, C.byref(cnt))
    return rc, cnt.value, desc, loc, aux


def test_capacity_too_small_reports_the_count_and_the_retry_matches(gpu):
    img, kw, md, mloc, maux = kc.mirror("pairA")
    rc, n, desc, *_ = _raw(gpu, img, 8, 64)
    assert rc == gpu._capi.APS_E_CAP and n == len(md)
    assert (desc == np.float32(-7.5)).all(), "nothing is written when the rows do not fit"
    capi = gpu._capi
    cnt = C.c_int64(-1)   # count-only mode: NULL outputs
    prm = capi.aps_kaze_params(1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_REGION, 0)
    rc = capi.lib.aps_kaze_extract(capi.ptr(np.ascontiguousarray(img)), img.shape[0], img.shape[1], 1, capi.APS_IMG_U8_HWC, C.byref(prm), None,
                                   capi.APS_ROWMAJOR, 64, None, 0, None, 0, C.byref(cnt))
    assert cnt.value == len(md) and rc == capi.APS_E_CAP
    rc, n2, desc, loc, aux = _raw(gpu, img, n, 64)
    assert rc == 0 and n2 == n
    assert_matches_mirror(desc[:n], np.ascontiguousarray(loc[:, :n].T), aux[:n], md, mloc, maux)


def test_leading_dimension_128_is_zero_padded_and_64_stays_inside(gpu):
    img, kw, md, _, _ = kc.mirror("97x131")
    n = len(md)
    rc, cnt, desc, _, _ = _raw(gpu, img, n + 3, 128)
    assert rc == 0 and cnt == n
    assert np.array_equal(u32(desc[:n, :64]), u32(md)) and not desc[:n, 64:].any()
    assert (desc[n:] == np.float32(-7.5)).all(), "rows beyond the count belong to the caller"
    rc, cnt, desc, _, _ = _raw(gpu, img, n + 3, 80)   # 64 <= ldd < 128: nothing beyond column 63
    assert rc == 0 and np.array_equal(u32(desc[:n, :64]), u32(md))
    assert (desc[:, 64:] == np.float32(-7.5)).all() and (desc[n:] == np.float32(-7.5)).all()
    rc, cnt, desc, _, _ = _raw(gpu, img, n, 64)
    assert rc == 0 and np.array_equal(u32(desc), u32(md))


def test_two_calls_and_four_threads_give_identical_bytes(fm):
    img = kc.mirror("pairA")[0]
    inp = {"detector": "KAZE"}
    ref = fm.kaze_extract(inp, img, want_aux=True)
    again = fm.kaze_extract(inp, img, want_aux=True)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(ref, again))
    got = [None] * 4

    def work(k):
        got[k] = fm.kaze_extract(inp, img, want_aux=True)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for g in got:
        assert g is not None and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(ref, g))


def test_too_small_image_and_resident_rows(fm):
    import torch

    f0, p0 = fm.kaze_extract({"detector": "KAZE"}, np.full((28, 300), 9, np.uint8))   # below level 1's margin: 2 * 14 + 1 rows
    assert f0.shape == (0, 64) and p0.shape == (0, 2) and f0.dtype == np.float32
    img, kw, md, mloc, _ = kc.mirror("97x131")
    res, pts = fm.kaze_extract({"detector": "KAZE"}, torch.from_numpy(np.array(img)).cuda(), device_out=True)
    assert res.shape[1] == 64 and res.stride(0) == 128 and np.array_equal(u32(res.cpu().numpy()), u32(md))
    full, _ = fm.extract_features({"detector": "KAZE"}, torch.from_numpy(np.array(img)).cuda(), device_out=True)
    assert full.shape[1] == 128 and not bool(full[:, 64:].any()) and np.array_equal(u32(full[:, :64].cpu().numpy()), u32(md))
    assert np.array_equal(np.asarray(pts).view(np.uint64), np.ascontiguousarray(mloc).view(np.uint64))
    with pytest.raises(NotImplementedError):
        fm.getFeaturePoints(dict(detector="KAZE"), img)


def test_matlab_layouts_give_the_same_features(gpu):
    """The layouts a MATLAB caller has: planar column-major image (APS_IMG_U8_MATLAB), column-major descriptors (APS_COLMAJOR)
    with a leading dimension above the count; elements between the columns stay the caller's."""
    capi = gpu._capi
    img, kw, md, mloc, _ = kc.mirror("131x97x3")
    n, h, w = len(md), img.shape[0], img.shape[1]
    planar = np.ascontiguousarray(img.transpose(2, 1, 0))   # [c][x][y]: MATLAB's h x w x 3 in memory
    ld = n + 5
    prm = capi.aps_kaze_params(1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_REGION, 0)
    desc = np.full((64, ld), np.float32(-7.5), np.float32)   # column-major ld x 64
    loc = np.full((2, ld), -7.5, np.float64)
    cnt = C.c_int64(0)
    rc = capi.lib.aps_kaze_extract(capi.ptr(planar), h, w, 3, capi.APS_IMG_U8_MATLAB, C.byref(prm), capi.ptr(desc), capi.APS_COLMAJOR, ld,
                                   capi.ptr(loc), ld, None, ld, C.byref(cnt))
    assert rc == 0 and cnt.value == n
    assert np.array_equal(u32(desc[:, :n].T), u32(md)) and (desc[:, n:] == np.float32(-7.5)).all()
    assert np.array_equal(np.ascontiguousarray(loc[:, :n].T).view(np.uint64), np.ascontiguousarray(mloc).view(np.uint64)) and (loc[:, n:] == -7.5).all()
