"""Device SURF against the NumPy mirror of the contract (tests/surf_mirror.py), bit for bit: the keypoint set and order, loc
as uint64, aux scale / metric / sign as uint32, descriptors as uint32.  angle_deg alone passes through atan2f and may
differ by 1e-3 degrees.  Shapes are the smallest at which each kernel can go wrong (see the table in CASES)."""
import ctypes as C
import threading
from importlib import import_module

import numpy as np
import pytest

import surf_cases as sc
import surf_mirror as sm

pytestmark = pytest.mark.gpu

# name: (image builder, MetricThreshold) - what it catches
CASES = {
    "64x64": (lambda: sc.band_limited(1, 64, 64, 2.5), 1000.0),            # one octave, borders everywhere
    "97x131": (lambda: sc.band_limited(2, 97, 131, 2.5), 1000.0),          # odd sizes, tails of every tile and wave
    "131x97x3": (lambda: sc.band_limited(3, 131, 97, 2.5, channels=3), 1000.0),  # RGB path, transposed tails
    "pairA": (lambda: sc.pair()[0], 1000.0),                              # 240 x 320: three octaves
    "48x2100": (lambda: sc.band_limited(4, 48, 2100, 2.5), 1000.0),        # the row scan's carry across 1024-px chunks
    "2100x48": (lambda: sc.band_limited(5, 2100, 48, 2.5), 1000.0),        # the column scan's carry across 64-row chunks
    "600x800": (lambda: sc.band_limited(6, 600, 800, 2.5), 50.0),          # thousands of keypoints: many bitmap words, scan blocks
}
_MIRROR = {}


def mirror(name):
    """The mirror's result for a case, computed once and shared (read-only)."""
    if name not in _MIRROR:
        build, thr = CASES[name]
        img = build()
        out = sm.extract(img, MetricThreshold=thr)
        for a in out:
            a.setflags(write=False)
        _MIRROR[name] = (img, thr) + out
    return _MIRROR[name]


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_matches_mirror(d, loc, aux, md, mloc, maux):
    assert d.shape == md.shape and loc.shape == mloc.shape, (d.shape, md.shape)
    assert d.dtype == np.float32 and loc.dtype == np.float64
    assert np.array_equal(np.ascontiguousarray(loc).view(np.uint64), np.ascontiguousarray(mloc).view(np.uint64)), "loc bits / keypoint order"
    for col, what in ((0, "scale"), (2, "metric"), (3, "sign of Laplacian")):
        assert np.array_equal(u32(aux[:, col]), u32(maux[:, col])), what
    da = np.abs((aux[:, 1].astype(np.float64) - maux[:, 1].astype(np.float64) + 180.0) % 360.0 - 180.0)
    assert da.size == 0 or da.max() <= 1e-3, da.max()
    assert np.array_equal(u32(d), u32(md)), "descriptor bits (%d rows differ)" % int((u32(d) != u32(md)).any(1).sum())


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_mirror(fm, name):
    img, thr, md, mloc, maux = mirror(name)
    assert len(md) >= 10, "the case must have keypoints to compare"
    d, loc, aux = fm.surf_extract({"detector": "SURF", "MetricThreshold": thr}, img, want_aux=True)
    assert_matches_mirror(d, loc, aux, md, mloc, maux)


def _raw(gpu, img, cap, ldd, fill=np.float32(-7.5), thr=1000.0):
    capi = gpu._capi
    prm = capi.aps_surf_params(thr, 8, 4, 0, 0)
    desc = np.full((max(cap, 1), ldd), fill, np.float32)
    loc = np.zeros((2, max(cap, 1)), np.float64)
    aux = np.zeros((max(cap, 1), 4), np.float32)
    cnt = C.c_int64(-1)
    img = np.ascontiguousarray(img)
    rc = capi.lib.aps_surf_extract(capi.ptr(img), img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, capi.APS_IMG_U8_HWC, C.byref(prm),
                                   capi.ptr(desc), capi.APS_ROWMAJOR, ldd, capi.ptr(loc), max(cap, 1), capi.ptr(aux), cap, C.byref(cnt))
    return rc, cnt.value, desc, loc, aux


def test_capacity_too_small_reports_the_count_and_the_retry_matches(gpu):
    img, thr, md, mloc, maux = mirror("pairA")
    rc, n, *_ = _raw(gpu, img, 8, 64)
    assert rc == gpu._capi.APS_E_CAP and n == len(md)
    rc, n2, desc, loc, aux = _raw(gpu, img, n, 64)
    assert rc == 0 and n2 == n
    assert_matches_mirror(desc[:n], np.ascontiguousarray(loc[:, :n].T), aux[:n], md, mloc, maux)


def test_leading_dimension_128_is_zero_padded_and_64_stays_inside(gpu):
    img, thr, md, _, _ = mirror("97x131")
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
    img = mirror("pairA")[0]
    ref = fm.surf_extract({"detector": "SURF"}, img, want_aux=True)
    again = fm.surf_extract({"detector": "SURF"}, img, want_aux=True)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(ref, again))
    got = [None] * 4

    def work(k):
        got[k] = fm.surf_extract({"detector": "SURF"}, img, want_aux=True)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for g in got:
        assert g is not None and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(ref, g))


def test_getFeaturePoints_contract(fm):
    """Fails with NotImplementedError without the feature."""
    img = mirror("pairA")[0]
    f, pts = fm.getFeaturePoints(dict(detector="SURF"), img)
    assert f.dtype == np.float32 and pts.dtype == np.float64
    assert f.ndim == 2 and f.shape[1] == 64 and pts.shape == (len(f), 2) and len(f) > 100
    assert np.abs(np.linalg.norm(f.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    f0, p0 = fm.getFeaturePoints(dict(detector="SURF"), np.zeros((20, 20), np.uint8))   # below the first octave's support
    assert f0.shape == (0, 64) and p0.shape == (0, 2)
    with pytest.raises(NotImplementedError):
        fm.getFeaturePoints(dict(detector="BRISK"), img)


def test_oversized_image_is_refused(gpu):
    """height * width * 255 >= 2^32 does not fit the 32-bit integral image: APS_E_ARG before any work (no pixel is read)."""
    capi = gpu._capi
    prm = capi.aps_surf_params(1000.0, 8, 4, 0, 0)
    cnt = C.c_int64(0)
    one = np.zeros(16, np.uint8)
    rc = capi.lib.aps_surf_extract(capi.ptr(one), 4200, 4200, 1, capi.APS_IMG_U8_HWC, C.byref(prm), None, capi.APS_ROWMAJOR, 64, None, 0,
                                   None, 0, C.byref(cnt))
    assert rc == capi.APS_E_ARG and b"integral" in capi.lib.aps_last_error()


def test_matlab_layouts_give_the_same_features(gpu):
    """The layouts a MATLAB caller has: planar column-major image (APS_IMG_U8_MATLAB), column-major descriptors (APS_COLMAJOR)
    with a leading dimension above the count; elements between the columns stay the caller's."""
    capi = gpu._capi
    img, thr, md, mloc, _ = mirror("131x97x3")
    n, h, w = len(md), img.shape[0], img.shape[1]
    planar = np.ascontiguousarray(img.transpose(2, 1, 0))   # [c][x][y]: MATLAB's h x w x 3 in memory
    ld = n + 5
    prm = capi.aps_surf_params(thr, 8, 4, 0, 0)
    desc = np.full((64, ld), np.float32(-7.5), np.float32)   # column-major ld x 64
    loc = np.full((2, ld), -7.5, np.float64)
    cnt = C.c_int64(0)
    rc = capi.lib.aps_surf_extract(capi.ptr(planar), h, w, 3, capi.APS_IMG_U8_MATLAB, C.byref(prm), capi.ptr(desc), capi.APS_COLMAJOR, ld,
                                   capi.ptr(loc), ld, None, ld, C.byref(cnt))
    assert rc == 0 and cnt.value == n
    assert np.array_equal(u32(desc[:, :n].T), u32(md)) and (desc[:, n:] == np.float32(-7.5)).all()
    assert np.array_equal(np.ascontiguousarray(loc[:, :n].T).view(np.uint64), np.ascontiguousarray(mloc).view(np.uint64)) and (loc[:, n:] == -7.5).all()
