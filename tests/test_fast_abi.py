"""CPU tests of the FAST/FREAK boundary and of the binary matching branch's host half: they need the built library but no
device, and fail without the feature."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest


def fmod(aps):
    return import_module(aps.__name__ + ".featureMatching")


def test_fast_entry_points_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("aps_fast_extract", "aps_freak_pattern"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert [n for n, _ in capi.aps_fast_params._fields_] == ["threshold", "quality_num", "quality_den", "max_features"]


def test_getFeaturePoints_dispatches_fast_to_the_library(aps):
    """'FAST' reaches aps_fast_extract: features with a device, APS_E_DEVICE without one - never NotImplementedError."""
    fm = fmod(aps)
    img = np.zeros((64, 64), np.uint8)
    try:
        f, pts = fm.getFeaturePoints({"detector": "FAST"}, img)
    except aps.ApsError as e:
        assert aps.lib.aps_device_count() == 0 and e.code == aps._capi.APS_E_DEVICE
    else:
        assert isinstance(f, fm.binaryFeatures) and f.Features.shape == (0, 64) and pts.shape == (0, 2)
    for det in ("vl_SIFT", "HARRIS", "BRISK", "ORB", "KAZE"):
        with pytest.raises(NotImplementedError):
            fm.getFeaturePoints({"detector": det}, img)


def test_arguments_are_checked_before_any_device_work(aps):
    capi = aps._capi
    cnt = C.c_int64(0)
    one = np.zeros(16, np.uint8)

    def call(h, w, prm):
        return capi.lib.aps_fast_extract(capi.ptr(one), h, w, 1, capi.APS_IMG_U8_HWC, C.byref(prm), None, capi.APS_ROWMAJOR, 64, None, 0,
                                         None, 0, C.byref(cnt))

    assert call(4200, 4200, capi.aps_fast_params(51, 100000, 1000000, 0)) == capi.APS_E_ARG   # 4200 * 4200 * 255 >= 2^32
    assert b"integral" in capi.lib.aps_last_error()
    assert call(64, 64, capi.aps_fast_params(256, 1, 10, 0)) == capi.APS_E_ARG
    assert call(64, 64, capi.aps_fast_params(51, 11, 10, 0)) == capi.APS_E_ARG and b"MinQuality" in capi.lib.aps_last_error()
    assert call(64, 64, capi.aps_fast_params(51, 1, 0, 0)) == capi.APS_E_ARG


def test_binaryFeatures_object(aps):
    fm = fmod(aps)
    f = fm.binaryFeatures(np.zeros((5, 64), np.uint8))
    assert len(f) == 5 and f.NumFeatures == 5 and f.NumBits == 512 and f.Features.dtype == np.uint8
    with pytest.raises(TypeError):
        fm.binaryFeatures(np.zeros((5, 64), np.float32))


def test_empty_binary_sets_give_empty_results_without_a_device(aps):
    fm = fmod(aps)
    e, a = fm.binaryFeatures(np.zeros((0, 64), np.uint8)), fm.binaryFeatures(np.ones((3, 64), np.uint8))
    for pair in ((e, a), (a, e), (e, e)):
        for method in ("Exhaustive", "Approximate"):
            m, d = fm.matchFeaturesScratch(*pair, Method=method, MatchThreshold=10)
            assert m.shape == (0, 2) and m.dtype == np.uint32 and d.shape == (0,) and d.dtype == np.float32
    m, d = fm.matchFeaturesScratch(np.zeros((0, 16), bool), np.ones((2, 16), bool))
    assert m.shape == (0, 2) and d.shape == (0,)
    with pytest.raises(TypeError):
        fm.matchFeaturesScratch(a, np.ones((3, 64), np.float32))
    g = fm.featureMatchingGlobal({"Ratiothreshold": 0.6, "k": 4}, [e, e], 2)
    assert g == [[None, None], [None, None]]
    with pytest.raises(TypeError):   # mixed float and binary sets: refused, not dropped
        fm.featureMatchingGlobal({"Ratiothreshold": 0.6, "k": 4}, [a, np.ones((3, 128), np.float32)], 2)


def test_packBits_against_a_hand_packed_row(aps):
    fm = fmod(aps)
    bits = np.array([[1, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0], [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1]], bool)
    packed, n = fm.packBits(bits)   # MSB first: 1000 0011 = 131, 010x xxxx = 64; 0000 0001 = 1, 111 -> 1110 0000 = 224
    assert n == 11 and packed.dtype == np.uint8 and packed.tolist() == [[131, 64], [1, 224]]


def test_filter_matches_binary_uses_the_linear_ratio(aps):
    """best = 30, second = 60 (percent), MaxRatio 0.6: linear 30 <= 36 keeps, squared 30 <= 0.36 * 60 = 21.6 drops.
    Row 2: 40 vs 60: 40 > 36, dropped by both.  Row 3 passes the ratio but not the threshold."""
    fm = fmod(aps)
    idx2 = np.array([2, 1, 3], np.uint32)
    best, second = np.array([30, 40, 50], np.float32), np.array([60, 60, 100], np.float32)
    m, d = fm.filter_matches(idx2, best, second, 3, 0.6, 45.0, True, binary=True)
    assert m.tolist() == [[1, 2]] and d.tolist() == [30.0]
    m2, _ = fm.filter_matches(idx2, best, second, 3, 0.6, 45.0, True)
    assert m2.shape == (0, 2)
    # greedy uniqueness on the columns, ascending distance
    m3, d3 = fm.filter_matches(np.array([1, 1], np.uint32), np.array([12, 6], np.float32), np.array([50, 50], np.float32), 2, 0.6, 45.0, True, binary=True)
    assert m3.tolist() == [[2, 1]] and d3.tolist() == [6.0]


def test_distributed_path_refuses_binary_sets(aps):
    par = import_module(aps.__name__ + ".parallel")
    with pytest.raises(NotImplementedError):
        par.stitch_distributed({"detector": "FAST"}, {}, 0, None)
