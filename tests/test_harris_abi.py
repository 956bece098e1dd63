"""CPU tests of the Harris corner boundary (aps_corner_extract, aps_corner_extract_batch, aps_harris_planes, input.CornerMethod):
they need the built library but no device, and fail without the feature."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

NAMES = ("aps_corner_extract", "aps_corner_extract_batch", "aps_harris_planes")
S12 = (1200000, 1000000)


def test_entry_points_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aps.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and hasattr(capi.lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert [n for n, _ in capi.aps_corner_params._fields_] == ["chain", "corner", "descriptor"]
    assert dict(capi.aps_corner_params._fields_)["chain"] is capi.aps_fast_orb_params
    assert C.sizeof(capi.aps_corner_params) == 13 * C.sizeof(C.c_int)
    assert capi.aps_corner_params.corner.offset == 11 * C.sizeof(C.c_int) and capi.aps_corner_params.descriptor.offset == 12 * C.sizeof(C.c_int)
    assert re.search(r"typedef struct aps_corner_params \{\s*aps_fast_orb_params chain;[^}]*int corner;[^}]*int descriptor;[^}]*\}", header)
    assert re.search(r"enum \{ APS_CORNER_FAST = 0, APS_CORNER_HARRIS = 1 \};", header)
    assert re.search(r"enum \{ APS_DESC_FREAK = 0, APS_DESC_ORB = 1 \};", header)
    assert (capi.APS_CORNER_FAST, capi.APS_CORNER_HARRIS, capi.APS_DESC_FREAK, capi.APS_DESC_ORB) == (0, 1, 0, 1)
    # the existing structs keep their fields
    assert C.sizeof(capi.aps_fast_orb_params) == 11 * C.sizeof(C.c_int) and C.sizeof(capi.aps_fast_pyramid_params) == 7 * C.sizeof(C.c_int)
    assert [n for n, _ in capi.aps_fast_view._fields_] == ["img", "desc", "loc", "aux", "cap", "count"]


def corner_params(capi, corner=1, descriptor=0, select=0, n_select=0, rows=0, cols=0, fast=None, pyramid=(3,) + S12):
    fast = capi.aps_fast_params(0, 10000, 1000000, 0) if fast is None else fast
    chain = capi.aps_fast_orb_params(capi.aps_fast_pyramid_params(fast, *pyramid), select, n_select, rows, cols)
    return capi.aps_corner_params(chain, corner, descriptor)


def test_arguments_are_checked_before_any_device_work(aps):
    """Every refusal below comes back without a device (this test runs where there is none)."""
    capi = aps._capi
    cnt = C.c_int64(0)
    one = np.zeros(16, np.uint8)

    def extract(h, w, prm, ch=1, count=cnt, layout=None, img_layout=None):
        return capi.lib.aps_corner_extract(capi.ptr(one), h, w, ch, capi.APS_IMG_U8_HWC if img_layout is None else img_layout,
                                           None if prm is None else C.byref(prm), None, capi.APS_ROWMAJOR if layout is None else layout, 64,
                                           None, 0, None, 0, None if count is None else C.byref(count))

    for corner in (0, 1):
        for bad in (-1, 2, 9):
            assert extract(64, 64, corner_params(capi, corner, bad)) == capi.APS_E_ARG and b"descriptor" in capi.lib.aps_last_error()
    for bad in (-1, 2, 9):
        assert extract(64, 64, corner_params(capi, bad, 0)) == capi.APS_E_ARG and b"corner" in capi.lib.aps_last_error()
    assert extract(64, 64, None) == capi.APS_E_ARG and extract(64, 64, corner_params(capi), count=None) == capi.APS_E_ARG
    for corner in (0, 1):
        for desc in (0, 1):
            for select in (-1, 3):
                assert extract(64, 64, corner_params(capi, corner, desc, select, 10, 4, 4)) == capi.APS_E_ARG
                assert b"select" in capi.lib.aps_last_error()
            for select in (1, 2):
                assert extract(64, 64, corner_params(capi, corner, desc, select, 0, 4, 4)) == capi.APS_E_ARG
            for rows, cols in ((0, 4), (4, 33)):
                assert extract(64, 64, corner_params(capi, corner, desc, 2, 10, rows, cols)) == capi.APS_E_ARG
                assert b"UniformGrid" in capi.lib.aps_last_error()
            # what the FAST entries refuse, the threshold that Harris does not read included
            for pyr in ((0,) + S12, (17,) + S12, (3, 1000000, 1000000), (3, 2000001, 1000000), (3, 3, 0)):
                for select in (0, 1, 2):
                    assert extract(64, 64, corner_params(capi, corner, desc, select, 10, 4, 4, pyramid=pyr)) == capi.APS_E_ARG, (pyr, select)
            for fast_bad, word in ((capi.aps_fast_params(256, 1, 10, 0), b"threshold"), (capi.aps_fast_params(0, 11, 10, 0), b"MinQuality"),
                                   (capi.aps_fast_params(0, 1, (1 << 24) + 1, 0), b"MinQuality")):
                assert extract(64, 64, corner_params(capi, corner, desc, fast=fast_bad)) == capi.APS_E_ARG and word in capi.lib.aps_last_error()
            assert extract(4200, 4200, corner_params(capi, corner, desc)) == capi.APS_E_ARG and b"integral" in capi.lib.aps_last_error()
            assert extract(0, 64, corner_params(capi, corner, desc)) == capi.APS_E_DIM
            assert extract(64, 64, corner_params(capi, corner, desc), ch=2) == capi.APS_E_DIM
            assert extract(64, 64, corner_params(capi, corner, desc), layout=77) == capi.APS_E_TYPE
            assert extract(64, 64, corner_params(capi, corner, desc), img_layout=77) == capi.APS_E_TYPE
    # the group entry: no selection, NULL params / views / image, the number of views
    views = (capi.aps_fast_view * 17)()
    for v in views:
        v.img = capi.ptr(one)

    def batch(views_, n, prm):
        return capi.lib.aps_corner_extract_batch(views_, n, 64, 64, 1, capi.APS_IMG_U8_HWC, None if prm is None else C.byref(prm),
                                                 capi.APS_ROWMAJOR, 64, 0)

    ok = corner_params(capi)
    for select in (1, 2, -1):
        assert batch(views, 1, corner_params(capi, 1, 0, select, 10, 4, 4)) == capi.APS_E_ARG and b"select" in capi.lib.aps_last_error()
        assert batch(views, 1, corner_params(capi, 0, 1, select, 10, 4, 4)) == capi.APS_E_ARG
    assert batch(views, 1, corner_params(capi, 2, 0)) == capi.APS_E_ARG and batch(views, 1, corner_params(capi, 1, 2)) == capi.APS_E_ARG
    assert batch(views, 1, None) == capi.APS_E_ARG and batch(None, 1, ok) == capi.APS_E_ARG
    assert batch(views, 0, ok) == capi.APS_E_ARG and batch(views, 17, ok) == capi.APS_E_ARG
    views[1].img = None
    assert batch(views, 2, ok) == capi.APS_E_ARG
    assert batch(views, 1, corner_params(capi, pyramid=(0,) + S12)) == capi.APS_E_ARG

    # the test hook: its checks, and the size alone needs no device
    def planes(h, w, pyr, out=None, cap=0, count=cnt):
        return capi.lib.aps_harris_planes(capi.ptr(one), h, w, 1, capi.APS_IMG_U8_HWC, None if pyr is None else C.byref(pyr), out, cap,
                                          None if count is None else C.byref(count))

    pyr = ok.chain.pyramid
    assert planes(64, 64, None) == capi.APS_E_ARG and planes(64, 64, pyr, count=None) == capi.APS_E_ARG
    assert planes(64, 64, capi.aps_fast_pyramid_params(pyr.fast, 0, *S12)) == capi.APS_E_ARG and planes(0, 64, pyr) == capi.APS_E_DIM
    assert planes(96, 128, pyr) == 0 and cnt.value == 96 * 128 + 80 * 107 + 67 * 89
    buf = np.zeros(8, np.int64)
    assert planes(96, 128, pyr, capi.ptr(buf), 8) == capi.APS_E_CAP and cnt.value == 96 * 128 + 80 * 107 + 67 * 89


def test_corner_method_is_read_and_checked_by_the_wrappers(aps):
    capi = aps._capi
    fm = import_module(aps.__name__ + ".featureMatching")
    pl = import_module(aps.__name__ + ".pipeline")
    img = np.zeros((64, 64), np.uint8)
    assert "CornerMethod" not in pl.DEFAULT_INPUT and "CornerMethod" not in pl.default_input()
    assert pl.default_input(detector="FAST", CornerMethod="Harris")["CornerMethod"] == "Harris"
    for bad in ("bogus", "HARRIS", "harris", "", None, 1):
        for extra in ({}, {"DescriptorMethod": "ORB"}):
            inp = {"detector": "FAST", "CornerMethod": bad, **extra}
            for call in (lambda: fm.fast_extract(inp, img), lambda: fm.fast_extract_batch(inp, [img]), lambda: fm.getFeaturePoints(inp, img),
                         lambda: fm.extract_features(inp, img)):
                with pytest.raises(ValueError, match="CornerMethod"):
                    call()
    # the key is read only with detector = 'FAST'
    with pytest.raises(NotImplementedError):
        fm.getFeaturePoints({"detector": "HARRIS", "CornerMethod": "bogus"}, img)
    # fast_extract_batch keeps refusing the selection keys
    for key in ("NumStrongest", "NumUniform"):
        with pytest.raises(ValueError, match="fast_extract_batch"):
            fm.fast_extract_batch({"detector": "FAST", "CornerMethod": "Harris", key: 10}, [img])
    with pytest.raises(ValueError):   # one selection rule per call, before any library call
        fm.fast_extract({"detector": "FAST", "CornerMethod": "Harris", "NumStrongest": 5, "NumUniform": 5}, img)
    # the selection values are the library's to refuse: the keys reach aps_corner_extract
    for extra in ({"NumStrongest": 0}, {"NumUniform": 0}, {"NumUniform": 5, "UniformGrid": (0, 4)}, {"NumLevels": 3, "NumStrongest": -2},
                  {"NumLevels": 0}, {"MinQuality": 1.5}):
        for desc in ("FREAK", "ORB"):
            with pytest.raises(aps.ApsError) as e:
                fm.fast_extract({"detector": "FAST", "CornerMethod": "Harris", "DescriptorMethod": desc, **extra}, img)
            assert e.value.code == capi.APS_E_ARG, extra
    # MinContrast is ignored: a value the FAST entries refuse does not reach the library
    prm = fm._corner_params({"detector": "FAST", "CornerMethod": "Harris", "MinContrast": 7.0}, 2, None, "ORB")
    assert prm.chain.pyramid.fast.threshold == 0 and (prm.corner, prm.descriptor) == (capi.APS_CORNER_HARRIS, capi.APS_DESC_ORB)
    assert (prm.chain.pyramid.fast.quality_num, prm.chain.pyramid.fast.quality_den) == (10000, 1000000)   # detectHarrisFeatures' 0.01
    assert fm._fast_params({"detector": "FAST"}).quality_num == 100000                                     # FAST keeps its 0.1
    if capi.lib.aps_device_count() > 0:
        f, pts = fm.fast_extract({"detector": "FAST", "CornerMethod": "Harris"}, img)
        assert f.Features.shape == (0, 64)
    else:
        with pytest.raises(aps.ApsError) as e:
            fm.fast_extract({"detector": "FAST", "CornerMethod": "Harris"}, img)
        assert e.value.code == capi.APS_E_DEVICE


def test_the_unchanged_refusals(aps):
    fm = import_module(aps.__name__ + ".featureMatching")
    par = import_module(aps.__name__ + ".parallel")
    img = np.zeros((64, 64), np.uint8)
    with pytest.raises(NotImplementedError):
        fm.getFeaturePoints({"detector": "HARRIS"}, img)
    with pytest.raises(NotImplementedError):
        par.stitch_distributed({"detector": "FAST", "CornerMethod": "Harris"}, {}, 0, None)
