"""CPU tests of the KAZE boundary: they need the built library but no device, and all but the last fail without the feature."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kaze_entry_point_is_declared_bound_and_exported(aps):
    capi = aps._capi
    header = open(os.path.join(ROOT, "include", "aps.h")).read()
    assert re.search(r"\bint\s+aps_kaze_extract\s*\(", header)
    assert "aps_kaze_extract" in capi.EXPORTED_SYMBOLS
    assert hasattr(C.CDLL(capi.LIB_PATH), "aps_kaze_extract")
    fields = [n for n, _ in capi.aps_kaze_params._fields_]
    assert fields == ["threshold", "num_octaves", "num_scale_levels", "diffusion", "max_features"]
    body = re.search(r"typedef struct aps_kaze_params \{(.*?)\} aps_kaze_params;", header, re.S).group(1)
    assert re.findall(r"(?:double|int)\s+(\w+);", body) == fields
    for name in ("APS_KAZE_DIFFUSION_REGION", "APS_KAZE_DIFFUSION_SHARPEDGE", "APS_KAZE_DIFFUSION_EDGE"):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) == getattr(capi, name)


def test_arguments_are_checked_before_any_device_work(aps):
    """Every refusal carries APS_E_ARG (or the layout's / shape's own code) and its own message, with or without a device: no
    pixel is read, and no refusal is APS_E_DEVICE."""
    capi = aps._capi
    cnt = C.c_int64(0)
    one = np.zeros(16, np.uint8)

    def call(prm, h=64, w=64, c=1, img_layout=capi.APS_IMG_U8_HWC, desc_layout=capi.APS_ROWMAJOR, img=one, count=cnt, cap=0):
        return capi.lib.aps_kaze_extract(capi.ptr(img), h, w, c, img_layout, C.byref(prm) if prm is not None else None, None, desc_layout, 64,
                                         None, 0, None, cap, C.byref(count) if count is not None else None)

    ok = (1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_REGION, 0)
    P = capi.aps_kaze_params
    for prm, word in ((P(1e-4, 0, 4, 0, 0), b"NumOctaves"), (P(1e-4, 5, 4, 0, 0), b"NumOctaves"), (P(1e-4, 3, 2, 0, 0), b"NumScaleLevels"),
                      (P(1e-4, 3, 11, 0, 0), b"NumScaleLevels"), (P(-1e-4, 3, 4, 0, 0), b"Threshold"),
                      (P(1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_SHARPEDGE, 0), b"not built"), (P(1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_EDGE, 0), b"not built"),
                      (P(1e-4, 3, 4, 7, 0), b"Diffusion")):
        assert call(prm) == capi.APS_E_ARG and word in capi.lib.aps_last_error(), word
    assert call(None) == capi.APS_E_ARG and call(P(*ok), img=None) == capi.APS_E_ARG and call(P(*ok), count=None) == capi.APS_E_ARG
    assert call(P(*ok), cap=-1) == capi.APS_E_ARG
    assert call(P(*ok), h=50000, w=50000) == capi.APS_E_ARG and b"2^31" in capi.lib.aps_last_error()
    assert call(P(*ok), h=0) == capi.APS_E_DIM and call(P(*ok), c=2) == capi.APS_E_DIM
    assert call(P(*ok), img_layout=99) == capi.APS_E_TYPE and call(P(*ok), desc_layout=99) == capi.APS_E_TYPE


def test_wrappers_refuse_the_diffusivities_that_are_not_built(aps):
    fm = import_module(aps.__name__ + ".featureMatching")
    img = np.zeros((64, 64), np.uint8)
    for value in ("sharpedge", "edge", "nonsense"):
        for call in (fm.kaze_extract, fm.extract_features):
            with pytest.raises(ValueError):
                call({"detector": "KAZE", "Diffusion": value}, img)


def test_extract_features_reaches_the_library(aps):
    """'KAZE' reaches aps_kaze_extract through extract_features and kaze_extract: features with a device, APS_E_DEVICE without
    one - never NotImplementedError."""
    fm = import_module(aps.__name__ + ".featureMatching")
    img = np.zeros((64, 64), np.uint8)
    for call in (fm.extract_features, fm.kaze_extract):
        try:
            f, pts = call({"detector": "KAZE"}, img)
        except aps.ApsError as e:
            assert aps.lib.aps_device_count() == 0 and e.code == aps._capi.APS_E_DEVICE
        else:
            assert f.shape == (0, 64) and pts.shape == (0, 2)
    pl = import_module(aps.__name__ + ".pipeline")
    assert not any(k in pl.default_input() for k in ("Threshold", "NumOctaves", "NumScaleLevels", "Diffusion"))
    assert pl._group_route(pl.default_input(detector="KAZE")) is None


def test_getFeaturePoints_still_refuses_kaze(aps):
    fm = import_module(aps.__name__ + ".featureMatching")
    with pytest.raises(NotImplementedError):
        fm.getFeaturePoints({"detector": "KAZE"}, np.zeros((64, 64), np.uint8))
