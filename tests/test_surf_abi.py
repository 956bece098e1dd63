"""CPU tests of the SURF boundary: they need the built library but no device, and fail without the feature."""
import ctypes as C
from importlib import import_module

import numpy as np


def test_surf_entry_point_is_declared_bound_and_exported(aps):
    capi = aps._capi
    assert "aps_surf_extract" in capi.EXPORTED_SYMBOLS
    assert hasattr(C.CDLL(capi.LIB_PATH), "aps_surf_extract")
    fields = [n for n, _ in capi.aps_surf_params._fields_]
    assert fields == ["metric_threshold", "n_octaves", "n_scale_levels", "upright", "max_features"]


def test_arguments_are_checked_before_any_device_work(aps):
    """The size limit of the 32-bit integral image (height * width * 255 < 2^32) and the parameter ranges are refused with
    their own codes and messages, with or without a device: no pixel is read."""
    capi = aps._capi
    cnt = C.c_int64(0)
    one = np.zeros(16, np.uint8)

    def call(h, w, prm):
        return capi.lib.aps_surf_extract(capi.ptr(one), h, w, 1, capi.APS_IMG_U8_HWC, C.byref(prm), None, capi.APS_ROWMAJOR, 64, None, 0,
                                         None, 0, C.byref(cnt))

    assert call(4200, 4200, capi.aps_surf_params(1000.0, 8, 4, 0, 0)) == capi.APS_E_ARG
    assert b"integral" in capi.lib.aps_last_error()
    assert call(64, 64, capi.aps_surf_params(1000.0, 8, 2, 0, 0)) == capi.APS_E_ARG and b"NumScaleLevels" in capi.lib.aps_last_error()
    assert call(64, 64, capi.aps_surf_params(1000.0, 0, 4, 0, 0)) == capi.APS_E_ARG and b"NumOctaves" in capi.lib.aps_last_error()
    assert call(64, 64, capi.aps_surf_params(-1.0, 8, 4, 0, 0)) == capi.APS_E_ARG


def test_getFeaturePoints_dispatches_surf_to_the_library(aps):
    """'SURF' reaches aps_surf_extract: features with a device, APS_E_DEVICE without one - never NotImplementedError."""
    fm = import_module(aps.__name__ + ".featureMatching")
    img = np.zeros((64, 64), np.uint8)
    try:
        f, pts = fm.getFeaturePoints({"detector": "SURF"}, img)
    except aps.ApsError as e:
        assert aps.lib.aps_device_count() == 0 and e.code == aps._capi.APS_E_DEVICE
    else:
        assert f.shape == (0, 64) and pts.shape == (0, 2)
