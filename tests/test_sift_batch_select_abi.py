"""CPU tests of the grouped SIFT selections (aps_sift_extract_batch_strongest, aps_sift_extract_batch_uniform): they need the built
library but no device, and fail without the feature."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

NAMES = ("aps_sift_extract_batch_strongest", "aps_sift_extract_batch_uniform")
SIFT = (1.6, 4, 0.00133, 6.0, 0)


def fmod(aps):
    return import_module(aps.__name__ + ".featureMatching")


def test_entry_points_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aps.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and hasattr(capi.lib, name)
        assert re.search(r"\bint %s\(aps_sift_view\* views, int n_views," % name, header)
    # the argument lists are aps_sift_extract_batch's, with the selection's parameter struct
    base = capi._SIGNATURES["aps_sift_extract_batch"]
    for name, struct in zip(NAMES, (capi.aps_sift_strongest_params, capi.aps_sift_uniform_params)):
        sig = capi._SIGNATURES[name]
        assert len(sig) == len(base) == 10 and sig[:6] == base[:6] and sig[7:] == base[7:] and sig[6] is C.POINTER(struct)


def _strongest(capi, n):
    return capi.aps_sift_strongest_params(capi.aps_sift_params(*SIFT), n)


def _uniform(capi, n, rows, cols):
    return capi.aps_sift_uniform_params(_strongest(capi, n), rows, cols)


def _call(capi, entry, prm, views="one", n_views=1, img="zeros"):
    """The entry on one 64 x 64 gray view with count-only outputs; views=None / img=None pass NULL."""
    pixels = np.zeros(64 * 64, np.uint8)
    if views is not None:
        views = (capi.aps_sift_view * 1)()
        views[0].img = None if img is None else capi.ptr(pixels)
        views[0].cap, views[0].count = 0, -1
    return entry(views, n_views, 64, 64, 1, capi.APS_IMG_U8_HWC, None if prm is None else C.byref(prm), capi.APS_ROWMAJOR, 128, 1)


def _refused(capi, rc):
    return rc == capi.APS_E_ARG and len(capi.lib.aps_last_error() or b"") > 0


def test_arguments_are_checked_before_any_device_work(aps):
    """Every refusal is APS_E_ARG with a message where there is no device (this test runs there), ahead of APS_E_DEVICE."""
    capi = aps._capi
    s, u = capi.lib.aps_sift_extract_batch_strongest, capi.lib.aps_sift_extract_batch_uniform
    assert _refused(capi, _call(capi, s, _strongest(capi, 0))) and b"NumStrongest" in capi.lib.aps_last_error()
    assert _refused(capi, _call(capi, u, _uniform(capi, 0, 8, 8))) and b"NumUniform" in capi.lib.aps_last_error()
    for grid in ((0, 8), (8, 0), (33, 8), (8, 33)):
        assert _refused(capi, _call(capi, u, _uniform(capi, 10, *grid))) and b"UniformGrid" in capi.lib.aps_last_error()
    for entry, prm in ((s, _strongest(capi, 10)), (u, _uniform(capi, 10, 8, 8))):
        for n_views in (0, capi.APS_SIFT_MAX_VIEWS + 1):
            assert _refused(capi, _call(capi, entry, prm, n_views=n_views)) and b"n_views" in capi.lib.aps_last_error()
        assert _refused(capi, _call(capi, entry, prm, views=None))
        assert _refused(capi, _call(capi, entry, None))
        assert _refused(capi, _call(capi, entry, prm, img=None))
        if capi.lib.aps_device_count() == 0:   # a good call gets as far as the device
            assert _call(capi, entry, prm) == capi.APS_E_DEVICE


def test_both_keys_are_refused_in_python(aps):
    img = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="NumUniform"):
        fmod(aps).sift_extract_batch({"detector": "SIFT", "NumUniform": 10, "NumStrongest": 10}, [img, img])


@pytest.mark.parametrize("keys", [{"NumStrongest": 10}, {"NumUniform": 10}, {"NumUniform": 10, "UniformGrid": (3, 5)}])
def test_either_key_reaches_the_library(aps, keys):
    """No ValueError: features with a device, APS_E_DEVICE without one; a bad value is the library's APS_E_ARG."""
    capi = aps._capi
    fm = fmod(aps)
    img = np.zeros((64, 64, 3), np.uint8)
    try:
        out = fm.sift_extract_batch({"detector": "SIFT", **keys}, [img, img])
    except aps.ApsError as e:
        assert capi.lib.aps_device_count() == 0 and e.code == capi.APS_E_DEVICE
    else:
        assert [len(o[1]) for o in out] == [0, 0]
    bad = {k: (0 if k != "UniformGrid" else v) for k, v in keys.items()}
    with pytest.raises(aps.ApsError) as e:
        fm.sift_extract_batch({"detector": "SIFT", **bad}, [img, img])
    assert e.value.code == capi.APS_E_ARG
