"""CPU tests of the max-weight multiband boundary: they need the built library but no device, and fail without the feature."""
import ctypes as C
import re
from importlib import import_module

import numpy as np
import pytest


def test_symbol_and_enum_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    assert "aps_maxweight_weights" in capi.EXPORTED_SYMBOLS
    assert hasattr(lib, "aps_maxweight_weights") and hasattr(capi.lib, "aps_maxweight_weights")
    assert capi.APS_BLEND_MULTIBAND_MAXWEIGHT == 3
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aps.h")).read()
    assert re.search(r"APS_BLEND_MULTIBAND_MAXWEIGHT\s*=\s*3\b", header)
    assert re.search(r"int\s+aps_maxweight_weights\s*\(\s*const float\*\s*Wt,\s*int k,\s*int h,\s*int w,\s*float\*\s*out\)", header)


def test_maxweight_weights_refuses_bad_arguments_before_any_device_work(aps):
    capi = aps._capi
    W = np.ones((2, 3, 4), np.float32)
    out = np.zeros_like(W)
    f = capi.lib.aps_maxweight_weights
    for args in ((None, 2, 3, 4, capi.ptr(out)), (capi.ptr(W), 2, 3, 4, None), (capi.ptr(W), 0, 3, 4, capi.ptr(out)),
                 (capi.ptr(W), 2, 0, 4, capi.ptr(out)), (capi.ptr(W), 2, 3, 0, capi.ptr(out)),
                 (capi.ptr(W), -1, 3, 4, capi.ptr(out))):
        assert f(*args) == capi.APS_E_ARG, args
    assert not out.any()


def test_render_and_planar_entries_refuse_modes_above_three_as_before(aps):
    """blending = 4 is APS_E_ARG at every entry that takes a blending (and 3 is not refused as an unknown mode: without a
    device the call gets as far as the device and reports that)."""
    capi = aps._capi
    rp = import_module(aps.__name__ + ".renderPanorama")
    img = np.zeros((8, 8, 3), np.uint8)
    arr, keep = rp.make_image_structs([img], [{"K": np.eye(3), "R": np.eye(3)}])
    cv = capi.aps_canvas(capi.APS_PROJ_SPHERICAL, 8, 8, 10.0, 0.0, 0.0)
    pano, cov = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8)

    def render(blending):
        ro = capi.aps_render_opts(8, 8, 2.0, blending, 3, 1.0, 0, 0)
        return [capi.lib.aps_render(arr, 1, C.byref(cv), C.byref(ro), capi.APS_IMG_U8_HWC, capi.ptr(pano), capi.ptr(cov)),
                capi.lib.aps_render_tiles(arr, 1, C.byref(cv), C.byref(ro), capi.APS_IMG_U8_HWC, 0, 1, capi.ptr(pano), capi.ptr(cov)),
                capi.lib.aps_render_tile_range(arr, 1, C.byref(cv), C.byref(ro), capi.APS_IMG_U8_HWC, 0, 1, capi.ptr(pano), capi.ptr(cov))]

    assert render(4) == [capi.APS_E_ARG] * 3 and b"unknown blending" in capi.lib.aps_last_error()
    ok = (capi.APS_OK,) if capi.lib.aps_device_count() > 0 else (capi.APS_E_DEVICE,)
    assert all(st in ok for st in render(capi.APS_BLEND_MULTIBAND_MAXWEIGHT))
    # the byte formulas: what multiband returns, and a refusal above 3
    view = {"ImageSize": (40, 50), "XWorldLimits": (0.5, 50.5), "YWorldLimits": (0.5, 40.5), "PixelExtentInWorldX": 1.0,
            "PixelExtentInWorldY": 1.0}
    ih, iw, ic = (np.array([v], np.int32) for v in (30, 40, 3))
    H = np.ascontiguousarray(np.eye(3).reshape(1, 9))
    dense = [int(capi.lib.aps_planar_composite_bytes(1, capi.ptr(ih), capi.ptr(iw), capi.ptr(ic), 40, 50, m, 3)) for m in (2, 3, 4)]
    compact = [int(capi.lib.aps_planar_composite_compact_bytes(1, capi.ptr(ih), capi.ptr(iw), capi.ptr(ic), capi.ptr(H), 40, 50, 0.5,
                                                               0.5, 1.0, 1.0, m, 3)) for m in (2, 3, 4)]
    assert dense[0] > 0 and dense[1] == dense[0] and dense[2] == capi.APS_E_ARG
    assert compact[0] > 0 and compact[1] == compact[0] and compact[2] == capi.APS_E_ARG
    del keep, view


class _NoCalls:
    """Stands in for the loaded library: any attribute access is a library call the test forbids."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the multibandWeights check")


@pytest.mark.parametrize("bad", ["maxWeights", "", "linear", 1, None])
def test_unknown_multibandWeights_is_a_ValueError_before_any_library_call(aps, monkeypatch, bad):
    rp = import_module(aps.__name__ + ".renderPanorama")
    bl = import_module(aps.__name__ + ".blending")
    monkeypatch.setattr(rp, "lib", _NoCalls())
    monkeypatch.setattr(bl, "lib", _NoCalls())
    img = np.zeros((20, 30, 3), np.uint8)
    cams = [{"K": np.array([[50.0, 0, 15.5], [0, 50.0, 10.5], [0, 0, 1]]), "R": np.eye(3)}]
    opts = {"blending": "multiband", "multibandWeights": bad, "tile": (16, 16), "gainCompensation": True}
    with pytest.raises(ValueError, match="multibandWeights"):
        rp.renderPanorama({}, [img], [(20, 30, 3)], cams, "spherical", 0, opts)
    pcams = [{"H2refined": np.eye(3), "noRotation": 1}]
    for extra in ({}, {"planarCompositor": "host"}, {"planarCompositor": "compact"}):
        with pytest.raises(ValueError, match="multibandWeights"):
            rp.pureNonRotationalPanoramas([img], pcams, 1, dict(opts, **extra))
    view = {"ImageSize": (20, 30), "XWorldLimits": (0.5, 30.5), "YWorldLimits": (0.5, 20.5), "PixelExtentInWorldX": 1.0,
            "PixelExtentInWorldY": 1.0}
    for fn in (rp.planar_composite, rp.planar_composite_compact):
        with pytest.raises(ValueError, match="multibandWeights"):
            fn([img], [np.eye(3)], view, {"blending": "multiband", "multibandWeights": bad})
    with pytest.raises(ValueError, match="Weights"):
        bl.multiBandBlending([np.zeros((4, 4, 3), np.float32)], [np.ones((4, 4), np.float32)], 2, True, 1.0, Weights=bad)


def test_the_key_is_read_only_with_multiband_blending(aps):
    rp = import_module(aps.__name__ + ".renderPanorama")
    assert rp.multiband_weights({"blending": "linear", "multibandWeights": "nonsense"}) == "tent"
    assert rp.blend_mode({"blending": "none", "multibandWeights": "maxweight"}) == aps._capi.APS_BLEND_NONE
    assert rp.blend_mode({"blending": "multiband"}) == aps._capi.APS_BLEND_MULTIBAND
    assert rp.blend_mode({"blending": "multiband", "multibandWeights": "tent"}) == aps._capi.APS_BLEND_MULTIBAND
    assert rp.blend_mode({"blending": "Multiband", "multibandWeights": "MaxWeight"}) == aps._capi.APS_BLEND_MULTIBAND_MAXWEIGHT
    pl = import_module(aps.__name__ + ".pipeline")
    assert "multibandWeights" not in pl.DEFAULT_INPUT
