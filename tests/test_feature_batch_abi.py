"""CPU tests of the group entries of SURF and FAST/FREAK (aps_surf_extract_batch, aps_surf_extract_batch_strongest,
aps_surf_extract_batch_uniform, aps_fast_extract_batch): they need the built library but no device, and fail without the feature."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

SURF_NAMES = ("aps_surf_extract_batch", "aps_surf_extract_batch_strongest", "aps_surf_extract_batch_uniform")
NAMES = SURF_NAMES + ("aps_fast_extract_batch",)
HEADER = open(os.path.join(os.path.dirname(__file__), "..", "include", "aps.h")).read()


def fmod(aps):
    return import_module(aps.__name__ + ".featureMatching")


def test_entry_points_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and hasattr(capi.lib, name)
        view = "aps_surf_view" if "surf" in name else "aps_fast_view"
        assert re.search(r"\bint %s\(%s\* views, int n_views," % (name, view), HEADER)
    # the argument lists are aps_sift_extract_batch's, with the detector's view and parameter structs
    base = capi._SIGNATURES["aps_sift_extract_batch"]
    structs = (capi.aps_surf_params, capi.aps_surf_strongest_params, capi.aps_surf_uniform_params, capi.aps_fast_pyramid_params)
    for name, struct in zip(NAMES, structs):
        sig = capi._SIGNATURES[name]
        view = capi.aps_surf_view if "surf" in name else capi.aps_fast_view
        assert len(sig) == len(base) == 10 and sig[1:6] == base[1:6] and sig[7:] == base[7:]
        assert sig[0] is C.POINTER(view) and sig[6] is C.POINTER(struct)


@pytest.mark.parametrize("det, desc_type", [("surf", "float"), ("fast", "uint8_t")])
def test_view_structs_match_the_header(aps, det, desc_type):
    capi = aps._capi
    m = re.search(r"typedef struct aps_%s_view \{(.*?)\} aps_%s_view;" % (det, det), HEADER, re.S)
    assert m, "aps_%s_view is not declared" % det
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["const uint8_t* img", "%s* desc" % desc_type, "double* loc", "float* aux", "int64_t cap", "int64_t count"]
    struct = getattr(capi, "aps_%s_view" % det)
    assert [n for n, _ in struct._fields_] == ["img", "desc", "loc", "aux", "cap", "count"]
    assert [t for _, t in struct._fields_] == [C.c_void_p] * 4 + [C.c_int64] * 2
    assert re.search(r"#define APS_%s_MAX_VIEWS 16\b" % det.upper(), HEADER) and getattr(capi, "APS_%s_MAX_VIEWS" % det.upper()) == 16


def _surf(capi, thr=1000.0, octaves=8, levels=4):
    return capi.aps_surf_params(thr, octaves, levels, 0, 0)


def _strongest(capi, n, **kw):
    return capi.aps_surf_strongest_params(_surf(capi, **kw), n)


def _uniform(capi, n, rows, cols, **kw):
    return capi.aps_surf_uniform_params(_strongest(capi, n, **kw), rows, cols)


def _fast(capi, n_levels=1, num=1200000, den=1000000, t=51, qn=100000, qd=1000000):
    return capi.aps_fast_pyramid_params(capi.aps_fast_params(t, qn, qd, 0), n_levels, num, den)


def _call(capi, entry, prm, views="one", n_views=1, img="zeros", h=64, w=64):
    """The entry on one h x w gray view with count-only outputs; views=None / img=None pass NULL.  (No pixel is read before the
    checks are through: the buffer holds 64 x 64 whatever h and w say.)"""
    pixels = np.zeros(64 * 64, np.uint8)
    if views is not None:
        views = ((capi.aps_surf_view if "surf" in entry.__name__ else capi.aps_fast_view) * 1)()
        views[0].img = None if img is None else capi.ptr(pixels)
        views[0].cap, views[0].count = 0, -1
    return entry(views, n_views, h, w, 1, capi.APS_IMG_U8_HWC, None if prm is None else C.byref(prm), capi.APS_ROWMAJOR, 128, 1)


def _refused(capi, rc):
    return rc == capi.APS_E_ARG and len(capi.lib.aps_last_error() or b"") > 0


def test_arguments_are_checked_before_any_device_work(aps):
    """Every refusal is APS_E_ARG with a message where there is no device (this test runs there), ahead of APS_E_DEVICE."""
    capi = aps._capi
    p, s, u = (getattr(capi.lib, n) for n in SURF_NAMES)
    f = capi.lib.aps_fast_extract_batch
    good = ((p, _surf(capi)), (s, _strongest(capi, 10)), (u, _uniform(capi, 10, 8, 8)), (f, _fast(capi)), (f, _fast(capi, 3)))
    for entry, prm in good:
        for n_views in (0, 17):
            assert _refused(capi, _call(capi, entry, prm, n_views=n_views)) and b"n_views" in capi.lib.aps_last_error()
        assert _refused(capi, _call(capi, entry, prm, views=None))
        assert _refused(capi, _call(capi, entry, None))
        assert _refused(capi, _call(capi, entry, prm, img=None))
        assert _refused(capi, _call(capi, entry, prm, h=4200, w=4200)) and b"integral" in capi.lib.aps_last_error()   # 4200^2 * 255 >= 2^32
        if capi.lib.aps_device_count() == 0:   # a good call gets as far as the device
            assert _call(capi, entry, prm) == capi.APS_E_DEVICE
    # the selection's own values
    assert _refused(capi, _call(capi, s, _strongest(capi, 0))) and b"NumStrongest" in capi.lib.aps_last_error()
    assert _refused(capi, _call(capi, u, _uniform(capi, 0, 8, 8))) and b"NumUniform" in capi.lib.aps_last_error()
    for grid in ((0, 8), (8, 0), (33, 8), (8, 33)):
        assert _refused(capi, _call(capi, u, _uniform(capi, 10, *grid))) and b"UniformGrid" in capi.lib.aps_last_error()
    # every parameter range the single-view entries check
    for kw, word in ((dict(levels=2), b"NumScaleLevels"), (dict(levels=9), b"NumScaleLevels"), (dict(octaves=0), b"NumOctaves"),
                     (dict(octaves=13), b"NumOctaves"), (dict(thr=-1.0), b"MetricThreshold")):
        for entry, prm in ((p, _surf(capi, **kw)), (s, _strongest(capi, 10, **kw)), (u, _uniform(capi, 10, 8, 8, **kw))):
            assert _refused(capi, _call(capi, entry, prm)) and word in capi.lib.aps_last_error()
    for kw, word in ((dict(t=256), b"threshold"), (dict(t=-1), b"threshold"), (dict(qn=11, qd=10), b"MinQuality"), (dict(qd=0), b"MinQuality"),
                     (dict(n_levels=0), b"NumLevels"), (dict(n_levels=17), b"NumLevels"), (dict(num=1000000), b"ScaleFactor"),
                     (dict(num=2000001), b"ScaleFactor"), (dict(den=0), b"ScaleFactor")):
        assert _refused(capi, _call(capi, f, _fast(capi, **kw))) and word in capi.lib.aps_last_error()
    # a capacity outside 0 .. 2^31 - 1
    for entry, prm in good:
        views = ((capi.aps_surf_view if "surf" in entry.__name__ else capi.aps_fast_view) * 1)()
        pixels = np.zeros(64 * 64, np.uint8)
        views[0].img, views[0].cap = capi.ptr(pixels), -1
        assert _refused(capi, entry(views, 1, 64, 64, 1, capi.APS_IMG_U8_HWC, C.byref(prm), capi.APS_ROWMAJOR, 128, 1))


def test_fast_groups_refuse_the_selection_keys_in_python(aps):
    img = np.zeros((64, 64, 3), np.uint8)
    for key in ("NumStrongest", "NumUniform"):
        with pytest.raises(ValueError, match="fast_extract per view"):
            fmod(aps).fast_extract_batch({"detector": "FAST", key: 10}, [img, img])
    with pytest.raises(ValueError, match="NumUniform"):
        fmod(aps).surf_extract_batch({"detector": "SURF", "NumUniform": 10, "NumStrongest": 10}, [img, img])
    with pytest.raises(ValueError, match="one shape"):
        fmod(aps).surf_extract_batch({"detector": "SURF"}, [img, img[:32]])


@pytest.mark.parametrize("det, keys", [("SURF", {}), ("SURF", {"NumStrongest": 10}), ("SURF", {"NumUniform": 10, "UniformGrid": (3, 5)}),
                                       ("FAST", {}), ("FAST", {"NumLevels": 3})])
def test_the_wrappers_reach_the_library(aps, det, keys):
    """Features with a device, APS_E_DEVICE without one; a bad value is the library's APS_E_ARG."""
    capi = aps._capi
    fm = fmod(aps)
    batch = fm.surf_extract_batch if det == "SURF" else fm.fast_extract_batch
    img = np.zeros((64, 64, 3), np.uint8)
    try:
        out = batch({"detector": det, **keys}, [img, img])
    except aps.ApsError as e:
        assert capi.lib.aps_device_count() == 0 and e.code == capi.APS_E_DEVICE
    else:
        assert [len(o[1]) for o in out] == [0, 0] and all(len(o) == 2 for o in out)
    bad = {"NumOctaves": 0} if det == "SURF" else {"NumLevels": 17}
    with pytest.raises(aps.ApsError) as e:
        batch({"detector": det, **keys, **bad}, [img, img])
    assert e.value.code == capi.APS_E_ARG
