"""CPU tests of the FAST/ORB boundary: they need the built library but no device, and fail without the feature.
The last test reads the shipped gfx950 code object: orb_keypoint_kernel keeps everything in registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

import orb_mirror as om

NAMES = ("aps_fast_orb_extract", "aps_fast_orb_extract_batch", "aps_orb_pattern")
S12 = (1200000, 1000000)


def test_entry_points_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aps.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and hasattr(capi.lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert [n for n, _ in capi.aps_fast_orb_params._fields_] == ["pyramid", "select", "n_select", "grid_rows", "grid_cols"]
    assert dict(capi.aps_fast_orb_params._fields_)["pyramid"] is capi.aps_fast_pyramid_params
    assert C.sizeof(capi.aps_fast_orb_params) == 11 * C.sizeof(C.c_int)
    assert re.search(r"typedef struct aps_fast_orb_params \{\s*aps_fast_pyramid_params pyramid;[^}]*int select;[^}]*int n_select;[^}]*"
                     r"int grid_rows, grid_cols;[^}]*\}", header)
    # the existing structs keep their fields
    assert C.sizeof(capi.aps_fast_pyramid_params) == 7 * C.sizeof(C.c_int) and C.sizeof(capi.aps_fast_params) == 4 * C.sizeof(C.c_int)
    assert C.sizeof(capi.aps_fast_strongest_params) == 8 * C.sizeof(C.c_int) and C.sizeof(capi.aps_fast_uniform_params) == 10 * C.sizeof(C.c_int)
    assert [n for n, _ in capi.aps_fast_view._fields_] == ["img", "desc", "loc", "aux", "cap", "count"]


def test_pattern_equals_the_mirror(aps):
    tests, table, disc, reach = om.load_pattern(aps._capi)
    mtests, mtable, mdisc, _ = om.pattern()
    assert np.array_equal(tests, mtests) and np.array_equal(table, mtable) and np.array_equal(disc, mdisc)
    assert reach == om.reach(mtable) == 16
    margin = C.c_int(0)
    aps._capi.check(aps._capi.lib.aps_freak_pattern(None, None, None, None, None, C.byref(margin)))
    assert reach <= margin.value == om.MARGIN
    # every pointer may be NULL
    assert aps._capi.lib.aps_orb_pattern(None, None, None, None) == 0
    only = np.full((256, 4), 99, np.int32)
    assert aps._capi.lib.aps_orb_pattern(aps._capi.ptr(only), None, None, None) == 0 and np.array_equal(only, mtests)


def orb_params(capi, select=0, n_select=0, rows=0, cols=0, fast=None, pyramid=(3,) + S12):
    fast = capi.aps_fast_params(51, 100000, 1000000, 0) if fast is None else fast
    return capi.aps_fast_orb_params(capi.aps_fast_pyramid_params(fast, *pyramid), select, n_select, rows, cols)


def test_arguments_are_checked_before_any_device_work(aps):
    """Every refusal below comes back without a device (this test runs where there is none)."""
    capi = aps._capi
    cnt = C.c_int64(0)
    one = np.zeros(16, np.uint8)

    def extract(h, w, prm, ch=1, count=cnt, layout=None, img_layout=None):
        return capi.lib.aps_fast_orb_extract(capi.ptr(one), h, w, ch, capi.APS_IMG_U8_HWC if img_layout is None else img_layout,
                                             None if prm is None else C.byref(prm), None, capi.APS_ROWMAJOR if layout is None else layout, 32,
                                             None, 0, None, 0, None if count is None else C.byref(count))

    for select in (-1, 3, 7):
        assert extract(64, 64, orb_params(capi, select, 10, 4, 4)) == capi.APS_E_ARG, select
        assert b"select" in capi.lib.aps_last_error()
    for select in (1, 2):
        for bad in (0, -1):
            assert extract(64, 64, orb_params(capi, select, bad, 4, 4)) == capi.APS_E_ARG, (select, bad)
    for rows, cols in ((0, 4), (4, 0), (33, 4), (4, 33), (-1, 4)):
        assert extract(64, 64, orb_params(capi, 2, 10, rows, cols)) == capi.APS_E_ARG, (rows, cols)
        assert b"UniformGrid" in capi.lib.aps_last_error()
    assert extract(64, 64, None) == capi.APS_E_ARG and extract(64, 64, orb_params(capi), count=None) == capi.APS_E_ARG
    # what the FAST entries refuse
    for pyr in ((0,) + S12, (17,) + S12, (3, 1000000, 1000000), (3, 2000001, 1000000), (3, 3, 0)):
        for select in (0, 1, 2):
            assert extract(64, 64, orb_params(capi, select, 10, 4, 4, pyramid=pyr)) == capi.APS_E_ARG, (pyr, select)
    for fast_bad, word in ((capi.aps_fast_params(256, 1, 10, 0), b"threshold"), (capi.aps_fast_params(51, 11, 10, 0), b"MinQuality")):
        assert extract(64, 64, orb_params(capi, fast=fast_bad)) == capi.APS_E_ARG and word in capi.lib.aps_last_error()
    assert extract(4200, 4200, orb_params(capi)) == capi.APS_E_ARG and b"integral" in capi.lib.aps_last_error()
    assert extract(0, 64, orb_params(capi)) == capi.APS_E_DIM and extract(64, 64, orb_params(capi), ch=2) == capi.APS_E_DIM
    assert extract(64, 64, orb_params(capi), layout=77) == capi.APS_E_TYPE and extract(64, 64, orb_params(capi), img_layout=77) == capi.APS_E_TYPE
    # the group entry: NULL params / views / image, the number of views
    pyr = orb_params(capi).pyramid
    views = (capi.aps_fast_view * 17)()
    for v in views:
        v.img = capi.ptr(one)

    def batch(views_, n, prm=pyr):
        return capi.lib.aps_fast_orb_extract_batch(views_, n, 64, 64, 1, capi.APS_IMG_U8_HWC, None if prm is None else C.byref(prm),
                                                   capi.APS_ROWMAJOR, 32, 0)

    assert batch(views, 1, None) == capi.APS_E_ARG and batch(None, 1) == capi.APS_E_ARG
    assert batch(views, 0) == capi.APS_E_ARG and batch(views, 17) == capi.APS_E_ARG
    views[1].img = None
    assert batch(views, 2) == capi.APS_E_ARG
    assert batch(views, 1, capi.aps_fast_pyramid_params(pyr.fast, 0, *S12)) == capi.APS_E_ARG


def test_descriptor_method_is_read_and_checked_by_the_wrappers(aps):
    capi = aps._capi
    fm = import_module(aps.__name__ + ".featureMatching")
    pl = import_module(aps.__name__ + ".pipeline")
    img = np.zeros((64, 64), np.uint8)
    assert "DescriptorMethod" not in pl.DEFAULT_INPUT and "DescriptorMethod" not in pl.default_input()
    for bad in ("BRIEF", "orb", "", None, 32):
        inp = {"detector": "FAST", "DescriptorMethod": bad}
        for call in (lambda: fm.fast_extract(inp, img), lambda: fm.fast_extract_batch(inp, [img]), lambda: fm.getFeaturePoints(inp, img),
                     lambda: fm.extract_features(inp, img)):
            with pytest.raises(ValueError, match="DescriptorMethod"):
                call()
    # fast_extract_batch keeps refusing the selection keys, whatever the descriptor
    for key in ("NumStrongest", "NumUniform"):
        with pytest.raises(ValueError, match="fast_extract_batch"):
            fm.fast_extract_batch({"detector": "FAST", "DescriptorMethod": "ORB", key: 10}, [img])
    with pytest.raises(ValueError):   # one selection rule per call, before any library call
        fm.fast_extract({"detector": "FAST", "DescriptorMethod": "ORB", "NumStrongest": 5, "NumUniform": 5}, img)
    # the selection values are the library's to refuse: the key reaches aps_fast_orb_extract
    for extra in ({"NumStrongest": 0}, {"NumUniform": 0}, {"NumUniform": 5, "UniformGrid": (0, 4)}, {"NumLevels": 3, "NumStrongest": -2}):
        with pytest.raises(aps.ApsError) as e:
            fm.fast_extract({"detector": "FAST", "DescriptorMethod": "ORB", **extra}, img)
        assert e.value.code == capi.APS_E_ARG, extra
    if capi.lib.aps_device_count() > 0:
        f, pts = fm.fast_extract({"detector": "FAST", "DescriptorMethod": "ORB"}, img)
        assert f.Features.shape == (0, 32) and f.NumBits == 256
    else:
        with pytest.raises(aps.ApsError) as e:
            fm.fast_extract({"detector": "FAST", "DescriptorMethod": "ORB"}, img)
        assert e.value.code == capi.APS_E_DEVICE
    # the unchanged refusals
    with pytest.raises(NotImplementedError):
        fm.getFeaturePoints({"detector": "ORB"}, img)
    par = import_module(aps.__name__ + ".parallel")
    with pytest.raises(NotImplementedError):
        par.stitch_distributed({"detector": "FAST", "DescriptorMethod": "ORB"}, {}, 0, None)
    assert pl._group_route({"detector": "FAST", "DescriptorMethod": "ORB", "NumStrongest": 10}) is None


LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "orb_keypoint_kernel"


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="needs the ROCm llvm tools")
def test_orb_kernel_uses_no_scratch(aps, tmp_path):
    """The shipped gfx950 code object: orb_keypoint_kernel has no private segment and no VGPR or SGPR spills, and its LDS is the
    four waves' patches and box-sum planes."""
    so = os.path.join(tmp_path, "libaps_hip.so")
    shutil.copy(aps._capi.LIB_PATH, so)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True)
    found = []
    for co in sorted(os.path.join(tmp_path, f) for f in os.listdir(tmp_path) if f.endswith("gfx950")):
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s+- \.agpr_count:", "\n" + notes)[1:]:
            sym = re.search(r"\.symbol:\s+(\S+)", entry)
            if sym and KERNEL in sym.group(1):
                found.append({k: int(re.search(r"\.%s:\s+(\S+)" % k, entry).group(1))
                              for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "sgpr_count",
                                        "group_segment_fixed_size")})
    assert len(found) == 1
    md = found[0]
    print(KERNEL, md)
    assert (md["private_segment_fixed_size"], md["vgpr_spill_count"], md["sgpr_spill_count"]) == (0, 0, 0), md
    assert md["group_segment_fixed_size"] <= 4 * (31 * 32 + 2 * (27 * 27 + 1)) + 64, md
