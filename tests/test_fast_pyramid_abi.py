"""CPU tests of the FAST/FREAK pyramid's boundary: they need the built library but no device, and fail without the feature.
The last test reads the shipped gfx950 code object: the FAST kernels keep everything in registers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fast_pyramid_cases as pc
import fast_pyramid_mirror as pmir

NAMES = ("aps_fast_extract_pyramid", "aps_fast_pyramid_plan", "aps_fast_pyramid_planes")


def test_pyramid_entry_points_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and hasattr(capi.lib, name)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aps.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header)
    assert [n for n, _ in capi.aps_fast_pyramid_params._fields_] == ["fast", "n_levels", "scale_num", "scale_den"]
    assert dict(capi.aps_fast_pyramid_params._fields_)["fast"] is capi.aps_fast_params
    assert C.sizeof(capi.aps_fast_pyramid_params) == 7 * C.sizeof(C.c_int)
    assert re.search(r"typedef struct aps_fast_pyramid_params \{\s*aps_fast_params fast;[^}]*int n_levels;[^}]*int scale_num;[^}]*int scale_den;[^}]*\}", header)


def lib_plan(capi, h, w, n_levels, num, den):
    hs, ws, used = (C.c_int * 16)(*([-1] * 16)), (C.c_int * 16)(*([-1] * 16)), C.c_int(-1)
    rc = capi.lib.aps_fast_pyramid_plan(h, w, n_levels, num, den, hs, ws, C.byref(used))
    return rc, [(hs[l], ws[l]) for l in range(max(used.value, 0))], (list(hs), list(ws))


def test_plan_equals_the_mirror(aps):
    import fast_cases as fc

    capi = aps._capi
    margin = fc.tables().margin
    assert margin == 23
    todo = [(pc.image(n).shape[0], pc.image(n).shape[1], nl, sf) for n, (_, nl, sf, _, _) in pc.CASES.items()]
    todo += [(47, 49, 8, 1.2), (180, 240, 3, 1.2), (2160, 3840, 16, 1.2), (30, 20, 4, 1.2), (95, 95, 2, 2.0), (3000, 5000, 16, 1.000001)]
    for (h, w, nl, sf) in todo:
        num, den = pmir.scale_rational(sf)
        rc, got, (hs, ws) = lib_plan(capi, h, w, nl, num, den)
        want = pmir.plan(h, w, nl, num, den, margin)
        assert rc == 0 and got == want, (h, w, nl, sf)
        assert all(v == -1 for v in hs[len(want):] + ws[len(want):])   # nothing written beyond the plan
    assert lib_plan(capi, 120, 160, 4, 1200000, 1000000)[1] == pc.PLANS["120x160"]
    assert lib_plan(capi, 64, 64, 3, 1200000, 1000000)[1] == pc.PLANS["64x64"]
    assert lib_plan(capi, 47, 49, 8, 1200000, 1000000)[1] == [(47, 49)]
    used = C.c_int(0)
    assert capi.lib.aps_fast_pyramid_plan(120, 160, 4, 1200000, 1000000, None, None, C.byref(used)) == 0 and used.value == 4


REFUSED_PYRAMIDS = [(0, 1200000, 1000000), (17, 1200000, 1000000), (-1, 1200000, 1000000), (4, 1000000, 1000000),
                    (4, 999999, 1000000), (4, 2000001, 1000000), (4, 3, 0), (4, -3, -2), (4, 0, -1)]


def test_arguments_are_checked_before_any_device_work(aps):
    """Every refusal below comes back without a device (this test runs where there is none): the pyramid's own parameters, the
    oversized image and the refused aps_fast_params values of the parent entry, for all three entries."""
    capi = aps._capi
    cnt, nbytes = C.c_int64(0), C.c_int64(0)
    one = np.zeros(16, np.uint8)
    fast_ok = capi.aps_fast_params(51, 100000, 1000000, 0)

    def extract(h, w, prm):
        return capi.lib.aps_fast_extract_pyramid(capi.ptr(one), h, w, 1, capi.APS_IMG_U8_HWC, C.byref(prm), None, capi.APS_ROWMAJOR, 64,
                                                 None, 0, None, 0, C.byref(cnt))

    def planes(h, w, prm):
        return capi.lib.aps_fast_pyramid_planes(capi.ptr(one), h, w, 1, capi.APS_IMG_U8_HWC, C.byref(prm), None, 0, C.byref(nbytes))

    for (nl, num, den) in REFUSED_PYRAMIDS:
        prm = capi.aps_fast_pyramid_params(fast_ok, nl, num, den)
        assert extract(64, 64, prm) == capi.APS_E_ARG, (nl, num, den)
        assert planes(64, 64, prm) == capi.APS_E_ARG, (nl, num, den)
        assert lib_plan(capi, 64, 64, nl, num, den)[0] == capi.APS_E_ARG, (nl, num, den)
    assert b"ScaleFactor" in capi.lib.aps_last_error()
    good = capi.aps_fast_pyramid_params(fast_ok, 4, 1200000, 1000000)
    assert extract(4200, 4200, good) == capi.APS_E_ARG and b"integral" in capi.lib.aps_last_error()   # 4200 * 4200 * 255 >= 2^32
    assert planes(4200, 4200, good) == capi.APS_E_ARG
    for fast_bad, word in ((capi.aps_fast_params(256, 1, 10, 0), b"threshold"), (capi.aps_fast_params(-1, 1, 10, 0), b"threshold"),
                           (capi.aps_fast_params(51, 11, 10, 0), b"MinQuality"), (capi.aps_fast_params(51, 1, 0, 0), b"MinQuality"),
                           (capi.aps_fast_params(51, -1, 10, 0), b"MinQuality"), (capi.aps_fast_params(51, 1, (1 << 24) + 1, 0), b"MinQuality")):
        assert extract(64, 64, capi.aps_fast_pyramid_params(fast_bad, 4, 1200000, 1000000)) == capi.APS_E_ARG
        assert word in capi.lib.aps_last_error()
    assert extract(0, 64, good) == capi.APS_E_DIM
    assert capi.lib.aps_fast_extract_pyramid(capi.ptr(one), 64, 64, 2, capi.APS_IMG_U8_HWC, C.byref(good), None, capi.APS_ROWMAJOR, 64, None, 0,
                                             None, 0, C.byref(cnt)) == capi.APS_E_DIM
    assert capi.lib.aps_fast_extract_pyramid(capi.ptr(one), 64, 64, 1, capi.APS_IMG_U8_HWC, None, None, capi.APS_ROWMAJOR, 64, None, 0,
                                             None, 0, C.byref(cnt)) == capi.APS_E_ARG
    # the size of the planes needs no device either: out = NULL reports it
    assert planes(120, 160, good) == 0 and nbytes.value == sum(h * w for h, w in pc.PLANS["120x160"])


def test_fast_extract_reads_the_two_keys(aps):
    """NumLevels > 1 reaches the library's checks (a refused ScaleFactor is an ApsError, not a silent single level);
    the distributed path keeps refusing the binary family."""
    from importlib import import_module

    fm = import_module(aps.__name__ + ".featureMatching")
    img = np.zeros((64, 64), np.uint8)
    for bad in ({"NumLevels": 4, "ScaleFactor": 1.0}, {"NumLevels": 4, "ScaleFactor": 2.5}, {"NumLevels": 17}, {"NumLevels": 0}):
        with pytest.raises(aps.ApsError) as e:
            fm.fast_extract({"detector": "FAST", **bad}, img)
        assert e.value.code == aps._capi.APS_E_ARG
    assert "NumLevels" not in import_module(aps.__name__ + ".pipeline").default_input()
    par = import_module(aps.__name__ + ".parallel")
    with pytest.raises(NotImplementedError):
        par.stitch_distributed({"detector": "FAST", "NumLevels": 4}, {}, 0, None)


LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("fast_resample_kernel", "fast_detect_kernel", "fast_gate_kernel", "fast_emit_kernel", "freak_keypoint_kernel")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="needs the ROCm llvm tools")
def test_fast_kernels_use_no_scratch(aps, tmp_path):
    """The shipped gfx950 code object: the resampling kernel and the four kernels that take the level table keep everything
    in registers (no private segment, no VGPR or SGPR spills)."""
    so = os.path.join(tmp_path, "libaps_hip.so")
    shutil.copy(aps._capi.LIB_PATH, so)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True)
    found = {}
    for co in sorted(os.path.join(tmp_path, f) for f in os.listdir(tmp_path) if f.endswith("gfx950")):
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s+- \.agpr_count:", "\n" + notes)[1:]:
            sym = re.search(r"\.symbol:\s+(\S+)", entry)
            name = next((k for k in KERNELS if sym and k in sym.group(1)), None)
            if name:
                found[name] = {k: int(re.search(r"\.%s:\s+(\S+)" % k, entry).group(1))
                               for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    assert sorted(found) == sorted(KERNELS)
    for name, md in found.items():
        assert md == {"private_segment_fixed_size": 0, "vgpr_spill_count": 0, "sgpr_spill_count": 0}, (name, md)
