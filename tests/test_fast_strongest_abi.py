"""CPU tests of FAST/FREAK strongest-N's boundary: they need the built library but no device, and fail without the feature.
The last test reads the shipped gfx950 code object: the new kernels keep everything in registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

import fast_pyramid_cases as pc
import fast_pyramid_mirror as pmir
import fast_strongest_mirror as smir

NAMES = ("aps_fast_extract_strongest", "aps_fast_strongest_quota", "aps_fast_harris")
S12 = (1200000, 1000000)


def test_entry_points_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aps.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and hasattr(capi.lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert [n for n, _ in capi.aps_fast_strongest_params._fields_] == ["pyramid", "n_strongest"]
    assert dict(capi.aps_fast_strongest_params._fields_)["pyramid"] is capi.aps_fast_pyramid_params
    assert C.sizeof(capi.aps_fast_strongest_params) == 8 * C.sizeof(C.c_int)
    assert re.search(r"typedef struct aps_fast_strongest_params \{\s*aps_fast_pyramid_params pyramid;[^}]*int n_strongest;[^}]*\}", header)
    # the parents' structs keep their fields
    assert C.sizeof(capi.aps_fast_pyramid_params) == 7 * C.sizeof(C.c_int) and C.sizeof(capi.aps_fast_params) == 4 * C.sizeof(C.c_int)


def lib_quota(capi, h, w, n_levels, num, den, N):
    q, used = (C.c_int * 16)(*([-1] * 16)), C.c_int(-1)
    rc = capi.lib.aps_fast_strongest_quota(h, w, n_levels, num, den, N, q, C.byref(used))
    return rc, list(q)[:max(used.value, 0)], list(q)


def test_quota_equals_the_mirror(aps):
    capi = aps._capi
    assert lib_quota(capi, 120, 160, 4, *S12, 1)[1] == [1, 0, 0, 0]
    assert lib_quota(capi, 120, 160, 4, *S12, 3)[1] == [1, 1, 1, 0]
    assert lib_quota(capi, 120, 160, 4, *S12, 100)[1] == [33, 27, 22, 18]
    todo = [(pc.image(n).shape[0], pc.image(n).shape[1], nl, sf) for n, (_, nl, sf, _, _) in pc.CASES.items()]
    todo += [(47, 49, 8, 1.2), (180, 240, 3, 1.2), (2160, 3840, 16, 1.2), (2160, 3840, 8, 1.2), (95, 95, 2, 2.0)]
    for (h, w, nl, sf) in todo:
        num, den = pmir.scale_rational(sf)
        shapes = pmir.plan(h, w, nl, num, den, 23)
        for N in (1, 2, 7, 200, 5000, 2 ** 31 - 1):
            rc, got, raw = lib_quota(capi, h, w, nl, num, den, N)
            assert rc == 0 and got == smir.quotas(shapes, N) and sum(got) == N, (h, w, nl, sf, N)
            assert all(v == -1 for v in raw[len(shapes):])   # nothing written beyond the plan
    used = C.c_int(0)
    assert capi.lib.aps_fast_strongest_quota(120, 160, 4, *S12, 100, None, C.byref(used)) == 0 and used.value == 4


REFUSED_PYRAMIDS = [(0, 1200000, 1000000), (17, 1200000, 1000000), (-1, 1200000, 1000000), (4, 1000000, 1000000),
                    (4, 999999, 1000000), (4, 2000001, 1000000), (4, 3, 0), (4, -3, -2), (4, 0, -1)]


def test_arguments_are_checked_before_any_device_work(aps):
    """Every refusal below comes back without a device (this test runs where there is none): n_strongest below 1, the refused
    pyramids, the refused aps_fast_params values and the oversized image of the parent entries, and NULL params / count."""
    capi = aps._capi
    cnt = C.c_int64(0)
    one = np.zeros(16, np.uint8)
    fast_ok = capi.aps_fast_params(51, 100000, 1000000, 0)
    pyr_ok = capi.aps_fast_pyramid_params(fast_ok, 4, *S12)

    def extract(h, w, prm, ch=1, count=cnt):
        return capi.lib.aps_fast_extract_strongest(capi.ptr(one), h, w, ch, capi.APS_IMG_U8_HWC, None if prm is None else C.byref(prm), None,
                                                   capi.APS_ROWMAJOR, 64, None, 0, None, 0, None if count is None else C.byref(count))

    def harris(h, w, prm, count=cnt):
        return capi.lib.aps_fast_harris(capi.ptr(one), h, w, 1, capi.APS_IMG_U8_HWC, None if prm is None else C.byref(prm), None, 0,
                                        None if count is None else C.byref(count))

    for bad in (0, -1):
        assert extract(64, 64, capi.aps_fast_strongest_params(pyr_ok, bad)) == capi.APS_E_ARG
        assert b"n_strongest" in capi.lib.aps_last_error()
        assert lib_quota(capi, 64, 64, 4, *S12, bad)[0] == capi.APS_E_ARG
    for (nl, num, den) in REFUSED_PYRAMIDS:
        pyr = capi.aps_fast_pyramid_params(fast_ok, nl, num, den)
        assert extract(64, 64, capi.aps_fast_strongest_params(pyr, 10)) == capi.APS_E_ARG, (nl, num, den)
        assert harris(64, 64, pyr) == capi.APS_E_ARG, (nl, num, den)
        assert lib_quota(capi, 64, 64, nl, num, den, 10)[0] == capi.APS_E_ARG, (nl, num, den)
    assert b"ScaleFactor" in capi.lib.aps_last_error()
    good = capi.aps_fast_strongest_params(pyr_ok, 10)
    assert extract(4200, 4200, good) == capi.APS_E_ARG and b"integral" in capi.lib.aps_last_error()   # 4200 * 4200 * 255 >= 2^32
    assert harris(4200, 4200, pyr_ok) == capi.APS_E_ARG
    for fast_bad, word in ((capi.aps_fast_params(256, 1, 10, 0), b"threshold"), (capi.aps_fast_params(-1, 1, 10, 0), b"threshold"),
                           (capi.aps_fast_params(51, 11, 10, 0), b"MinQuality"), (capi.aps_fast_params(51, 1, 0, 0), b"MinQuality"),
                           (capi.aps_fast_params(51, -1, 10, 0), b"MinQuality"), (capi.aps_fast_params(51, 1, (1 << 24) + 1, 0), b"MinQuality")):
        pyr = capi.aps_fast_pyramid_params(fast_bad, 4, *S12)
        assert extract(64, 64, capi.aps_fast_strongest_params(pyr, 10)) == capi.APS_E_ARG
        assert word in capi.lib.aps_last_error()
        assert harris(64, 64, pyr) == capi.APS_E_ARG
    assert extract(0, 64, good) == capi.APS_E_DIM and extract(64, 64, good, ch=2) == capi.APS_E_DIM
    assert extract(64, 64, None) == capi.APS_E_ARG and extract(64, 64, good, count=None) == capi.APS_E_ARG
    assert harris(64, 64, None) == capi.APS_E_ARG and harris(64, 64, pyr_ok, count=None) == capi.APS_E_ARG
    assert capi.lib.aps_fast_strongest_quota(64, 64, 4, *S12, 10, None, None) == capi.APS_E_ARG
    assert lib_quota(capi, 0, 64, 4, *S12, 10)[0] == capi.APS_E_DIM


def test_fast_extract_reads_the_key(aps):
    """NumStrongest reaches the library for any NumLevels: a value below 1 is the library's APS_E_ARG, and a good one gets as far
    as the device (this test runs where there is none; on a machine with a device the call succeeds)."""
    capi = aps._capi
    fm = import_module(aps.__name__ + ".featureMatching")
    img = np.zeros((64, 64), np.uint8)
    for extra in ({}, {"NumLevels": 3}):
        for bad in (0, -5):
            with pytest.raises(aps.ApsError) as e:
                fm.fast_extract({"detector": "FAST", "NumStrongest": bad, **extra}, img)
            assert e.value.code == capi.APS_E_ARG
    if capi.lib.aps_device_count() > 0:
        f, pts = fm.fast_extract({"detector": "FAST", "NumStrongest": 10}, img)
        assert f.Features.shape == (0, 64)
    else:
        with pytest.raises(aps.ApsError) as e:
            fm.fast_extract({"detector": "FAST", "NumStrongest": 10}, img)
        assert e.value.code == capi.APS_E_DEVICE
    assert "NumStrongest" not in import_module(aps.__name__ + ".pipeline").default_input()
    par = import_module(aps.__name__ + ".parallel")
    with pytest.raises(NotImplementedError):
        par.stitch_distributed({"detector": "FAST", "NumStrongest": 100}, {}, 0, None)


LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("fast_harris_kernel", "strongest_counts_kernel", "strongest_flag_kernel", "strongest_word_kernel", "strongest_compact_kernel",
           "strongest_aux_kernel")
PARENT_KERNELS = ("fast_resample_kernel", "fast_detect_kernel", "fast_gate_kernel", "fast_emit_kernel", "freak_keypoint_kernel")


def test_new_kernel_names_do_not_shadow_the_parents():
    assert not [(k, p) for k in KERNELS for p in PARENT_KERNELS if p in k]


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="needs the ROCm llvm tools")
def test_strongest_kernels_use_no_scratch(aps, tmp_path):
    """The shipped gfx950 code object: the Harris kernel and the selection's kernels keep everything in registers (no private
    segment, no VGPR or SGPR spills)."""
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
                               for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "sgpr_count",
                                         "group_segment_fixed_size")}
    assert sorted(found) == sorted(KERNELS)
    for name, md in found.items():
        print(name, md)
        assert (md["private_segment_fixed_size"], md["vgpr_spill_count"], md["sgpr_spill_count"]) == (0, 0, 0), (name, md)
