"""CPU tests of SIFT / SURF strongest-N's boundary: they need the built library but no device, and fail without the feature.
The last test reads the shipped gfx950 code object: the new kernels keep everything in registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

NAMES = ("aps_sift_extract_strongest", "aps_surf_extract_strongest")


def test_entry_points_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aps.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and hasattr(capi.lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    for det, parent in (("sift", capi.aps_sift_params), ("surf", capi.aps_surf_params)):
        st = getattr(capi, "aps_%s_strongest_params" % det)
        assert [n for n, _ in st._fields_] == [det, "n_strongest"] and dict(st._fields_)[det] is parent
        assert dict(st._fields_)["n_strongest"] is C.c_int
        assert re.search(r"typedef struct aps_%s_strongest_params \{\s*aps_%s_params %s;[^}]*int n_strongest;[^}]*\}" % (det, det, det), header)
        # the argument list is the parent entry's, with the new struct
        sig, psig = capi._SIGNATURES["aps_%s_extract_strongest" % det], capi._SIGNATURES["aps_%s_extract" % det]
        assert len(sig) == len(psig) == 14 and sig[:5] == psig[:5] and sig[6:] == psig[6:] and sig[5] is not psig[5]
    # the parents' structs keep their fields
    assert [n for n, _ in capi.aps_sift_params._fields_] == ["sigma", "n_layers", "contrast_threshold", "edge_threshold", "max_features"]
    assert [n for n, _ in capi.aps_surf_params._fields_] == ["metric_threshold", "n_octaves", "n_scale_levels", "upright", "max_features"]


def _entries(capi):
    sift_ok, surf_ok = capi.aps_sift_params(1.6, 4, 0.00133, 6.0, 0), capi.aps_surf_params(1000.0, 8, 4, 0, 0)
    return (("sift", capi.lib.aps_sift_extract_strongest, lambda n, p=sift_ok: capi.aps_sift_strongest_params(p, n), 128),
            ("surf", capi.lib.aps_surf_extract_strongest, lambda n, p=surf_ok: capi.aps_surf_strongest_params(p, n), 64))


def test_arguments_are_checked_before_any_device_work(aps):
    """n_strongest below 1 comes back as APS_E_ARG without a device (this test runs where there is none), ahead of APS_E_DEVICE; so
    do the parents' refusals and NULL params / count."""
    capi = aps._capi
    one = np.zeros(64 * 64, np.uint8)
    for det, entry, make, ldd in _entries(capi):
        cnt = C.c_int64(0)

        def extract(h, w, prm, ch=1, count=cnt):
            return entry(capi.ptr(one), h, w, ch, capi.APS_IMG_U8_HWC, None if prm is None else C.byref(prm), None, capi.APS_ROWMAJOR, ldd, None,
                         0, None, 0, None if count is None else C.byref(count))

        for bad in (0, -1):
            assert extract(64, 64, make(bad)) == capi.APS_E_ARG, (det, bad)
            assert b"n_strongest" in capi.lib.aps_last_error()
        assert extract(64, 64, None) == capi.APS_E_ARG and extract(64, 64, make(10), count=None) == capi.APS_E_ARG
        assert extract(0, 64, make(10)) == capi.APS_E_DIM and extract(64, 64, make(10), ch=2) == capi.APS_E_DIM
        if capi.lib.aps_device_count() == 0:
            assert extract(64, 64, make(10)) == capi.APS_E_DEVICE, det
    sift_bad = capi.aps_sift_strongest_params(capi.aps_sift_params(1.6, 9, 0.00133, 6.0, 0), 10)
    surf_bad = capi.aps_surf_strongest_params(capi.aps_surf_params(1000.0, 8, 2, 0, 0), 10)
    for (det, entry, make, ldd), prm, word in zip(_entries(capi), (sift_bad, surf_bad), (b"NumLayersInOctave", b"NumScaleLevels")):
        cnt = C.c_int64(0)
        rc = entry(capi.ptr(one), 64, 64, 1, capi.APS_IMG_U8_HWC, C.byref(prm), None, capi.APS_ROWMAJOR, ldd, None, 0, None, 0, C.byref(cnt))
        assert rc == capi.APS_E_ARG and word in capi.lib.aps_last_error()
    cnt = C.c_int64(0)
    big = capi.aps_surf_strongest_params(capi.aps_surf_params(1000.0, 8, 4, 0, 0), 10)
    rc = capi.lib.aps_surf_extract_strongest(capi.ptr(one), 4200, 4200, 1, capi.APS_IMG_U8_HWC, C.byref(big), None, capi.APS_ROWMAJOR, 64, None, 0,
                                             None, 0, C.byref(cnt))
    assert rc == capi.APS_E_ARG and b"integral" in capi.lib.aps_last_error()   # 4200 * 4200 * 255 >= 2^32


@pytest.mark.parametrize("det", ["SIFT", "SURF"])
def test_the_wrappers_pass_the_key(aps, det):
    """NumStrongest reaches the library: a value below 1 is the library's APS_E_ARG (without the feature the key is ignored and the call
    gets as far as the device: APS_E_DEVICE here), through every host entry that extracts features."""
    capi = aps._capi
    fm = import_module(aps.__name__ + ".featureMatching")
    pl = import_module(aps.__name__ + ".pipeline")
    img = np.zeros((64, 64, 3), np.uint8)
    extract = {"SIFT": fm.sift_extract, "SURF": fm.surf_extract}[det]
    calls = (lambda inp: extract(inp, img), lambda inp: fm.getFeaturePoints(inp, img), lambda inp: fm.extract_features(inp, img),
             lambda inp: pl.extract_features(inp, [img]))
    for bad in (0, -5):
        for call in calls:
            with pytest.raises(aps.ApsError) as e:
                call({"detector": det, "NumStrongest": bad})
            assert e.value.code == capi.APS_E_ARG
    if capi.lib.aps_device_count() > 0:
        f, pts = extract({"detector": det, "NumStrongest": 10}, img)
        assert f.shape[0] == 0
    else:
        with pytest.raises(aps.ApsError) as e:
            extract({"detector": det, "NumStrongest": 10}, img)
        assert e.value.code == capi.APS_E_DEVICE
    assert "NumStrongest" not in pl.default_input() and "NumStrongest" not in pl.default_input(detector=det)


LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("sift_contr_key_kernel", "surf_metric_kernel")
SHARED_KERNELS = ("strongest_flag_kernel", "strongest_word_kernel")
COMPACT_KERNEL = "select_compact_kernel"   # one template in select_dev.h: sift.hip's instance moves OrientedKp, surf.hip's int4


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="needs the ROCm llvm tools")
def test_selection_kernels_use_no_scratch(aps, tmp_path):
    """The shipped gfx950 code object: the key kernels, the compactions and the shared selection kernels keep everything in
    registers (no private segment, no VGPR or SGPR spills)."""
    so = os.path.join(tmp_path, "libaps_hip.so")
    shutil.copy(aps._capi.LIB_PATH, so)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True)
    found = {}
    for co in sorted(os.path.join(tmp_path, f) for f in os.listdir(tmp_path) if f.endswith("gfx950")):
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s+- \.agpr_count:", "\n" + notes)[1:]:
            sym = re.search(r"\.symbol:\s+(\S+)", entry)
            name = next((k for k in KERNELS + SHARED_KERNELS + (COMPACT_KERNEL,) if sym and k in sym.group(1)), None)
            if name == COMPACT_KERNEL:
                name += "<OrientedKp>" if "OrientedKp" in sym.group(1) else "<int4>" if "HIP_vector_typeIiLj4E" in sym.group(1) else "<?>"
            if name:
                found.setdefault(name, []).append({k: int(re.search(r"\.%s:\s+(\S+)" % k, entry).group(1))
                                                   for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                                             "sgpr_count", "group_segment_fixed_size")})
    compactions = (COMPACT_KERNEL + "<OrientedKp>", COMPACT_KERNEL + "<int4>")
    assert sorted(found) == sorted(KERNELS + SHARED_KERNELS + compactions)
    assert all(len(found[k]) == 1 for k in KERNELS + compactions)
    assert all(len(found[k]) == 3 for k in SHARED_KERNELS)   # one copy each in fast.hip, sift.hip and surf.hip, from the one header
    for name, mds in found.items():
        for md in mds:
            print(name, md)
            assert (md["private_segment_fixed_size"], md["vgpr_spill_count"], md["sgpr_spill_count"]) == (0, 0, 0), (name, md)
