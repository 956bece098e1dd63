"""CPU tests of the boundary of aps_kaze_extract_select: they need the built library but no device, and fail without the feature.
The last test reads the shipped gfx950 code object: the new and re-instantiated kernels keep everything in registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["kaze", "select", "n_select", "grid_rows", "grid_cols", "upright"]


def test_entry_point_is_declared_bound_and_exported(aps):
    capi = aps._capi
    header = open(os.path.join(ROOT, "include", "aps.h")).read()
    assert re.search(r"\bint\s+aps_kaze_extract_select\s*\(", header)
    assert "aps_kaze_extract_select" in capi.EXPORTED_SYMBOLS
    assert hasattr(C.CDLL(capi.LIB_PATH), "aps_kaze_extract_select") and hasattr(capi.lib, "aps_kaze_extract_select")
    st = capi.aps_kaze_select_params
    assert [n for n, _ in st._fields_] == FIELDS
    assert dict(st._fields_)["kaze"] is capi.aps_kaze_params and all(dict(st._fields_)[n] is C.c_int for n in FIELDS[1:])
    body = re.search(r"typedef struct aps_kaze_select_params \{(.*?)\} aps_kaze_select_params;", header, re.S).group(1)
    assert re.findall(r"(?:aps_kaze_params|int)\s+(\w+);", body) == FIELDS
    assert C.sizeof(st) == C.sizeof(capi.aps_kaze_params) + 5 * 4 + 4   # (8-byte alignment of the nested double)
    assert st.select.offset == C.sizeof(capi.aps_kaze_params) and st.upright.offset == st.select.offset + 16
    # the argument list is aps_kaze_extract's, with the new struct; the parent's struct keeps its fields
    sig, psig = capi._SIGNATURES["aps_kaze_extract_select"], capi._SIGNATURES["aps_kaze_extract"]
    assert len(sig) == len(psig) == 14 and sig[:5] == psig[:5] and sig[6:] == psig[6:] and sig[5] is not psig[5]
    assert [n for n, _ in capi.aps_kaze_params._fields_] == ["threshold", "num_octaves", "num_scale_levels", "diffusion", "max_features"]


def test_arguments_are_checked_before_any_device_work(aps):
    """Every refusal of the new fields and every refusal of aps_kaze_extract comes back as APS_E_ARG (or the layout's / shape's own
    code) with or without a device, ahead of APS_E_DEVICE."""
    capi = aps._capi
    cnt = C.c_int64(0)
    one = np.zeros(16, np.uint8)
    ok = capi.aps_kaze_params(1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_REGION, 0)
    S = lambda select=0, n=0, rows=0, cols=0, upright=0, kaze=ok: capi.aps_kaze_select_params(kaze, select, n, rows, cols, upright)   # noqa: E731

    def call(prm, h=64, w=64, c=1, img_layout=capi.APS_IMG_U8_HWC, desc_layout=capi.APS_ROWMAJOR, img=one, count=cnt, cap=0):
        return capi.lib.aps_kaze_extract_select(capi.ptr(img), h, w, c, img_layout, C.byref(prm) if prm is not None else None, None,
                                                desc_layout, 64, None, 0, None, cap, C.byref(count) if count is not None else None)

    for prm, word in ((S(select=3), b"select"), (S(select=-1), b"select"), (S(select=1, n=0), b"n_select"), (S(select=1, n=-4), b"n_select"),
                      (S(select=2, n=0, rows=8, cols=8), b"NumUniform"), (S(select=2, n=10, rows=0, cols=8), b"UniformGrid"),
                      (S(select=2, n=10, rows=8, cols=33), b"UniformGrid"), (S(select=2, n=10, rows=33, cols=8), b"UniformGrid"),
                      (S(select=2, n=10, rows=8, cols=0), b"UniformGrid"), (S(upright=2), b"upright"), (S(upright=-1), b"upright"),
                      (S(select=1, n=10, upright=5), b"upright")):
        assert call(prm) == capi.APS_E_ARG and word in capi.lib.aps_last_error(), word
    assert call(None) == capi.APS_E_ARG and call(S(), img=None) == capi.APS_E_ARG and call(S(), count=None) == capi.APS_E_ARG
    P = capi.aps_kaze_params
    for kaze, word in ((P(1e-4, 0, 4, 0, 0), b"NumOctaves"), (P(1e-4, 5, 4, 0, 0), b"NumOctaves"), (P(1e-4, 3, 2, 0, 0), b"NumScaleLevels"),
                       (P(1e-4, 3, 11, 0, 0), b"NumScaleLevels"), (P(-1e-4, 3, 4, 0, 0), b"Threshold"),
                       (P(1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_SHARPEDGE, 0), b"not built"), (P(1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_EDGE, 0), b"not built"),
                       (P(1e-4, 3, 4, 7, 0), b"Diffusion")):
        for prm in (S(kaze=kaze), S(select=1, n=10, kaze=kaze), S(select=2, n=10, rows=8, cols=8, upright=1, kaze=kaze)):
            assert call(prm) == capi.APS_E_ARG and word in capi.lib.aps_last_error(), word
    good = S(select=2, n=10, rows=8, cols=8, upright=1)
    assert call(good, cap=-1) == capi.APS_E_ARG
    assert call(good, h=50000, w=50000) == capi.APS_E_ARG and b"2^31" in capi.lib.aps_last_error()
    assert call(good, h=0) == capi.APS_E_DIM and call(good, c=2) == capi.APS_E_DIM
    assert call(good, img_layout=99) == capi.APS_E_TYPE and call(good, desc_layout=99) == capi.APS_E_TYPE
    # fields that the selection does not read are not checked: the grid without select == 2, N without a selection
    if capi.lib.aps_device_count() == 0:
        for prm in (good, S(), S(select=1, n=5, rows=99, cols=-3), S(n=-7, rows=99)):
            assert call(prm) == capi.APS_E_DEVICE


def test_the_wrappers_pass_the_keys(aps):
    """Both selection keys together are a ValueError before any library call; each key alone reaches the library: a value the
    library refuses is its APS_E_ARG (without the feature the keys are ignored and the call gets as far as the device)."""
    capi = aps._capi
    fm = import_module(aps.__name__ + ".featureMatching")
    pl = import_module(aps.__name__ + ".pipeline")
    img = np.zeros((64, 64, 3), np.uint8)
    calls = (lambda inp: fm.kaze_extract(inp, img), lambda inp: fm.extract_features(inp, img), lambda inp: pl.extract_features(inp, [img]))
    for call in calls:
        with pytest.raises(ValueError):
            call({"detector": "KAZE", "NumStrongest": 10, "NumUniform": 10})
        for bad in ({"NumStrongest": 0}, {"NumUniform": -2}, {"NumUniform": 10, "UniformGrid": (0, 8)}, {"NumUniform": 10, "UniformGrid": (8, 40)},
                    {"NumStrongest": 0, "Upright": True}):
            with pytest.raises(aps.ApsError) as e:
                call(dict(bad, detector="KAZE"))
            assert e.value.code == capi.APS_E_ARG, bad
    for keys in ({"NumStrongest": 10}, {"NumUniform": 10}, {"Upright": True}, {"NumUniform": 10, "UniformGrid": (4, 4), "Upright": True}):
        try:
            f, pts = fm.kaze_extract(dict(keys, detector="KAZE"), img)
        except aps.ApsError as e:
            assert capi.lib.aps_device_count() == 0 and e.code == capi.APS_E_DEVICE
        else:
            assert f.shape == (0, 64) and pts.shape == (0, 2)
    assert not any(k in pl.default_input(detector="KAZE") for k in ("NumStrongest", "NumUniform", "UniformGrid", "Upright"))
    with pytest.raises(NotImplementedError):
        fm.getFeaturePoints({"detector": "KAZE", "NumStrongest": 10}, img)


def test_surf_params_carry_upright(aps):
    fm = import_module(aps.__name__ + ".featureMatching")
    assert fm._surf_params({}).upright == 0 and fm._surf_params({"Upright": False}).upright == 0
    assert fm._surf_params({"Upright": True}).upright == 1
    assert fm._surf_strongest_params({"Upright": True, "NumStrongest": 7}).surf.upright == 1
    assert fm._uniform_params(aps._capi.aps_surf_uniform_params, fm._surf_strongest_params({"Upright": True}, 7), (7, 8, 8)).strongest.surf.upright == 1


LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("kaze_key_kernel", "kaze_keypoint_kernelILb0", "kaze_keypoint_kernelILb1", "kaze_emit_kernel")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="needs the ROCm llvm tools")
def test_kaze_selection_kernels_use_no_scratch(aps, tmp_path):
    """The shipped gfx950 code object: the key kernel and both instantiations of the keypoint kernel have no private segment and no
    VGPR or SGPR spills, and the keypoint kernel's LDS is what its three arrays take in either form."""
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
                found.setdefault(name, []).append({k: int(re.search(r"\.%s:\s+(\S+)" % k, entry).group(1))
                                                   for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                                             "sgpr_count", "group_segment_fixed_size")})
    assert sorted(found) == sorted(KERNELS) and all(len(v) == 1 for v in found.values()), found
    for name, (md,) in found.items():
        print(name, md)
        assert (md["private_segment_fixed_size"], md["vgpr_spill_count"], md["sgpr_spill_count"]) == (0, 0, 0), (name, md)
    lds = 4 * (4 * 32 + 2 * 4 * 24 * 24)
    assert found["kaze_keypoint_kernelILb0"][0]["group_segment_fixed_size"] == found["kaze_keypoint_kernelILb1"][0]["group_segment_fixed_size"] == lds
