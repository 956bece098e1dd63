"""CPU tests of the batched Hamming matcher's boundary (aps_hamming_match_pairs / _pairwise): they need the built library but
no device, and fail without the feature."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fmod(aps):
    return import_module(aps.__name__ + ".featureMatching")


def test_entry_points_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aps.h")).read(), flags=re.S)
    for name in ("aps_hamming_match_pairs", "aps_hamming_match_pairwise"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and getattr(capi.lib, name).argtypes is not None
    assert [n for n, _ in capi.aps_hamming_match_opts._fields_] == ["max_ratio", "match_threshold", "unique", "nbits"]
    struct = re.search(r"typedef struct aps_hamming_match_opts \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"\b(?:double|int)\s+(\w+)\s*;", struct) == ["max_ratio", "match_threshold", "unique", "nbits"]
    assert C.sizeof(capi.aps_hamming_match_opts) == 24
    # the chunk bound is the Python wrapper's argument: no third public entry, no environment switch
    assert sorted(n for n in capi.EXPORTED_SYMBOLS if "hamming_match" in n) == ["aps_hamming_match_pairs", "aps_hamming_match_pairwise"]


class Call:
    """One valid call on two host sets of 3 x 64 bytes and the pair (0, 1); a test changes one argument and reads the status."""

    def __init__(self, capi):
        self.capi = capi
        self.A, self.B = np.zeros((3, 64), np.uint8), np.ones((3, 64), np.uint8)
        self.kw = dict(counts=[3, 3], ld=[64, 64], n_img=2, nbytes=64, layout=capi.APS_ROWMAJOR, pa=[0], pb=[1], n_pairs=1,
                       opts=(0.6, 10.0, 1, 0), cap=3, pairwise=False)

    def __call__(self, **change):
        capi, kw = self.capi, dict(self.kw, **change)
        ptrs = (C.c_void_p * 2)(capi.ptr(self.A), capi.ptr(self.B))
        counts, ld = (C.c_int64 * 2)(*kw["counts"]), (C.c_int64 * 2)(*kw["ld"])
        pa, pb = np.asarray(kw["pa"], np.int32), np.asarray(kw["pb"], np.int32)
        o = capi.aps_hamming_match_opts(*kw["opts"])
        pair_ptr, cnt = np.zeros(kw["n_pairs"] + 2, np.int64), C.c_int64(0)
        ia, ib, met = np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.float32)
        if kw["pairwise"]:
            return capi.lib.aps_hamming_match_pairwise(ptrs, counts, ld, kw["n_img"], kw["nbytes"], kw["layout"], C.byref(o), capi.ptr(pair_ptr),
                                                       capi.ptr(ia), capi.ptr(ib), capi.ptr(met), kw["cap"], C.byref(cnt))
        return capi.lib.aps_hamming_match_pairs(ptrs, counts, ld, kw["n_img"], kw["nbytes"], kw["layout"], capi.ptr(pa), capi.ptr(pb),
                                                kw["n_pairs"], C.byref(o), capi.ptr(pair_ptr), capi.ptr(ia), capi.ptr(ib), capi.ptr(met),
                                                kw["cap"], C.byref(cnt))


def test_arguments_are_checked_before_any_device_work(aps):
    """Without a device the unchanged call ends in APS_E_DEVICE; every bad argument is reported with its own code instead,
    with or without a device - so the check ran before the first device call."""
    capi = aps._capi
    call = Call(capi)
    if capi.lib.aps_device_count() == 0:
        assert call() == capi.APS_E_DEVICE and call(pairwise=True) == capi.APS_E_DEVICE
    for pw in (False, True):
        assert call(nbytes=0, pairwise=pw) == capi.APS_E_DIM and call(nbytes=65, pairwise=pw) == capi.APS_E_DIM
        assert b"1..64" in capi.lib.aps_last_error()
        assert call(opts=(0.0, 10.0, 1, 0), pairwise=pw) == capi.APS_E_ARG and call(opts=(1.0000001, 10.0, 1, 0), pairwise=pw) == capi.APS_E_ARG
        assert b"MaxRatio" in capi.lib.aps_last_error()
        assert call(opts=(0.6, -1.0, 1, 0), pairwise=pw) == capi.APS_E_ARG
        assert call(opts=(0.6, 10.0, 1, -1), pairwise=pw) == capi.APS_E_ARG and call(opts=(0.6, 10.0, 1, 513), pairwise=pw) == capi.APS_E_ARG
        assert b"nbits" in capi.lib.aps_last_error()
        assert call(nbytes=32, opts=(0.6, 10.0, 1, 257), pairwise=pw) == capi.APS_E_ARG
        assert call(layout=7, pairwise=pw) == capi.APS_E_TYPE
        assert call(cap=-1, pairwise=pw) == capi.APS_E_ARG
        assert call(counts=[3, -1], pairwise=pw) == capi.APS_E_ARG
        assert call(ld=[64, 63], pairwise=pw) == capi.APS_E_DIM   # row-major rows closer than their width
        assert call(layout=capi.APS_COLMAJOR, ld=[2, 64], pairwise=pw) == capi.APS_E_DIM   # column-major: ld < rows
    # image ids in range, two distinct images per pair
    for pa, pb in (([2], [1]), ([0], [2]), ([-1], [1]), ([0], [-1]), ([1], [1]), ([0], [0])):
        assert call(pa=pa, pb=pb) == capi.APS_E_ARG, (pa, pb)
        assert b"valid pair" in capi.lib.aps_last_error()
    assert call(pa=[0, 1], pb=[1, 1], n_pairs=2) == capi.APS_E_ARG   # the second pair of the list
    assert call(n_pairs=-1) == capi.APS_E_ARG
    assert call(n_img=-1, pairwise=True) == capi.APS_E_ARG


def test_pairs_with_an_empty_side_give_empty_csr_without_a_device(aps):
    fm = fmod(aps)
    e, a = fm.binaryFeatures(np.zeros((0, 64), np.uint8)), fm.binaryFeatures(np.ones((3, 64), np.uint8))
    p, i, j, d = fm.match_pairwise_binary_csr([e, a, e], 0.6, 10.0)   # (e, a), (e, e), (a, e)
    assert p.tolist() == [0, 0, 0, 0] and p.dtype == np.int64
    assert i.shape == (0,) and i.dtype == np.uint32 and j.shape == (0,) and j.dtype == np.uint32 and d.shape == (0,) and d.dtype == np.float32
    for uniq in (True, False):
        p, i, j, d = fm.match_pairs_binary_csr([e, a], [(0, 1), (1, 0), (0, 1)], 0.6, 10.0, Unique=uniq)
        assert p.tolist() == [0, 0, 0, 0] and len(i) == len(j) == len(d) == 0
    p, i, j, d = fm.match_pairs_binary_csr([a, a], [], 0.6, 10.0)
    assert p.tolist() == [0] and len(i) == 0
    assert fm.match_pairwise_binary_csr([a], 0.6, 10.0)[0].tolist() == [0]
    # unpacked bits, an empty side; sets of another width that meet only empty partners do not matter (as pair by pair)
    p, i, j, d = fm.match_pairs_binary_csr([np.zeros((0, 11), bool), np.ones((2, 11), bool)], [(0, 1)], 0.6, 10.0)
    assert p.tolist() == [0, 0]
    p, _, _, _ = fm.match_pairwise_binary_csr([fm.binaryFeatures(np.zeros((0, 32), np.uint8)), a], 0.6, 10.0)
    assert p.tolist() == [0, 0]
    got = fm.featureMatchingPairwise({"Matchingthreshold": 10.0, "Ratiothreshold": 0.6}, [e, a], 2)
    assert got[0][1].shape == (0, 2) and got[0][1].dtype == np.float64 and got[1][0] is None


def test_mixed_lists_raise_as_the_per_pair_branch_does(aps):
    fm = fmod(aps)
    a64, a32 = fm.binaryFeatures(np.ones((3, 64), np.uint8)), fm.binaryFeatures(np.ones((3, 32), np.uint8))
    with pytest.raises(TypeError):   # float and binary sets
        fm.match_pairwise_binary_csr([a64, np.ones((3, 128), np.float32)], 0.6, 10.0)
    with pytest.raises(TypeError):   # unpacked bits and binaryFeatures
        fm.match_pairs_binary_csr([a64, np.ones((3, 512), bool)], [(0, 1)], 0.6, 10.0)
    with pytest.raises(ValueError, match="Byte width mismatch"):
        fm.match_pairwise_binary_csr([a64, a32], 0.6, 10.0)
    with pytest.raises(ValueError, match="Byte width mismatch"):
        fm.match_pairs_binary_csr([np.ones((3, 16), bool), np.ones((3, 24), bool)], [(0, 1)], 0.6, 10.0)
    # a set of another width that meets only an empty partner is never looked at, as pair by pair
    p, _, _, _ = fm.match_pairs_binary_csr([np.zeros((0, 16), bool), np.ones((3, 24), bool), np.zeros((0, 16), bool)], [(0, 1), (1, 2)], 0.6, 10.0)
    assert p.tolist() == [0, 0, 0]
    for ratio, thr in ((0.0, 10.0), (1.5, 10.0), (0.6, -1.0)):
        with pytest.raises(ValueError):
            fm.match_pairwise_binary_csr([a64, a64], ratio, thr)
    with pytest.raises(ValueError):
        fm.match_pairs_binary_csr([a64, a64], [(0, 2)], 0.6, 10.0)
