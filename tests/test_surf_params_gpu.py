"""GPU parity of device SURF with the NumPy mirror across the parameter space: the arms of aps_surf_extract that the one
parameter set of test_surf_gpu.py never enters (surf_param_cases.py names them; test_surf_param_cases.py holds each case to
its arm and count), and the C entry's capacity, padding and refusal paths, which FAST had tested and SURF had not.

The acceptance rule is test_surf_gpu.assert_matches_mirror, unchanged: keypoint order and loc bits as uint64, scale / metric /
sign bits and descriptor bits as uint32 equal, angle_deg within 1e-3 degrees (atan2f).  Upright runs never reach atan2f:
their angle_deg is +0.0 bit for bit."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import surf_param_cases as pc
from test_surf_gpu import assert_matches_mirror, u32
from util import fetch, place, same_bits, sentinel_buffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


@pytest.fixture(scope="module")
def capi(gpu):
    return gpu._capi


def _raw(capi, img, cap, thr=1000.0, n_octaves=8, n_levels=4, upright=0, max_features=0, ldd=64, ldl=None, where="host", with_out=True):
    """aps_surf_extract, row-major, into sentinel-filled outputs of `cap` rows (at least one), all five fields of the
    parameter struct given.  Returns (rc, count, desc [rows, ldd], loc [2, ldl], aux [rows, 4])."""
    import torch

    prm = capi.aps_surf_params(thr, n_octaves, n_levels, upright, max_features)
    rows = max(cap, 1)
    ldl = rows if ldl is None else ldl
    desc = place(sentinel_buffer(rows * ldd, np.float32), where)
    loc = place(sentinel_buffer(2 * ldl, np.float64), where)
    aux = place(sentinel_buffer(rows * 4, np.float32), where)
    img = place(np.array(img), where)   # (a writable copy: the shared images are read-only, which torch does not take)
    cnt = C.c_int64(-1)
    torch.cuda.synchronize()
    pd, pl, pa = (capi.ptr(desc), capi.ptr(loc), capi.ptr(aux)) if with_out else (None, None, None)
    rc = capi.lib.aps_surf_extract(capi.ptr(img), img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, capi.APS_IMG_U8_HWC, C.byref(prm),
                                   pd, capi.APS_ROWMAJOR, ldd, pl, ldl, pa, cap, C.byref(cnt))
    capi.check(capi.lib.aps_synchronize())
    return rc, int(cnt.value), fetch(desc).reshape(rows, ldd), fetch(loc).reshape(2, ldl), fetch(aux).reshape(rows, 4)


def _untouched(*arrays):
    return all(same_bits(a.reshape(-1), sentinel_buffer(a.size, a.dtype)) for a in (np.ascontiguousarray(x) for x in arrays))


def _raw_case(capi, case, **more):
    return _raw(capi, pc.image(case.image), len(pc.mirror_of(case)[0]) + 3, case.thr, case.n_octaves, case.n_levels, int(case.upright), **more)


def _assert_raw_matches(got, want, ldd=64):
    """A raw result with spare rows against the mirror: rows 0..n by the acceptance rule, everything else the caller's."""
    rc, cnt, desc, loc, aux = got
    n = len(want[0])
    assert rc == 0 and cnt == n
    assert_matches_mirror(np.ascontiguousarray(desc[:n, :64]), np.ascontiguousarray(loc[:, :n].T), aux[:n], *want)
    assert _untouched(desc[n:], aux[n:], loc[:, n:]), "rows count..cap belong to the caller"
    if 64 < ldd < 128:
        assert _untouched(desc[:, 64:]), "64 <= ldd < 128: nothing beyond column 63"


# ---- 1. the parameter matrix ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_parameter_matrix_equals_mirror(fm, capi, case):
    want = pc.mirror_of(case)
    assert len(want[0]) == case.count if case.count is not None else len(want[0]) >= pc.COARSE_LEV6_FLOOR
    assert (len(want[0]) == 0) == (case.id in pc.EMPTY)
    if pc.needs_raw_abi(case):   # upright: the wrapper sends 0
        got = _raw_case(capi, case)
        _assert_raw_matches(got, want)
        n = len(want[0])
        assert np.array_equal(u32(got[4][:n, 1]), np.zeros(n, np.uint32)), "upright: angle_deg is exactly +0.0"
        return
    d, loc, aux = fm.surf_extract(pc.as_input(case), pc.image(case.image), want_aux=True)
    if case.id in pc.EMPTY:
        assert d.shape == (0, 64) and loc.shape == (0, 2) and aux.shape == (0, 4)
    assert_matches_mirror(d, loc, aux, *want)


def test_upright_differs_from_the_oriented_run_only_where_it_should(fm, capi):
    """The device's own two runs: same keypoints, angle 0 against a turned one, other descriptors."""
    case = pc.BY_ID["upright-small"]
    rc, n, desc, loc, aux = _raw_case(capi, case)
    assert rc == 0
    d, oloc, oaux = fm.surf_extract({"detector": "SURF"}, pc.image(case.image), want_aux=True)
    assert n == len(d) == case.count
    assert np.array_equal(np.ascontiguousarray(loc[:, :n].T).view(np.uint64), oloc.view(np.uint64))
    for col in (0, 2, 3):
        assert np.array_equal(u32(aux[:n, col]), u32(oaux[:, col]))
    assert (oaux[:, 1] != 0).mean() > 0.9 and not u32(aux[:n, 1]).any()
    assert (u32(desc[:n]) != u32(d)).any(1).mean() > 0.9


def test_lev8_through_the_raw_abi_too(capi):
    """Six bitmap planes per octave through both entries: the wrapper (the matrix above) and the C ABI."""
    case = pc.BY_ID["lev8"]
    _assert_raw_matches(_raw_case(capi, case), pc.mirror_of(case))


@pytest.mark.parametrize("where", ["host", "device"])
def test_threshold_above_every_response_writes_nothing(capi, where):
    """A four-octave plan, an all-zero bitmap: rc 0, count 0, and the kernels of the capacity grid leave the outputs alone."""
    case = pc.BY_ID["thr-huge"]
    rc, cnt, desc, loc, aux = _raw(capi, pc.image(case.image), 64, case.thr, case.n_octaves, case.n_levels, where=where)
    assert rc == 0 and cnt == 0
    assert _untouched(desc, loc, aux)


# ---- 2. the C entry's edges, on 97 x 131 at the default parameters ---------------------------------------------------------
def _edge():
    return pc.image(pc.EDGE_IMAGE), pc.mirror(pc.EDGE_IMAGE)


def test_capacity_zero_counts_and_writes_nothing(capi):
    img, want = _edge()
    rc, cnt, desc, loc, aux = _raw(capi, img, 0)
    assert rc == capi.APS_E_CAP and cnt == len(want[0]) > 0
    assert _untouched(desc, loc, aux)


def test_null_outputs_with_features_present(capi):
    img, want = _edge()
    rc, cnt, *_ = _raw(capi, img, len(want[0]), with_out=False)
    assert cnt == len(want[0]) and rc == capi.APS_E_ARG   # the count is reported; there is nothing to put the features in


def test_max_features_is_a_limit_on_the_count(capi):
    img, want = _edge()
    n = len(want[0])
    rc, cnt, *_ = _raw(capi, img, n, max_features=n - 1)
    assert rc == capi.APS_E_CAP and cnt == n
    assert b"max_features" in capi.lib.aps_last_error()
    rc, cnt, desc, loc, aux = _raw(capi, img, n, max_features=n)
    assert rc == 0 and cnt == n
    assert_matches_mirror(desc, np.ascontiguousarray(loc.T), aux, *want)


@pytest.mark.parametrize("where", ["host", "device"])
def test_padded_outputs_keep_their_padding(capi, where):
    """cap = n + 3, ldl = cap + 5, ldd = 80: the columns 64..79 of every row, the rows n..cap of desc and aux and the tail of
    both rows of loc stay the caller's, for host and for device pointers."""
    img, want = _edge()
    cap = len(want[0]) + 3
    got = _raw(capi, img, cap, ldd=80, ldl=cap + 5, where=where)
    assert got[3].shape == (2, cap + 5)
    _assert_raw_matches(got, want, ldd=80)


@pytest.mark.parametrize("bad", [dict(n_octaves=0), dict(n_octaves=13), dict(n_levels=2), dict(n_levels=9), dict(thr=-1.0)],
                         ids=lambda b: "%s=%g" % next(iter(b.items())))
def test_refused_parameters_leave_nothing_behind(capi, bad):
    img, want = _edge()
    cap = len(want[0]) + 3
    rc, cnt, desc, loc, aux = _raw(capi, img, cap, **bad)
    assert rc == capi.APS_E_ARG
    assert _untouched(desc, loc, aux)
    _assert_raw_matches(_raw(capi, img, cap), want)   # the next good call is the mirror's result
