"""GPU parity of device FAST/FREAK with the NumPy mirror at the edges of the threshold and of the quality gate that the
parameter sets of test_fast_gpu.py never touch (fast_param_cases.py names them; test_fast_param_cases.py holds each case to
its edge and to its keypoints).

Everything is integer arithmetic: the acceptance rule is test_fast_gpu.assert_equals_mirror, unchanged - locations and order,
scores, orientation bins and all 64 descriptor bytes equal."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import fast_param_cases as pc
from test_fast_gpu import assert_equals_mirror
from util import same_bits, sentinel_buffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


@pytest.fixture(scope="module")
def capi(gpu):
    return gpu._capi


def _raw(capi, img, cap, thr, num, den, max_features=0):
    """aps_fast_extract with the parameter struct's integers as given, row-major and tight, into sentinel-filled outputs of
    `cap` rows (at least one).  Returns (rc, count, desc [rows, 64], loc [2, rows], aux [rows, 4])."""
    prm = capi.aps_fast_params(thr, num, den, max_features)
    rows = max(cap, 1)
    desc = sentinel_buffer(rows * 64, np.uint8).reshape(rows, 64)
    loc = sentinel_buffer(2 * rows, np.float64).reshape(2, rows)
    aux = sentinel_buffer(rows * 4, np.float32).reshape(rows, 4)
    img = np.ascontiguousarray(img)
    cnt = C.c_int64(-1)
    rc = capi.lib.aps_fast_extract(capi.ptr(img), img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, capi.APS_IMG_U8_HWC, C.byref(prm),
                                   capi.ptr(desc), capi.APS_ROWMAJOR, 64, capi.ptr(loc), rows, capi.ptr(aux), cap, C.byref(cnt))
    return rc, int(cnt.value), desc, loc, aux


def _untouched(*arrays):
    return all(same_bits(a.reshape(-1), sentinel_buffer(a.size, a.dtype)) for a in (np.ascontiguousarray(x) for x in arrays))


def _assert_raw_matches(got, want):
    rc, cnt, desc, loc, aux = got
    n = len(want[0])
    assert rc == 0 and cnt == n
    assert_equals_mirror(np.ascontiguousarray(desc[:n]), np.ascontiguousarray(loc[:, :n].T), np.ascontiguousarray(aux[:n]), *want)
    assert _untouched(desc[n:], loc[:, n:], aux[n:]), "rows count..cap belong to the caller"


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_parameter_matrix_equals_mirror(fm, capi, case):
    want = pc.mirror(case.id)
    n = len(want[0])
    assert n == case.count and (n == 0) == (case.id in pc.EMPTY)
    assert n >= (0 if case.id in pc.EMPTY else 1 if case.id == pc.QUALITY_ONE else pc.FLOOR)
    if pc.is_raw(case):
        _assert_raw_matches(_raw(capi, pc.image(case.image), n + 3, case.thr, case.num, case.den), want)
        return
    f, loc, aux = fm.fast_extract(pc.as_input(case), pc.image(case.image), want_aux=True)
    assert isinstance(f, fm.binaryFeatures) and f.NumBits == 512 and f.NumFeatures == n
    assert_equals_mirror(f.Features, loc, aux, *want)


def test_wrapper_cases_through_their_integers(capi):
    """The gate's extremes as the C ABI sees them: q_num = 0 and q_num = q_den = 10^6, threshold 0."""
    for cid in ("q0", "q1", "thr0", "score255"):
        case = pc.BY_ID[cid]
        _assert_raw_matches(_raw(capi, pc.image(case.image), case.count + 3, *pc.integers(case)), pc.mirror(cid))


def test_quality_one_keeps_the_rows_at_the_maximum(fm):
    """The device's own two runs: MinQuality 1 is the rows of the MinQuality 0 run whose score is the largest."""
    img = pc.image(pc.BY_ID["q1"].image)
    f0, loc0, aux0 = fm.fast_extract(pc.as_input(pc.BY_ID["q0"]), img, want_aux=True)
    f1, loc1, aux1 = fm.fast_extract(pc.as_input(pc.BY_ID["q1"]), img, want_aux=True)
    top = aux0[:, 0] == aux0[:, 0].max()
    assert 1 <= top.sum() == len(loc1) < len(loc0)
    assert np.array_equal(loc1, loc0[top]) and np.array_equal(f1.Features, f0.Features[top]) and np.array_equal(aux1, aux0[top])


def test_the_boundary_rows_stay_with_num_and_go_with_num_plus_one(capi):
    img = pc.image(pc.BY_ID["boundary"].image)
    keep = _raw(capi, img, 512, 25, pc.BOUNDARY_NUM, pc.BOUNDARY_DEN)
    drop = _raw(capi, img, 512, 25, pc.BOUNDARY_NUM + 1, pc.BOUNDARY_DEN)
    assert keep[0] == 0 and drop[0] == 0
    ks, ds = keep[4][:keep[1], 0], drop[4][:drop[1], 0]
    assert ks.min() == pc.BOUNDARY_SCORE and ds.min() > pc.BOUNDARY_SCORE
    assert keep[1] - drop[1] == (ks == pc.BOUNDARY_SCORE).sum() >= 5


@pytest.mark.parametrize("bad", pc.REFUSED, ids=lambda b: "thr%d_num%d_den%d" % b)
def test_refused_parameters_leave_nothing_behind(capi, bad):
    case = pc.BY_ID["q0-small"]
    img, want = pc.image(case.image), pc.mirror(case.id)
    rc, cnt, desc, loc, aux = _raw(capi, img, case.count + 3, *bad)
    assert rc == capi.APS_E_ARG
    assert _untouched(desc, loc, aux)
    _assert_raw_matches(_raw(capi, img, case.count + 3, *pc.integers(case)), want)   # the next good call is the mirror's result
