"""CPU tests of the uniform-N boundary (DESIGN.md "Uniform-N selection"): they need the built library but no device, and fail
without the feature.  The host-only entries aps_uniform_quota and aps_uniform_cell - the functions the device kernels call - are
held against tests/uniform_mirror.py."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

import strongest_cases as sc
import uniform_mirror as um
from test_uniform_mirror import HAND

ENTRIES = ("aps_sift_extract_uniform", "aps_surf_extract_uniform", "aps_fast_extract_uniform")
NAMES = ENTRIES + ("aps_uniform_quota", "aps_uniform_cell")


def test_entry_points_are_declared_bound_and_exported(aps):
    capi = aps._capi
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "aps.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and hasattr(capi.lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    for det in ("sift", "surf", "fast"):
        st, parent = getattr(capi, "aps_%s_uniform_params" % det), getattr(capi, "aps_%s_strongest_params" % det)
        assert [n for n, _ in st._fields_] == ["strongest", "grid_rows", "grid_cols"]
        assert dict(st._fields_)["strongest"] is parent and dict(st._fields_)["grid_rows"] is dict(st._fields_)["grid_cols"] is C.c_int
        assert C.sizeof(st) == C.sizeof(parent) + 2 * C.sizeof(C.c_int)
        assert re.search(r"typedef struct aps_%s_uniform_params \{\s*aps_%s_strongest_params strongest;[^}]*int grid_rows, grid_cols;[^}]*\}"
                         % (det, det), header)
        # the argument list is the strongest entry's, with the new struct
        sig, psig = capi._SIGNATURES["aps_%s_extract_uniform" % det], capi._SIGNATURES["aps_%s_extract_strongest" % det]
        assert len(sig) == len(psig) == 14 and sig[:5] == psig[:5] and sig[6:] == psig[6:] and sig[5] is not psig[5]
    # the strongest structs keep their fields
    assert [n for n, _ in capi.aps_sift_strongest_params._fields_] == ["sift", "n_strongest"]
    assert [n for n, _ in capi.aps_surf_strongest_params._fields_] == ["surf", "n_strongest"]
    assert [n for n, _ in capi.aps_fast_strongest_params._fields_] == ["pyramid", "n_strongest"]


# ---- the host-only entries against the mirror ----------------------------------------------------------------------------------
def quota(capi, counts, Q):
    c = np.ascontiguousarray(counts, np.int64)
    keep = np.full(len(c) + 1, -77, np.int64)
    capi.check(capi.lib.aps_uniform_quota(capi.ptr(c), len(c), int(Q), capi.ptr(keep)))
    assert keep[-1] == -77
    return keep[:-1]


def test_quota_equals_the_mirror(aps):
    capi = aps._capi
    for counts, Q, want in HAND:
        assert quota(capi, counts, Q).tolist() == want == um.waterfill(counts, Q).tolist()
    rng = np.random.default_rng(12)
    for _ in range(300):
        m = int(rng.choice([1, 2, 15, 64, 97, 1024]))
        c = rng.integers(0, int(rng.choice([2, 5, 40, 3000])), m) * (rng.random(m) < rng.choice([0.2, 1.0]))
        total = int(c.sum())
        for Q in {0, 1, total, max(total - 1, 0), int(rng.integers(0, total + 1)), total + 9}:
            assert np.array_equal(quota(capi, c, Q), um.waterfill(c, Q)), (c.tolist(), Q)
    big = np.array([2 ** 32 - 1, 5, 2 ** 31], np.int64)   # the largest counts the entry takes
    assert quota(capi, big, 2 ** 32).tolist() == [2 ** 31 - 2, 5, 2 ** 31 - 3] == um.waterfill(big, 2 ** 32).tolist()


def test_quota_on_the_pairA_counts(aps):
    img, ref = sc.surf_reference("pairA")
    py, px, (H, W), metric = um.surf_pixels(img, 1000.0)
    counts = np.bincount(um.cell(py, px, H, W, (8, 8)), minlength=64)
    for N in (58, 146, 583, 584):
        k = quota(aps._capi, counts, N)
        assert np.array_equal(k, um.waterfill(counts, N)) and int(k.sum()) == N
        assert int((k > 0).sum()) == min(N, 64)


def test_quota_refuses_bad_arguments(aps):
    capi = aps._capi
    c, k = np.ones(4, np.int64), np.zeros(4, np.int64)
    q = capi.lib.aps_uniform_quota
    assert q(None, 4, 2, capi.ptr(k)) == capi.APS_E_ARG and q(capi.ptr(c), 4, 2, None) == capi.APS_E_ARG
    assert q(capi.ptr(c), 0, 2, capi.ptr(k)) == capi.APS_E_ARG and q(capi.ptr(c), 1025, 2, capi.ptr(k)) == capi.APS_E_ARG
    assert q(capi.ptr(c), 4, -1, capi.ptr(k)) == capi.APS_E_ARG
    for bad in (-1, 2 ** 32):
        assert q(capi.ptr(np.array([1, bad, 1, 1], np.int64)), 4, 2, capi.ptr(k)) == capi.APS_E_ARG
    assert not k.any()


def cell(capi, py, px, Hp, Wp, grid):
    out = C.c_int(-1)
    capi.check(capi.lib.aps_uniform_cell(py, px, Hp, Wp, grid[0], grid[1], C.byref(out)))
    return out.value


@pytest.mark.parametrize("shape,grid", [((97, 131), (3, 5)), ((97, 131), (8, 8)), ((37, 37), (32, 32)), ((240, 320), (8, 8)),
                                        ((5, 7), (32, 32)), ((120, 160), (1, 1)), ((33, 1), (32, 1))])
def test_cell_equals_the_mirror(aps, shape, grid):
    capi = aps._capi
    Hp, Wp = shape
    ys = sorted(set(range(0, Hp, max(Hp // 40, 1))) | {Hp - 1})
    xs = sorted(set(range(0, Wp, max(Wp // 40, 1))) | {Wp - 1})
    got = np.array([[cell(capi, y, x, Hp, Wp, grid) for x in xs] for y in ys])
    assert np.array_equal(got, um.cell(np.array(ys)[:, None], np.array(xs)[None, :], Hp, Wp, grid))
    assert got[0, 0] == 0
    if Hp >= grid[0] and Wp >= grid[1]:   # (a plane with fewer pixels than cells along a side does not reach the last cell)
        assert got[-1, -1] == grid[0] * grid[1] - 1


def test_cell_refuses_bad_arguments(aps):
    capi = aps._capi
    out = C.c_int(-1)
    f = capi.lib.aps_uniform_cell
    assert f(0, 0, 10, 10, 8, 8, None) == capi.APS_E_ARG
    for py, px in ((-1, 0), (10, 0), (0, -1), (0, 10)):
        assert f(py, px, 10, 10, 8, 8, C.byref(out)) == capi.APS_E_ARG
    for grid in ((0, 8), (8, 0), (33, 8), (8, 33)):
        assert f(0, 0, 10, 10, *grid, C.byref(out)) == capi.APS_E_ARG and b"UniformGrid" in capi.lib.aps_last_error()
    assert f(0, 0, 0, 10, 8, 8, C.byref(out)) == capi.APS_E_DIM
    assert out.value == -1


# ---- the three entries' argument checks ----------------------------------------------------------------------------------------
def _entries(capi):
    sift = capi.aps_sift_params(1.6, 4, 0.00133, 6.0, 0)
    surf = capi.aps_surf_params(1000.0, 8, 4, 0, 0)
    pyr = capi.aps_fast_pyramid_params(capi.aps_fast_params(12, 100000, 1000000, 0), 1, 1200000, 1000000)
    return (("sift", capi.lib.aps_sift_extract_uniform,
             lambda n, r, c: capi.aps_sift_uniform_params(capi.aps_sift_strongest_params(sift, n), r, c), 128),
            ("surf", capi.lib.aps_surf_extract_uniform,
             lambda n, r, c: capi.aps_surf_uniform_params(capi.aps_surf_strongest_params(surf, n), r, c), 64),
            ("fast", capi.lib.aps_fast_extract_uniform,
             lambda n, r, c: capi.aps_fast_uniform_params(capi.aps_fast_strongest_params(pyr, n), r, c), 64))


def test_arguments_are_checked_before_any_device_work(aps):
    """N below 1 and a grid value outside 1..32 come back as APS_E_ARG without a device (this test runs where there is none), ahead
    of APS_E_DEVICE; so do the parents' refusals and NULL params / count."""
    capi = aps._capi
    one = np.zeros(64 * 64, np.uint8)
    for det, entry, make, ldd in _entries(capi):
        cnt = C.c_int64(0)

        def extract(h, w, prm, ch=1, count=cnt):
            return entry(capi.ptr(one), h, w, ch, capi.APS_IMG_U8_HWC, None if prm is None else C.byref(prm), None, capi.APS_ROWMAJOR, ldd, None,
                         0, None, 0, None if count is None else C.byref(count))

        for bad in (0, -1):
            assert extract(64, 64, make(bad, 8, 8)) == capi.APS_E_ARG, (det, bad)
            assert b"NumUniform" in capi.lib.aps_last_error()
        for grid in ((0, 8), (8, 0), (33, 8), (8, 33), (-1, 8)):
            assert extract(64, 64, make(10, *grid)) == capi.APS_E_ARG, (det, grid)
            assert b"UniformGrid" in capi.lib.aps_last_error()
        assert extract(64, 64, None) == capi.APS_E_ARG and extract(64, 64, make(10, 8, 8), count=None) == capi.APS_E_ARG
        assert extract(0, 64, make(10, 8, 8)) == capi.APS_E_DIM and extract(64, 64, make(10, 8, 8), ch=2) == capi.APS_E_DIM
        if capi.lib.aps_device_count() == 0:
            for grid in ((1, 1), (8, 8), (32, 32), (3, 5)):
                assert extract(64, 64, make(10, *grid)) == capi.APS_E_DEVICE, (det, grid)


# ---- the Python operators ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", ["SIFT", "SURF", "FAST"])
def test_the_wrappers_pass_the_keys(aps, det):
    """NumUniform and UniformGrid reach the library through every host entry that extracts features: a bad value is the library's
    APS_E_ARG (without the feature the keys are ignored and the call gets as far as the device: APS_E_DEVICE here)."""
    capi = aps._capi
    fm = import_module(aps.__name__ + ".featureMatching")
    pl = import_module(aps.__name__ + ".pipeline")
    img = np.zeros((64, 64, 3), np.uint8)
    extract = {"SIFT": fm.sift_extract, "SURF": fm.surf_extract, "FAST": fm.fast_extract}[det]
    calls = (lambda inp: extract(inp, img), lambda inp: fm.getFeaturePoints(inp, img), lambda inp: fm.extract_features(inp, img),
             lambda inp: pl.extract_features(inp, [img]))
    for bad in ({"NumUniform": 0}, {"NumUniform": -5}, {"NumUniform": 10, "UniformGrid": (0, 8)}, {"NumUniform": 10, "UniformGrid": (8, 33)}):
        for call in calls:
            with pytest.raises(aps.ApsError) as e:
                call({"detector": det, **bad})
            assert e.value.code == capi.APS_E_ARG
    for call in calls:   # both selection rules: refused in Python, before any library call
        with pytest.raises(ValueError, match="NumUniform"):
            call({"detector": det, "NumUniform": 10, "NumStrongest": 10})
    good = {"detector": det, "NumUniform": 10, "UniformGrid": (3, 5)}
    if capi.lib.aps_device_count() > 0:
        assert len(extract(good, img)[1]) == 0
    else:
        with pytest.raises(aps.ApsError) as e:
            extract(good, img)
        assert e.value.code == capi.APS_E_DEVICE
    # UniformGrid without NumUniform is ignored: the call is the one without any key, whatever the grid says
    if capi.lib.aps_device_count() == 0:
        with pytest.raises(aps.ApsError) as e:
            extract({"detector": det, "UniformGrid": (0, 99)}, img)
        assert e.value.code == capi.APS_E_DEVICE
    for key in ("NumUniform", "UniformGrid"):
        assert key not in pl.default_input() and key not in pl.default_input(detector=det) and key not in getattr(pl, "DEFAULT_INPUT", {})


def test_the_parameter_structs_carry_the_keys(aps):
    capi = aps._capi
    fm = import_module(aps.__name__ + ".featureMatching")
    assert fm._uniform_keys({"NumStrongest": 5, "UniformGrid": (2, 2)}) is None
    assert fm._uniform_keys({"NumUniform": 7}) == (7, 8, 8) and fm._uniform_keys({"NumUniform": 7, "UniformGrid": (3, 5)}) == (7, 3, 5)
    inp = {"NumUniform": 7, "UniformGrid": (3, 5), "maxFeatures": 123, "NumLevels": 4}
    u = fm._uniform_keys(inp)
    p = fm._uniform_params(capi.aps_sift_uniform_params, fm._sift_strongest_params(inp, u[0]), u)
    assert (p.strongest.n_strongest, p.grid_rows, p.grid_cols, p.strongest.sift.max_features) == (7, 3, 5, 123)
    p = fm._uniform_params(capi.aps_surf_uniform_params, fm._surf_strongest_params(inp, u[0]), u)
    assert (p.strongest.n_strongest, p.grid_rows, p.grid_cols, p.strongest.surf.max_features) == (7, 3, 5, 123)
    p = fm._uniform_params(capi.aps_fast_uniform_params, fm._fast_strongest_params(inp, 4, u[0]), u)
    assert (p.strongest.n_strongest, p.grid_rows, p.grid_cols, p.strongest.pyramid.n_levels) == (7, 3, 5, 4)


def test_stitch_distributed_keeps_refusing_fast(aps):
    par = import_module(aps.__name__ + ".parallel")
    with pytest.raises(NotImplementedError):
        par.stitch_distributed({"detector": "FAST", "NumUniform": 100}, {}, 0, None)
