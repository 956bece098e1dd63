"""featureMatchingGlobal's device chain across its parameter space: aps_global_normalize -> aps_knn_global_screened (or the
blocked aps_knn_global) -> aps_global_filter, on the fixtures of global_cases.py (test_global_cases.py holds each fixture to
the arm it is there for).  Every comparison is against the CPU oracle and bit for bit: indices, distance bits, CSR lists.
No tolerance appears anywhere - the kernels compute the oracle's canonical f32 arithmetic or they are wrong.

  images smaller than a wave, an empty one, a tiny last one (mosaic)      the `edge` appends of global_screen_reduce_kernel /
                                                                         global_phase_b_kernel, 1-, 2-, 3-row column sets
  two images, one image (pair2, solo)                                    a1 = a2 = -1; no cross-image job at all
  four near rows in one image / block, exact duplicates (crowded, blocked_pools)   the exact-rows repair, ties by index
  APS_KNN_MODE=f32, APS_MATCH_NO_SCREEN, APS_MATCH_NO_POOL, APS_KNN_SLOT_CAP        every switch of the search, same lists
  last blocks of 1, 2, 3 rows, one block, raw and badly scaled pools, k = 1..4      the blocked aps_knn_global
  APS_COLMAJOR, padded ld / ldo, resident arguments                      on the screened and the blocked path
  ft x fq x k sweep around the 64-row train tile and the 128-row query tile        knn_f32_kernel<4|8>
  synthetic neighbour tables                                             aps_global_filter alone
  every <NW, K> of hamming_knn_kernel"""
import ctypes as C
import re
from importlib import import_module

import numpy as np
import pytest

import global_cases as gc
import oracle
from util import bits, fetch, padded, place, same_bits, sentinel_buffer, sift_like, unpad

pytestmark = pytest.mark.gpu

WHERE = ["host", "device"]
SWITCHES = ("APS_KNN_MODE", "APS_MATCH_NO_SCREEN", "APS_MATCH_NO_POOL", "APS_KNN_SLOT_CAP", "APS_KNN_BLOCK", "APS_TRACE")
# APS_KNN_SLOT_CAP that cuts the query images into passes INSIDE a run of tiny images (a pass takes images while
# rows * n_img stays within the cap): mosaic's passes are images {0, 1, 2}, {3}, {4}, ... ; crowded's {0, 1, 2}, {3, 4}, ...
SECOND_CAP = {"mosaic": 34 * 8, "pair2": 2 * 5000, "solo": 1, "crowded": 12 * 1600}


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


@pytest.fixture(scope="module")
def capi(gpu):
    return gpu._capi


@pytest.fixture(autouse=True)
def _no_switch_set(monkeypatch):
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)


def _call(capi, fn, *args):
    """One ABI call bracketed the way a resident caller brackets it (test_abi_layouts_gpu._call)."""
    import torch

    torch.cuda.synchronize()
    rc = fn(*args)
    capi.check(capi.lib.aps_synchronize())
    return rc


def _with_env(monkeypatch, env, fn):
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    try:
        return fn()
    finally:
        for key in env:
            monkeypatch.delenv(key)


def _flat(a, colmajor):
    """A writable flat copy of matrix a, tight, row- or column-major."""
    return np.array(a.T if colmajor else a, order="C").reshape(-1)


def _screen_stats(capi):
    rows, surv = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib.aps_knn_global_screen_stats(C.byref(rows), C.byref(surv)))
    return rows.value, surv.value


# ---- the screened pooled search, table level ---------------------------------------------------------------------------------
def _screened(capi, pool, sizes, ratio, k, colmajor=False, ld=None, ldo=None, where="host"):
    """aps_knn_global_screened -> (idx, dist, padding intact)."""
    f = len(pool)
    ld = ld or (f if colmajor else 128)
    ldo = ldo or (f if colmajor else k)
    src = place(padded(pool, colmajor, ld) if ld != (f if colmajor else 128) else _flat(pool, colmajor), where)
    n_out = (k if colmajor else f) * ldo
    idx, dist = place(sentinel_buffer(n_out, np.uint32), where), place(sentinel_buffer(n_out, np.float32), where)
    off = gc.offsets(sizes)
    capi.check(_call(capi, capi.lib.aps_knn_global_screened, capi.ptr(src), f, ld, 128, capi.APS_COLMAJOR if colmajor else capi.APS_ROWMAJOR,
                     capi.ptr(off), len(sizes), float(ratio), k, capi.ptr(idx), capi.ptr(dist), ldo))
    if ldo == (f if colmajor else k):
        shape = (k, f) if colmajor else (f, k)
        i, d = fetch(idx, np.uint32).reshape(shape), fetch(dist).reshape(shape)
        return (np.ascontiguousarray(i.T), np.ascontiguousarray(d.T), True) if colmajor else (i, d, True)
    i, ok_i = unpad(fetch(idx, np.uint32), f, k, colmajor, ldo)
    d, ok_d = unpad(fetch(dist), f, k, colmajor, ldo)
    return i, d, ok_i and ok_d


def _check_screened_table(name, ratio, k, idx, dist):
    """Every row is the oracle's, bits and all, or a dismissed one (k copies of itself at distance 0) that the oracle chain
    accepts no match for."""
    _, oi, od, _, _ = gc.pool_knn(name, k)
    f = len(oi)
    exact = (idx == oi).all(axis=1) & (bits(dist) == bits(od)).all(axis=1)
    dismissed = (idx == np.arange(1, f + 1, dtype=np.uint32)[:, None]).all(axis=1) & (bits(dist) == 0).all(axis=1)
    bad = np.flatnonzero(~exact & ~dismissed)
    assert len(bad) == 0, (name, ratio, k, bad[:8], idx[bad[:4]], oi[bad[:4]])
    accepted = gc.accepted_queries(name, ratio, k)
    wrong = np.intersect1d(np.flatnonzero(~exact), accepted)
    assert len(wrong) == 0, (name, ratio, k, "dismissed rows the oracle accepts", wrong[:8])
    return int((~exact).sum()), len(accepted)


@pytest.mark.parametrize("name", list(gc.POOLS))
def test_screened_search_rows_are_the_oracles_or_provably_dropped(capi, name):
    pool = gc.pool_knn(name, 4)[0]
    sizes = gc.POOL_SIZES[name]
    f = len(pool)
    seen_dismissed = 0
    for k in (1, 2, 3, 4):
        for ratio in gc.RATIOS:
            idx, dist, _ = _screened(capi, pool, sizes, ratio, k)
            n_dismissed, n_accepted = _check_screened_table(name, ratio, k, idx, dist)
            rows, surv = _screen_stats(capi)
            assert rows == f and n_accepted <= surv <= f, (name, ratio, k, rows, surv, n_accepted)
            seen_dismissed += n_dismissed if k > 1 else 0
            if name == "crowded" and k == 4:  # the planted rows come back exactly (the `own` one through the repair)
                _, oi, od, _, _ = gc.pool_knn(name, 4)
                for key in ("own", "other"):
                    q = gc.pool_row(name, *gc.CROWDED_PLANTS[key]["row"])
                    assert np.array_equal(idx[q], oi[q]) and np.array_equal(bits(dist[q]), bits(od[q])), (key, ratio)
    if len(sizes) > 1:
        assert seen_dismissed > 0     # the screen does dismiss rows on this pool: both arms of the check above ran


@pytest.mark.parametrize("name", list(gc.POOLS))
def test_screen_statistics_are_pinned(capi, capfd, name):
    """Bit-exact tables cannot see a screen that dismisses fewer rows than it did: the result is the same, only the work
    grows.  aps_knn_global_screen_stats' (rows, survivors) at k = 4 are counts, not orders of atomics: pinned."""
    pool = gc.pool_knn(name, 4)[0]
    got = {}
    for ratio in gc.RATIOS:
        _screened(capi, pool, gc.POOL_SIZES[name], ratio, 4)
        got[ratio] = _screen_stats(capi)
        with capfd.disabled():
            print(name, ratio, "(rows, survivors)", got[ratio])
    assert got == {ratio: (len(pool), gc.SCREEN_SURVIVORS[name][ratio]) for ratio in gc.RATIOS}, name


# ---- the same at list level, under every switch ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.POOLS))
def test_match_lists_equal_the_oracle_chain_under_every_switch(fm, capi, monkeypatch, name):
    descs = list(gc.POOLS[name]())
    sizes = gc.POOL_SIZES[name]
    n_img = len(sizes)
    f = sum(sizes)
    want = gc.csr_of(gc.pool_chain(name, 0.6, 4), n_img, fm.pair_order(n_img))
    assert want[0][-1] == gc.PINNED[name][1][0.6][0]
    runs = {"default": {}, "f32": {"APS_KNN_MODE": "f32"}, "no_screen": {"APS_MATCH_NO_SCREEN": "1"},
            "no_pool": {"APS_MATCH_NO_POOL": "1"}, "cap1": {"APS_KNN_SLOT_CAP": "1"},
            "cap_tiny": {"APS_KNN_SLOT_CAP": str(SECOND_CAP[name])}}
    got = {}
    for run, env in runs.items():
        got[run] = _with_env(monkeypatch, env, lambda: fm.match_global_csr(descs, 0.6, 4))
        if run != "f32":
            rows, surv = _screen_stats(capi)
            assert rows == f and want[0][-1] <= surv <= f, (run, rows, surv)
            if run == "no_screen":
                assert surv == f
        for g, w, what in zip(got[run], want, ("pair_ptr", "idx_i", "idx_j")):
            assert np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64)), (name, run, what)
    for run in runs:
        assert all(np.array_equal(a, b) for a, b in zip(got[run], got["default"])), run
    assert len(got["default"][0]) == n_img * (n_img - 1) // 2 + 1
    if name == "solo":
        assert got["default"][0].tolist() == [0] and len(got["default"][1]) == 0
    # the other ratios, with and without the pooled tiles; k = 1 .. 3 (k = 1: never two candidates, no match anywhere)
    for ratio in (0.3, 0.95):
        w = gc.csr_of(gc.pool_chain(name, ratio, 4), n_img, fm.pair_order(n_img))
        for env in ({}, {"APS_MATCH_NO_POOL": "1"}):
            g = _with_env(monkeypatch, env, lambda: fm.match_global_csr(descs, ratio, 4))
            assert all(np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64)) for a, b in zip(g, w)), (name, ratio, env)
    for k in (1, 2, 3):
        w = gc.csr_of(gc.pool_chain(name, 0.6, k), n_img, fm.pair_order(n_img))
        g = fm.match_global_csr(descs, 0.6, k)
        assert all(np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64)) for a, b in zip(g, w)), (name, k)
        if k == 1:
            assert g[0][-1] == 0 and not g[0].any() and len(g[1]) == 0


# ---- the exact-rows repair is really reached ---------------------------------------------------------------------------------
def test_exact_rows_repair_is_reached(fm, capi, monkeypatch, capfd):
    """knn_rows_block_top4_kernel + knn_rows_merge_kernel repair what knn_merge3_kernel / knn_merge_kernel cannot certify;
    the counts the library reports under APS_TRACE prove that the fixtures get there (a count of 0: the fixture is wrong)."""
    pool = gc.pool_knn("crowded", 4)[0]
    monkeypatch.setenv("APS_TRACE", "1")
    capfd.readouterr()
    idx, dist, _ = _screened(capi, pool, gc.CROWDED_SIZES, 0.6, 4)
    err = capfd.readouterr().err
    m = re.search(r"screened pooled k-NN: (\d+) images, (\d+) of (\d+) rows searched, (\d+) recomputed exactly", err)
    assert m, err
    with capfd.disabled():
        print("crowded: recomputed exactly", m.group(4), "searched", m.group(2), "of", m.group(3))
    assert int(m.group(1)) == len(gc.CROWDED_SIZES) and int(m.group(3)) == len(pool) and int(m.group(4)) >= 1
    assert int(m.group(4)) == gc.RECOMPUTED["crowded"] and int(m.group(2)) == gc.SCREEN_SURVIVORS["crowded"][0.6]
    _check_screened_table("crowded", 0.6, 4, idx, dist)
    x = gc.blocked_pool("unit8193").x
    monkeypatch.setenv("APS_KNN_BLOCK", str(gc.BLOCK))
    capfd.readouterr()
    bi, bd = fm.flann_knn_win(x, x, 4)
    err = capfd.readouterr().err
    m = re.search(r"blocked k-NN: (\d+) blocks, (\d+) of (\d+) rows recomputed", err)
    assert m, err
    with capfd.disabled():
        print("unit8193: recomputed", m.group(2), "of", m.group(3), "in", m.group(1), "blocks")
    assert int(m.group(1)) == 17 and int(m.group(3)) == 8193 and int(m.group(2)) >= 1
    assert int(m.group(2)) == gc.RECOMPUTED["unit8193"]
    oi, od = gc.blocked_knn("unit8193")
    assert np.array_equal(bi, oi) and np.array_equal(bits(bd), bits(od))


# ---- blocked aps_knn_global -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [p.name for p in gc.blocked_pools()])
def test_blocked_knn_equals_oracle(fm, monkeypatch, name):
    """The pool against itself (the same array object: the blocked path) at 512-row blocks, screened and all-f32."""
    x = gc.blocked_pool(name).x
    oi, od = gc.blocked_knn(name)
    for k in (1, 2, 3, 4):
        for env in ({"APS_KNN_BLOCK": str(gc.BLOCK)}, {"APS_KNN_BLOCK": str(gc.BLOCK), "APS_KNN_MODE": "f32"}):
            idx, dist = _with_env(monkeypatch, env, lambda: fm.flann_knn_win(x, x, k))
            bad = np.flatnonzero((idx != oi[:, :k]).any(axis=1) | (bits(dist) != bits(od[:, :k])).any(axis=1))
            assert len(bad) == 0, (name, k, env, bad[:8], idx[bad[:4]], oi[bad[:4], :k])


def test_blocked_knn_single_block_and_one_row_second_block(fm, monkeypatch):
    for name in ("unit8192", "unit8195"):  # the default block size: nb == 1
        x = gc.blocked_pool(name).x
        oi, od = gc.blocked_knn(name)
        for k in (2, 4):
            idx, dist = fm.flann_knn_win(x, x, k)
            assert np.array_equal(idx, oi[:, :k]) and np.array_equal(bits(dist), bits(od[:, :k])), (name, k)
    x = gc.blocked_pool("unit8193").x     # two blocks, the second of one row
    oi, od = gc.blocked_knn("unit8193")
    for k in (1, 4):
        idx, dist = _with_env(monkeypatch, {"APS_KNN_BLOCK": "8192"}, lambda: fm.flann_knn_win(x, x, k))
        assert np.array_equal(idx, oi[:, :k]) and np.array_equal(bits(dist), bits(od[:, :k])), k


# ---- layouts on the large paths ----------------------------------------------------------------------------------------------
def _knn_self(capi, x, k, colmajor, ld, ldo, where):
    """aps_knn_global of a pool against itself: one buffer, the same pointer twice."""
    f = len(x)
    tight = ld == (f if colmajor else 128)
    src = place(_flat(x, colmajor) if tight else padded(x, colmajor, ld), where)
    n_out = (k if colmajor else f) * ldo
    idx, dist = place(sentinel_buffer(n_out + 5, np.uint32), where), place(sentinel_buffer(n_out + 5, np.float32), where)
    capi.check(_call(capi, capi.lib.aps_knn_global, capi.ptr(src), f, ld, capi.ptr(src), f, ld, 128,
                     capi.APS_COLMAJOR if colmajor else capi.APS_ROWMAJOR, k, capi.ptr(idx), capi.ptr(dist), ldo))
    if ldo == (f if colmajor else k):  # tight: unpad wants ld > the extent
        shape = (k, f) if colmajor else (f, k)
        i, d = fetch(idx, np.uint32)[:n_out].reshape(shape), fetch(dist)[:n_out].reshape(shape)
        return (np.ascontiguousarray(i.T), np.ascontiguousarray(d.T), True) if colmajor else (i, d, True)
    i, ok_i = unpad(fetch(idx, np.uint32), f, k, colmajor, ldo)
    d, ok_d = unpad(fetch(dist), f, k, colmajor, ldo)
    return i, d, ok_i and ok_d


@pytest.mark.parametrize("where", WHERE)
def test_blocked_knn_column_major_padded(capi, monkeypatch, where):
    """The MATLAB gateway's call (column-major, flann_knn_win(X, X, k): one pointer) on the blocked path."""
    x = gc.blocked_pool("unit8195").x
    f, k = len(x), 4
    oi, od = gc.blocked_knn("unit8195")
    monkeypatch.setenv("APS_KNN_BLOCK", str(gc.BLOCK))
    i0, d0, _ = _knn_self(capi, x, k, False, 128, k, "host")
    ic, dc, intact_c = _knn_self(capi, x, k, True, f + 7, f + 3, where)
    ir, dr, intact_r = _knn_self(capi, x, k, False, 128, k + 3, where)
    assert same_bits(i0, oi) and same_bits(d0, od)
    assert same_bits(ic, i0) and same_bits(dc, d0) and same_bits(ir, i0) and same_bits(dr, d0)
    assert intact_c and intact_r, "elements outside the F x k result were written"


@pytest.mark.parametrize("where", WHERE)
def test_screened_knn_column_major_padded(capi, where):
    pool = gc.pool_knn("mosaic", 4)[0]
    f, k = len(pool), 4
    i0, d0, _ = _screened(capi, pool, gc.MOSAIC_SIZES, 0.6, k)
    _check_screened_table("mosaic", 0.6, k, i0, d0)
    ic, dc, intact_c = _screened(capi, pool, gc.MOSAIC_SIZES, 0.6, k, True, f + 7, f + 3, where)
    ir, dr, intact_r = _screened(capi, pool, gc.MOSAIC_SIZES, 0.6, k, False, 128, k + 3, where)
    assert same_bits(ic, i0) and same_bits(dc, d0) and same_bits(ir, i0) and same_bits(dr, d0)
    assert intact_c and intact_r, "elements outside the F x k result were written"


@pytest.mark.parametrize("where", WHERE)
def test_normalize_column_major_padded(capi, where):
    x = np.concatenate([gc.normalize_rows(), np.concatenate(gc.crowded()[:3])])
    n = len(x)
    want = gc.normalize(x)
    out_r, out_c = place(sentinel_buffer(n * 128 + 7, np.float32), where), place(sentinel_buffer(n * 128 + 7, np.float32), where)
    x_r, x_c = place(_flat(x, False), where), place(padded(x, True, n + 5), where)
    capi.check(_call(capi, capi.lib.aps_global_normalize, capi.ptr(x_r), n, 128, 128, capi.APS_ROWMAJOR, capi.ptr(out_r)))
    capi.check(_call(capi, capi.lib.aps_global_normalize, capi.ptr(x_c), n, n + 5, 128, capi.APS_COLMAJOR, capi.ptr(out_c)))
    for out in (out_r, out_c):
        o = fetch(out)
        assert same_bits(o[:n * 128].reshape(n, 128), want)
        assert same_bits(o[n * 128:], sentinel_buffer(7, np.float32))


def _filter(capi, case, colmajor=False, ldn=None, where="host", cap=None):
    """aps_global_filter -> (pair_ptr, idx_i, idx_j, outputs beyond the count intact)."""
    f, k = case.nn_idx.shape
    ldn = ldn or (f if colmajor else k)
    tight = ldn == (f if colmajor else k)
    lay = lambda a: _flat(a, colmajor) if tight else padded(a, colmajor, ldn)  # noqa: E731
    ni, nd = place(lay(case.nn_idx), where), place(lay(case.nn_dist), where)
    img, loc = place(np.array(case.img_idx), where), place(np.array(case.local_idx), where)
    cap = f + 9 if cap is None else cap
    n_pairs = case.n_img * (case.n_img - 1) // 2
    pp = np.full(n_pairs + 1, -7, np.int64)
    oi, oj = place(sentinel_buffer(max(cap, 1), np.uint32), where), place(sentinel_buffer(max(cap, 1), np.uint32), where)
    cnt = C.c_int64(-1)
    capi.check(_call(capi, capi.lib.aps_global_filter, capi.ptr(ni), capi.ptr(nd), f, k, ldn, capi.APS_COLMAJOR if colmajor else capi.APS_ROWMAJOR,
                     capi.ptr(img), capi.ptr(loc), case.n_img, float(case.ratio), capi.ptr(pp), capi.ptr(oi), capi.ptr(oj), cap, C.byref(cnt)))
    n = cnt.value
    hi, hj = fetch(oi, np.uint32), fetch(oj, np.uint32)
    sent = sentinel_buffer(1, np.uint32)[0]
    return pp, hi[:n].copy(), hj[:n].copy(), bool(np.all(hi[n:] == sent) and np.all(hj[n:] == sent))


def _filter_want(fm, case):
    rows = oracle.global_filter(case.nn_idx, case.nn_dist, case.img_idx, case.local_idx, case.ratio)
    return gc.csr_of(rows, case.n_img, fm.pair_order(case.n_img))


@pytest.mark.parametrize("where", WHERE)
def test_filter_column_major_padded(fm, capi, where):
    cases = {c.name: c for c in gc.filter_tables()}
    _, ni, nd, img, loc = gc.pool_knn("mosaic", 4)
    big = gc.FilterCase("mosaic", ni, nd, img, loc, len(gc.MOSAIC_SIZES), 0.6, 4)
    for case in (cases["images40"], cases["holes_and_self"], cases["k7"], big):
        f = len(case.img_idx)
        want = _filter_want(fm, case)
        for got in (_filter(capi, case), _filter(capi, case, True, f + 3, where), _filter(capi, case, False, case.k + 3, where)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), case.name
            assert got[3], "elements beyond the match count were written"


# ---- aps_global_filter, direct ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in gc.filter_tables()])
def test_filter_tables_equal_oracle(fm, gpu, capi, name):
    case = next(c for c in gc.filter_tables() if c.name == name)
    want = _filter_want(fm, case)
    pp, oi, oj, intact = _filter(capi, case)
    assert np.array_equal(pp, want[0]), name
    assert np.array_equal(oi, want[1]) and np.array_equal(oj, want[2]) and intact, name
    total = int(want[0][-1])
    if total > 0:  # an exact capacity is enough, one less is an error
        pp, oi, oj, _ = _filter(capi, case, cap=total)
        assert np.array_equal(pp, want[0]) and np.array_equal(oi, want[1]) and np.array_equal(oj, want[2])
        with pytest.raises(gpu.ApsError):
            _filter(capi, case, cap=total - 1)


# ---- aps_global_normalize, direct ------------------------------------------------------------------------------------------
def test_normalize_equals_numpy_chain(capi):
    x = gc.normalize_rows()
    out = np.zeros_like(x)
    capi.check(capi.lib.aps_global_normalize(capi.ptr(x), len(x), 128, 128, capi.APS_ROWMAJOR, capi.ptr(out)))
    want = gc.normalize(x)
    assert not np.isnan(want).any()
    bad = np.flatnonzero((bits(out) != bits(want)).any(axis=1))
    assert len(bad) == 0, (bad, out[bad[:2], :4], want[bad[:2], :4])


# ---- knn_f32_kernel<4|8> sweep ----------------------------------------------------------------------------------------------
KNN_FT = (1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 193)


@pytest.mark.parametrize("fq", [1, 127, 128, 129, 257])
def test_knn_f32_sweep(fm, fq):
    """Train counts around the 64-row train tile against query counts around the 128-row query tile, every k in 1..8
    (k <= 4: knn_f32_kernel<4>, above: <8>); distinct train and query arrays; slots beyond ft: index 0 / inf."""
    for ft in KNN_FT:
        rng = np.random.default_rng(1000 * fq + ft)
        train, query = sift_like(rng, ft), sift_like(rng, fq)
        if ft >= 2:
            train[ft // 2] = train[0]              # an exact duplicate pair: ties resolve to the lower index
        v = np.maximum(train[ft - 1] + np.float32(1e-3) * rng.standard_normal(128).astype(np.float32), 0)
        query[fq // 2] = (v / np.linalg.norm(v)).astype(np.float32)   # the last train row is somebody's nearest neighbour
        if fq > 2:
            query[fq - 1] = train[0]               # an exact hit on the duplicated row
        o8i, o8d = oracle.knn(train, query, 8)
        if ft != 2:
            assert o8i[fq // 2, 0] == ft
        for k in range(1, 9):
            idx, dist = fm.flann_knn_win(train, query, k)
            oi, od = oracle.knn(train, query, k)
            assert np.array_equal(oi, o8i[:, :k])
            assert np.array_equal(idx, oi) and np.array_equal(bits(dist), bits(od)), (ft, fq, k)
            if k > ft:
                assert np.all(idx[:, ft:] == 0) and np.all(np.isinf(dist[:, ft:])) and np.all(idx[:, :ft] > 0)


# ---- hamming_knn_kernel<NW, K>: all six instantiations ------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [1, 4, 31, 32, 33, 64])
def test_hamming_knn_every_instantiation(fm, nbytes):
    """nbytes <= 32: NW = 8, above: 16; k <= 2, <= 4, <= 8: K = 2, 4, 8.  Train counts around the 256-row LDS tile."""
    for nt in (3, 255, 256, 257, 513):
        rng = np.random.default_rng(100 * nbytes + nt)
        train = rng.integers(0, 256, (nt, nbytes), dtype=np.uint8)
        query = rng.integers(0, 256, (300, nbytes), dtype=np.uint8)
        train[nt - 1] = train[0]                               # duplicated train rows, the last row among them
        train[nt // 2] = train[1]
        query[:100] = train[rng.integers(0, nt, 100)]          # queries copied from the train set: distance 0, ties
        query[299] = train[nt - 1]
        for k in (1, 2, 3, 4, 5, 8):
            idx, dist = fm.flann_knn_win(train, query, k)
            oi, od = oracle.knn_hamming(train, query, k)
            assert np.array_equal(idx, oi) and np.array_equal(bits(dist), bits(od)), (nbytes, nt, k)
            assert np.all(dist[:100, 0] == 0)
