"""The 1024-row workgroups of the int8 stream kernels (APS_SCREEN_ROWS=1024, the default: 128 A rows per wave) against the
512-row form (APS_SCREEN_ROWS=512), the all-f32 kernel (APS_MATCH_MODE=f32) and the CPU oracle, bit for bit, at the row and
column counts where the new tiling can go wrong: around one wave (127..129), around the 512-row remainder rule (511..513),
around one and two wide workgroups (1023..1025, 1537, 2049); column counts around one B tile (255..257), two tiles (513)
and 2049 + 256 * 8 = 4097 (17 tiles: crosses a kSeg = 8 segment boundary, ragged last tile), and 2.

Descriptors are integer codes 0 .. 255, matched in normalised form (over their f32 norm: the exact integer path); one column
set carries a single non-integer entry, so its jobs take the rounded codes.

What the library exposes of the screen is the match lists (row, column, metric = d1; d2 enters through the ratio test, and
with Unique = False every row that passes is listed), the survivor COUNT of a call (aps_match_screen_stats), the number of
jobs on exact codes (aps_match_screen_exact_jobs) and, under APS_TRACE, the workgroup counts of a screening pass.  A row's
verdict depends on that row and the column set only, so equal counts per single-pair call at every shape, together with
equal lists, is the survivor identity checked here."""
import ctypes
import re
from importlib import import_module

import numpy as np
import pytest

import oracle
from util import bits, sift_like

pytestmark = pytest.mark.gpu

N_A = (1, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1537, 2049)
N_B = (2, 255, 256, 257, 513, 2049 + 256 * 8)
FILTERS = ((0.6, 3.5, True), (0.8, 1.5, False))  # (MaxRatio, MatchThreshold in percent, Unique)
SWITCHES = ("APS_SCREEN_ROWS", "APS_LIST_ROWS", "APS_MATCH_MODE", "APS_TRACE")


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def _codes(x):
    return np.round(x * 512).clip(0, 255).astype(np.float32)


@pytest.fixture(scope="module")
def sets():
    """A (2049 rows) and B (4097 columns) as integer codes; the cases are their leading rows.  Half of the A rows are noisy
    copies of a column - the partner's position is drawn so that every column count keeps some: a quarter among the first 255,
    a quarter among the first two - with noise levels on both sides of the ratio test.  Br: B with one non-integer entry."""
    rng = np.random.default_rng(1024)
    na, nb = max(N_A), max(N_B)
    a = sift_like(rng, na)
    b = sift_like(rng, nb)
    rows = rng.permutation(na)[: na // 2]
    reach = rng.choice([2, 255, nb, nb], size=len(rows))
    cols = (rng.random(len(rows)) * reach).astype(np.int64)
    noise = rng.uniform(0.0, 0.12, len(rows))[:, None].astype(np.float32)
    pert = np.maximum(b[cols] + noise * rng.standard_normal((len(rows), 128)).astype(np.float32), 0)
    a[rows] = pert / (np.linalg.norm(pert, axis=1, keepdims=True) + 1e-12)
    a[0] = b[1]  # (the one-row set has a match in the two-column set)
    A, B = _codes(a), _codes(b)
    assert A.max() > 2 and np.array_equal(A, np.rint(A)) and np.array_equal(B, np.rint(B))
    Br = B.copy()
    Br[1, 5] += np.float32(0.5)
    return {"A": A, "B": B, "Br": Br, "oracle": {}}


def _oracle(sets, which, na, nb, flt):
    key = (which, na, nb, flt)
    if key not in sets["oracle"]:
        m, met = oracle.match_features(sets["A"][:na], sets[which][:nb], flt[0], flt[1], flt[2], 2)
        sets["oracle"][key] = (np.asarray(m, np.int64).reshape(-1, 2), bits(met))
    return sets["oracle"][key]


def _clean(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


def _stats(gpu):
    rows, surv, jobs, ex = (ctypes.c_int64(-1) for _ in range(4))
    gpu._capi.check(gpu.lib.aps_match_screen_stats(ctypes.byref(rows), ctypes.byref(surv)))
    gpu._capi.check(gpu.lib.aps_match_screen_exact_jobs(ctypes.byref(jobs), ctypes.byref(ex)))
    return rows.value, surv.value, jobs.value, ex.value


def _all_pairs(sets, which):
    descs = [sets["A"][:n] for n in N_A] + [sets[which][:n] for n in N_B]
    pairs = [(i, len(N_A) + j) for i in range(len(N_A)) for j in range(len(N_B))]
    return descs, pairs


@pytest.mark.parametrize("which", ["B", "Br"])
@pytest.mark.parametrize("flt", FILTERS)
def test_every_shape_equals_512_rows_f32_and_oracle(fm, gpu, monkeypatch, sets, which, flt):
    """All 72 (nA, nB) jobs in one aps_match_pairs call - the survivors of the twelve row sets that share a column set are
    pooled into common list tiles, with APS_LIST_ROWS=1024 cut like the screen's - under the 1024-row screen, the same with
    the 1024-row list pass, the 512-row form and the all-f32 kernel: the same lists, and pair by pair the oracle's."""
    descs, pairs = _all_pairs(sets, which)
    got = {}
    for mode, env in (("1024", {}), ("1024+list", {"APS_LIST_ROWS": "1024"}), ("512", {"APS_SCREEN_ROWS": "512"}),
                      ("f32", {"APS_MATCH_MODE": "f32"})):
        _clean(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got[mode] = fm.match_pairs_csr(descs, pairs, flt[0], flt[1], flt[2])
        if mode != "f32":
            rows, surv, jobs, ex = _stats(gpu)
            got[mode + "_stats"] = (rows, surv, jobs, ex)
    _clean(monkeypatch)
    pp, ia, ib, met = got["1024"]
    for other in ("1024+list", "512", "f32"):
        qp, qa, qb, qm = got[other]
        assert np.array_equal(pp, qp) and np.array_equal(ia, qa) and np.array_equal(ib, qb), other
        assert np.array_equal(bits(met), bits(qm)), other
    assert got["1024_stats"] == got["512_stats"] == got["1024+list_stats"]
    rows, surv, jobs, ex = got["1024_stats"]
    assert rows == len(N_B) * sum(N_A) and jobs == len(pairs)
    # exact-job coverage: every job of two integer sets; none against the set with a non-integer entry
    assert ex == (len(pairs) if which == "B" else 0)
    # the pooled list pass has wide tiles to cut: more than 1024 survivors against the largest column set alone
    assert surv > 1024
    total = 0
    for p, (i, j) in enumerate(pairs):
        om, omet = _oracle(sets, which, N_A[i], N_B[j - len(N_A)], flt)
        s, e = pp[p], pp[p + 1]
        assert np.array_equal(np.stack([ia[s:e], ib[s:e]], 1).astype(np.int64), om), (N_A[i], N_B[j - len(N_A)])
        assert np.array_equal(bits(met[s:e]), omet), (N_A[i], N_B[j - len(N_A)])
        total += len(om)
    assert total > 2000  # (the planted matches are found: the comparison is not one of empty lists)


def test_survivor_counts_per_job_equal_the_512_row_form(fm, gpu, monkeypatch, sets):
    """One call per shape: rows, survivors and the exact-code verdict of the job under both forms, and its list against the
    oracle.  The job with 2049 rows against 4097 columns leaves more than 1024 survivors: its list pass runs 1024-row tiles."""
    flt = FILTERS[1]
    most = 0
    for na in N_A:
        for nb in N_B:
            a, b = sets["A"][:na], sets["B"][:nb]
            seen = []
            for env in (None, "512"):
                _clean(monkeypatch)
                if env:
                    monkeypatch.setenv("APS_SCREEN_ROWS", env)
                else:
                    monkeypatch.setenv("APS_LIST_ROWS", "1024")
                pp, ia, ib, met = fm.match_pairs_csr([a, b], [(0, 1)], flt[0], flt[1], flt[2])
                seen.append(_stats(gpu))
                om, omet = _oracle(sets, "B", na, nb, flt)
                assert np.array_equal(np.stack([ia, ib], 1).astype(np.int64), om) and np.array_equal(bits(met), omet), (na, nb, env)
            assert seen[0] == seen[1], (na, nb, seen)
            assert seen[0][0] == na and seen[0][2:] == (1, 1), (na, nb, seen)
            most = max(most, seen[0][1])
    _clean(monkeypatch)
    assert most > 1024


def test_exact_codes_where_due(fm, gpu, monkeypatch, sets):
    """Two column sets in one call, one of integer codes and one with a non-integer entry: the first job takes the exact
    codes, the second the rounded ones, under both forms."""
    a = sets["A"][:1025]
    for env in (None, "512"):
        _clean(monkeypatch)
        if env:
            monkeypatch.setenv("APS_SCREEN_ROWS", env)
        pp, ia, ib, met = fm.match_pairs_csr([a, sets["B"][:513], sets["Br"][:513]], [(0, 1), (0, 2)], 0.6, 3.5, True)
        assert _stats(gpu)[2:] == (2, 1)
        for p, which in enumerate(("B", "Br")):
            om, omet = _oracle(sets, which, 1025, 513, FILTERS[0])
            s, e = pp[p], pp[p + 1]
            assert np.array_equal(np.stack([ia[s:e], ib[s:e]], 1).astype(np.int64), om) and np.array_equal(bits(met[s:e]), omet)
    _clean(monkeypatch)


@pytest.mark.parametrize("rows,na,wide,narrow", [
    ("1024", 1, 0, 1), ("1024", 512, 0, 1), ("1024", 513, 1, 0), ("1024", 1024, 1, 0), ("1024", 1025, 1, 1),
    ("1024", 1536, 1, 1), ("1024", 1537, 2, 0), ("1024", 2049, 2, 1), ("512", 1025, 0, 3), ("512", 2049, 0, 5)])
def test_remainder_routing(fm, monkeypatch, capfd, sets, rows, na, wide, narrow):
    """A job's rows are cut into 1024-row workgroups; a remainder of up to 512 rows takes one 512-row workgroup, a larger
    one a ragged wide workgroup: 1025 rows = 1 + 1.  Read from the workgroup counts the library reports under APS_TRACE."""
    _clean(monkeypatch)
    monkeypatch.setenv("APS_SCREEN_ROWS", rows)
    monkeypatch.setenv("APS_TRACE", "1")
    capfd.readouterr()
    pp, ia, ib, met = fm.match_pairs_csr([sets["A"][:na], sets["B"][:257]], [(0, 1)], 0.6, 3.5, True)
    err = capfd.readouterr().err
    _clean(monkeypatch)
    m = re.search(r"int8 screen workgroups: (\d+) of 1024 rows, (\d+) of 512 rows", err)
    assert m, err
    assert (int(m.group(1)), int(m.group(2))) == (wide, narrow), err
    if na in N_A:
        om, omet = _oracle(sets, "B", na, 257, FILTERS[0])
        assert np.array_equal(np.stack([ia, ib], 1).astype(np.int64), om) and np.array_equal(bits(met), omet)


def test_pooled_matcher_bounds_pass(fm, gpu, monkeypatch, capfd):
    """aps_knn_global_screened, k = 4, on three small images - 5121, 2561 and 512 rows: five wide workgroups with a one-row
    remainder, two with a ragged third, a single narrow one; 8194 rows in all, just past the small-pool shortcut that skips
    the screen: the CSR lists of the 1024-row bounds pass equal those of the 512-row form and of the plain exact search
    (APS_KNN_MODE=f32), with the same number of dismissed rows."""
    rng = np.random.default_rng(4)
    base = sift_like(rng, 6000)
    descs = []
    for n in (5121, 2561, 512):
        keep = rng.permutation(6000)[:n]
        noise = rng.uniform(0.0, 0.1, n)[:, None]
        d = np.maximum(base[keep] + noise * rng.standard_normal((n, 128)).astype(np.float32), 0)
        descs.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))

    def share():
        rows, surv = ctypes.c_int64(-1), ctypes.c_int64(-1)
        gpu._capi.check(gpu.lib.aps_knn_global_screen_stats(ctypes.byref(rows), ctypes.byref(surv)))
        return rows.value, surv.value

    _clean(monkeypatch)
    monkeypatch.delenv("APS_KNN_MODE", raising=False)
    monkeypatch.setenv("APS_TRACE", "1")
    capfd.readouterr()
    wide = fm.match_global_csr(descs, 0.6, 4)
    err = capfd.readouterr().err
    s_wide = share()
    monkeypatch.delenv("APS_TRACE")
    monkeypatch.setenv("APS_SCREEN_ROWS", "512")
    narrow = fm.match_global_csr(descs, 0.6, 4)
    s_narrow = share()
    monkeypatch.delenv("APS_SCREEN_ROWS")
    monkeypatch.setenv("APS_KNN_MODE", "f32")
    plain = fm.match_global_csr(descs, 0.6, 4)
    monkeypatch.delenv("APS_KNN_MODE")
    for other in (narrow, plain):
        for x, y in zip(wide, other):
            assert np.array_equal(x, y)
    assert wide[0][-1] > 200
    assert s_wide == s_narrow and 0 < s_wide[1] < s_wide[0]
    # two jobs per query image: 5121 rows = 5 + 1, 2561 rows = 3 + 0, 512 rows = 0 + 1
    found = re.findall(r"int8 screen workgroups: (\d+) of 1024 rows, (\d+) of 512 rows", err)
    assert found and (sum(int(w) for w, _ in found), sum(int(n) for _, n in found)) == (16, 4), err
