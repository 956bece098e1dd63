"""The batched Hamming matcher (aps_hamming_match_pairs / _pairwise, fm.match_pairs_binary_csr) against two expectations:
a NumPy restatement (tests/hamming_pairs_cases.py: brute-force XOR / popcount 2-NN with the mex's tie rule, then the package's
host filter) and the per-pair matchFeaturesScratch it replaces.  Equal means every offset, index and metric bit, in order.

Per-image counts straddle the kernel's boundaries (0, 1, 2; 127 / 128 / 129 around the B tile; 255 / 256 / 257 around the row
block; 300), so the all-pairs list meets each of them on the A side and on the B side."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import fast_cases as fc
import hamming_pairs_cases as hc

RULES = ((0.6, 12.5, True), (0.8, 20.0, False))
PLANTED_RULES = ((0.5, 12.5, True), (1.0, 100.0, True), (0.5, 12.5, False), (0.6, 20.0, True))


def fmod(aps):
    return import_module(aps.__name__ + ".featureMatching")


def pair_order(n):
    return [(i, j) for j in range(1, n) for i in range(j)]   # featureMatchingPairwise.m:48


# ---- device-free: the comparison is not empty, and the planted rows decide what they were planted for -------------------
def test_restatement_alone_yields_matches_for_every_non_degenerate_pair(aps):
    fm = fmod(aps)
    for name, sets, nbits, counts in (("s64", hc.sets_64(), 512, hc.COUNTS_64), ("s32", hc.sets_32(), 256, hc.COUNTS_32),
                                      ("odd", [hc.pack(b) for b in hc.sets_odd_bits()], hc.NBITS_ODD, hc.COUNTS_BITS)):
        pairs = pair_order(len(sets))
        for rule in RULES:
            p, _, _, _ = hc.expected_csr(fm, name, sets, nbits, pairs, *rule)
            for k, (i, j) in enumerate(pairs):
                if min(counts[i], counts[j]) >= 100:   # both sets hold the 100 shared world rows
                    assert p[k + 1] - p[k] >= 50, (name, rule, i, j, int(p[k + 1] - p[k]))


def test_planted_rows_decide_as_planted(aps):
    fm = fmod(aps)
    A, B, rows = hc.planted()
    A, B = hc.pack(A), hc.pack(B)
    D = hc.hamming(A, B)
    r = rows
    assert D[r["best_tie"], 0] == D[r["best_tie"], 1] == 10 and D[r["zero_second"], 0] == D[r["zero_second"], 1] == 0
    assert D[r["column_tie_lo"], 2] == D[r["column_tie_hi"], 2] == 20
    assert sorted(D[r["on_threshold"]])[0] == 64 and sorted(D[r["on_ratio"]])[:2] == [64, 128]
    assert sorted(D[r["beyond_threshold"]])[0] == 65 and sorted(D[r["beyond_ratio"]])[:2] == [63, 125]
    m, d = hc.match(fm, A, B, 512, 0.5, 12.5, True)
    kept = {int(a) - 1: int(b) for a, b in m}
    assert r["best_tie"] not in kept                       # d1 == d2 fails a ratio of 0.5
    assert kept[r["zero_second"]] == 1                     # the second of 0 was patched: kept, and on the lower of the equal columns
    assert kept[r["column_tie_lo"]] == 3 and r["column_tie_hi"] not in kept
    assert kept[r["on_threshold"]] == 4 and kept[r["on_ratio"]] == 5
    assert r["beyond_threshold"] not in kept and r["beyond_ratio"] not in kept
    assert d[[int(a) - 1 for a in m[:, 0]].index(r["on_ratio"])] == np.float32(12.5)
    m1, _ = hc.match(fm, A, B, 512, 1.0, 100.0, True)      # ratio 1: the tie row passes the filter and loses column 1 to the zero row
    kept1 = {int(a) - 1: int(b) for a, b in m1}
    assert r["best_tie"] not in kept1 and kept1[r["zero_second"]] == 1 and r["beyond_threshold"] in kept1 and r["beyond_ratio"] in kept1
    m0, _ = hc.match(fm, A, B, 512, 1.0, 100.0, False)
    assert m0[r["best_tie"]].tolist() == [r["best_tie"] + 1, 1] and len(m0) == len(A)


# ---- device ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fm(gpu):
    return fmod(gpu)


@pytest.fixture(scope="module")
def descs_64(fm):
    return [fm.binaryFeatures(s) for s in hc.sets_64()]


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
def test_all_pairs_of_64_byte_sets_equal_both_expectations(fm, descs_64, rule):
    pairs = pair_order(len(descs_64))
    got = fm.match_pairwise_binary_csr(descs_64, *rule)
    assert got[1].dtype == np.uint32 and got[2].dtype == np.uint32 and got[0].dtype == np.int64 and len(got[1]) > 1000
    assert hc.same_csr(got, hc.expected_csr(fm, "s64", hc.sets_64(), 512, pairs, *rule))
    assert hc.same_csr(got, hc.per_pair_csr(fm, descs_64, pairs, *rule))
    assert hc.same_csr(fm.match_pairs_binary_csr(descs_64, pairs, *rule), got)   # the explicit list of the same pairs


@pytest.mark.gpu
def test_explicit_pair_list_in_both_orientations_with_a_repeated_pair(fm, descs_64):
    pairs = [(9, 6), (6, 9), (9, 6), (1, 8), (8, 1), (0, 9), (9, 0), (2, 5), (5, 2), (7, 3), (3, 7), (4, 8)]
    for rule in RULES:
        got = fm.match_pairs_binary_csr(descs_64, pairs, *rule)
        assert hc.same_csr(got, hc.expected_csr(fm, "s64", hc.sets_64(), 512, pairs, *rule))
        assert hc.same_csr(got, hc.per_pair_csr(fm, descs_64, pairs, *rule))
        assert hc.same_csr(fm.match_pairs_binary_csr(descs_64, np.asarray(pairs, np.int32), *rule), got)
    p = got[0]
    assert p[1] - p[0] == p[3] - p[2] > 50 and np.array_equal(got[1][p[0]:p[1]], got[1][p[2]:p[3]])


@pytest.mark.gpu
def test_32_byte_sets_and_a_bit_width_that_is_no_multiple_of_8(fm):
    sets = hc.sets_32()
    descs = [fm.binaryFeatures(s) for s in sets]
    pairs = pair_order(len(sets)) + [(4, 2), (3, 1)]
    for rule in RULES:
        got = fm.match_pairs_binary_csr(descs, pairs, *rule)
        assert len(got[1]) > 200
        assert hc.same_csr(got, hc.expected_csr(fm, "s32", sets, 256, pairs, *rule))
        assert hc.same_csr(got, hc.per_pair_csr(fm, descs, pairs, *rule))
    bits = hc.sets_odd_bits()   # unpacked 250-bit rows: packBits pads them to 32 bytes, the percent values divide by 250
    packed = [hc.pack(b) for b in bits]
    pairs = pair_order(len(bits)) + [(3, 0), (2, 1)]
    for rule in RULES:
        got = fm.match_pairs_binary_csr(bits, pairs, *rule)
        assert len(got[1]) > 200
        assert hc.same_csr(got, hc.expected_csr(fm, "odd", packed, hc.NBITS_ODD, pairs, *rule))
        assert hc.same_csr(got, hc.per_pair_csr(fm, bits, pairs, *rule))


@pytest.mark.gpu
@pytest.mark.parametrize("rule", PLANTED_RULES)
def test_planted_rows_for_every_decision(fm, rule):
    A, B, _ = hc.planted()
    sets = [hc.pack(A), hc.pack(B)]
    descs = [fm.binaryFeatures(s) for s in sets]
    pairs = [(0, 1), (1, 0)]
    got = fm.match_pairs_binary_csr(descs, pairs, *rule)
    assert hc.same_csr(got, hc.expected_csr(fm, "planted", sets, 512, pairs, *rule))
    assert hc.same_csr(got, hc.per_pair_csr(fm, descs, pairs, *rule))


def _c_call(capi, ptrs, counts, lds, nbytes, layout, pa, pb, rule, pair_ptr, ia, ib, met, cap, pairwise=False, nbits=0):
    n = len(counts)
    tbl = (C.c_void_p * n)(*ptrs)
    o = capi.aps_hamming_match_opts(rule[0], rule[1], 1 if rule[2] else 0, nbits)
    cnt = C.c_int64(-1)
    P = lambda x: capi.ptr(x) if x is not None else None   # noqa: E731
    if pairwise:
        rc = capi.lib.aps_hamming_match_pairwise(tbl, (C.c_int64 * n)(*counts), (C.c_int64 * n)(*lds), n, nbytes, layout, C.byref(o), P(pair_ptr),
                                                 P(ia), P(ib), P(met), cap, C.byref(cnt))
    else:
        rc = capi.lib.aps_hamming_match_pairs(tbl, (C.c_int64 * n)(*counts), (C.c_int64 * n)(*lds), n, nbytes, layout, P(pa), P(pb), len(pa),
                                              C.byref(o), P(pair_ptr), P(ia), P(ib), P(met), cap, C.byref(cnt))
    return rc, cnt.value


@pytest.mark.gpu
def test_c_abi_layouts_pointers_capacity_and_count_only(gpu, fm):
    """Column-major and padded sets on host and on device pointers; padding and the capacity tail stay the caller's; a small
    cap and the count-only forms report APS_E_CAP with the true count and the offsets; device-side pair lists and outputs."""
    import torch

    capi = gpu._capi
    rule = RULES[0]
    sets = [hc.sets_64()[k] for k in (9, 5, 1, 0, 8)]   # 300, 129, 1, 0, 257 rows
    counts = [len(s) for s in sets]
    pairs = [(0, 1), (1, 0), (4, 0), (2, 4), (3, 0), (0, 4)]
    pa, pb = np.asarray([p[0] for p in pairs], np.int32), np.asarray([p[1] for p in pairs], np.int32)
    want = hc.expected_csr(fm, "s64", hc.sets_64(), 512, [((9, 5, 1, 0, 8)[a], (9, 5, 1, 0, 8)[b]) for a, b in pairs], *rule)
    total = int(want[0][-1])
    assert total > 300
    cap = total + 7

    def padded(layout, dev):
        out, lds = [], []
        for s in sets:
            n = len(s)
            if layout == capi.APS_ROWMAJOR:
                buf = np.full((max(n, 1), 64 + 5), 0xA5, np.uint8)
                buf[:n, :64] = s
                lds.append(64 + 5)
            else:
                buf = np.full((64, n + 3), 0xA5, np.uint8)   # column k at buf[k, :n]: element (i, k) at i + k * (n + 3)
                buf[:, :n] = s.T
                lds.append(n + 3)
            out.append(torch.from_numpy(buf).cuda() if dev else buf)
        return out, lds

    for layout in (capi.APS_ROWMAJOR, capi.APS_COLMAJOR):
        for dev in (False, True):
            bufs, lds = padded(layout, dev)
            before = [b.clone() if dev else b.copy() for b in bufs]
            if dev:
                ia, ib = torch.full((cap,), 77, dtype=torch.int32, device="cuda"), torch.full((cap,), 77, dtype=torch.int32, device="cuda")
                met, pp = torch.full((cap,), -3.0, dtype=torch.float32, device="cuda"), torch.full((len(pairs) + 2,), -9, dtype=torch.int64, device="cuda")
                dpa, dpb = torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()
                torch.cuda.synchronize()
            else:
                ia, ib, met, pp = np.full(cap, 77, np.uint32), np.full(cap, 77, np.uint32), np.full(cap, -3.0, np.float32), np.full(len(pairs) + 2, -9, np.int64)
                dpa, dpb = pa, pb
            rc, cnt = _c_call(capi, [capi.ptr(b) if n else None for b, n in zip(bufs, counts)], counts, lds, 64, layout, dpa, dpb, rule, pp, ia, ib, met, cap)
            assert rc == capi.APS_OK and cnt == total, (layout, dev, capi.lib.aps_last_error())
            host = lambda x: x.cpu().numpy() if dev else x   # noqa: E731
            ia, ib, met, pp = host(ia), host(ib), host(met), host(pp)
            assert hc.same_csr((pp[:len(pairs) + 1], ia[:total], ib[:total], met[:total]), want), (layout, dev)
            assert pp[-1] == -9 and (ia[total:] == 77).all() and (ib[total:] == 77).all() and (met[total:] == -3.0).all()
            for b, b0 in zip(bufs, before):   # the sets, padding included, are the caller's
                assert bool((b == b0).all())
    # capacity: one short, zero, and no lists at all - the true count and the offsets, nothing written
    bufs, lds = padded(capi.APS_ROWMAJOR, False)
    ptrs = [capi.ptr(b) if n else None for b, n in zip(bufs, counts)]
    for (cap_k, lists) in ((total - 1, True), (0, True), (cap, False)):
        ia, ib, met, pp = np.full(cap, 77, np.uint32), np.full(cap, 77, np.uint32), np.full(cap, -3.0, np.float32), np.zeros(len(pairs) + 1, np.int64)
        rc, cnt = _c_call(capi, ptrs, counts, lds, 64, capi.APS_ROWMAJOR, pa, pb, rule, pp, *((ia, ib, met) if lists else (None, None, None)), cap_k)
        assert rc == capi.APS_E_CAP and cnt == total and np.array_equal(pp, want[0])
        assert (ia == 77).all() and (ib == 77).all() and (met == -3.0).all()
    # the all-pairs entry on the same tables
    want_all = hc.expected_csr(fm, "s64", hc.sets_64(), 512, [((9, 5, 1, 0, 8)[a], (9, 5, 1, 0, 8)[b]) for a, b in pair_order(5)], *rule)
    t_all = int(want_all[0][-1])
    ia, ib, met, pp = np.zeros(t_all, np.uint32), np.zeros(t_all, np.uint32), np.zeros(t_all, np.float32), np.zeros(11, np.int64)
    rc, cnt = _c_call(capi, ptrs, counts, lds, 64, capi.APS_ROWMAJOR, None, None, rule, pp, ia, ib, met, t_all, pairwise=True)
    assert rc == capi.APS_OK and cnt == t_all and hc.same_csr((pp, ia, ib, met), want_all)


@pytest.mark.gpu
def test_chunked_walk_gives_the_same_lists(fm, descs_64):
    """max_columns below one pair's columns (every pair a chunk of its own), and one that splits the list in the middle."""
    pairs = pair_order(len(descs_64)) + [(9, 8), (8, 9)]
    for rule in RULES:
        whole = fm.match_pairs_binary_csr(descs_64, pairs, *rule)
        for bound in (1, 700, 2000):
            assert hc.same_csr(fm.match_pairs_binary_csr(descs_64, pairs, *rule, max_columns=bound), whole), (rule, bound)


@pytest.mark.gpu
def test_device_out_with_resident_sets_equals_the_host_result(fm, descs_64):
    import torch

    resident = [fm.binaryFeatures(torch.from_numpy(d.Features).cuda()) for d in descs_64]
    torch.cuda.synchronize()
    pairs = pair_order(len(descs_64))
    for rule in RULES:
        host = fm.match_pairs_binary_csr(descs_64, pairs, *rule)
        p, ia, ib, met = fm.match_pairs_binary_csr(resident, pairs, *rule, device_out=True)
        assert all(torch.is_tensor(x) and x.is_cuda for x in (ia, ib, met)) and isinstance(p, np.ndarray)
        assert ia.dtype == torch.int32 and ib.dtype == torch.int32 and met.dtype == torch.float32
        assert hc.same_csr((p, ia.cpu().numpy(), ib.cpu().numpy(), met.cpu().numpy()), host)
        assert hc.same_csr(fm.match_pairs_binary_csr(resident, pairs, *rule), host)   # resident sets, host lists
    p, ia, ib, met = fm.match_pairs_binary_csr(resident, [(0, 1), (1, 0)], *RULES[0], device_out=True)   # set 0 is empty
    assert p.tolist() == [0, 0, 0] and all(torch.is_tensor(x) and x.is_cuda and x.numel() == 0 for x in (ia, ib, met))


@pytest.mark.gpu
def test_fast_descriptors_of_three_views_equal_the_per_pair_loop(fm):
    inp = {"detector": "FAST", "MinContrast": 0.08}
    descs = [fm.getFeaturePoints(inp, v)[0] for v in fc.scene()[0]]   # three 240 x 320 views, 227 / 220 / 220 features
    got = fm.match_pairwise_binary_csr(descs, 0.6, 20.0, True)
    assert np.diff(got[0]).tolist() == [80, 44, 82]
    assert hc.same_csr(got, hc.per_pair_csr(fm, descs, pair_order(3), 0.6, 20.0, True))
    cells = fm.featureMatchingPairwise({"Matchingthreshold": 20.0, "Ratiothreshold": 0.6}, descs, 3)
    assert np.array_equal(cells[0][2], np.stack([got[1][80:124], got[2][80:124]], 1).astype(np.float64))
