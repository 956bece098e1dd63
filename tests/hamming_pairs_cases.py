"""Seeded binary descriptor sets and the NumPy restatement shared by the batched Hamming matcher's tests (helper, not a test).

Random bytes never pass a 0.6 ratio, so every set is built from one `world` of random rows: a set of n rows holds noisy copies
(0 .. 20 flipped bits of the row's width) of the world's first min(n, 100) rows at shuffled positions, and random rows for the
rest.  Any two sets of 100 rows or more therefore share 100 world rows, whose copies lie at most 40 bits apart while unrelated
rows of 256 (512) bits lie about 128 (256) bits apart.  Every second set of 120 rows or more holds a second noisy copy of world rows
0 .. 9: as the A side its two copies bid for one column (the uniqueness step decides), as the B side they give a row two near
candidates (the ratio decides).  At least 90 shared rows stay clear of both."""
import functools

import numpy as np

ROW_BLOCK, TILE_B = 256, 128   # csrc/hamming_pairs.hip: A rows per job, B rows per LDS tile
# per-image counts: 0, 1, 2, around the B tile, around the row block, one larger
COUNTS_64 = (0, 1, 2, TILE_B - 1, TILE_B, TILE_B + 1, ROW_BLOCK - 1, ROW_BLOCK, ROW_BLOCK + 1, 300)
COUNTS_32 = (0, 1, TILE_B + 1, ROW_BLOCK + 1, 300)
COUNTS_BITS, NBITS_ODD = (2, TILE_B, ROW_BLOCK, 150), 250   # unpacked-bit sets: 250 bits in 32 bytes

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def _flip(bits_row, which):
    out = bits_row.copy()
    out[list(which)] ^= True
    return out


def make_bit_sets(seed, counts, nbits):
    """[n_i x nbits bool] as described above."""
    rng = np.random.default_rng(seed)
    world = rng.integers(0, 2, (100, nbits)).astype(bool)
    sets = []
    for i, n in enumerate(counts):
        rows = rng.integers(0, 2, (n, nbits)).astype(bool)
        k = min(n, 100)
        spots = rng.permutation(n)
        for w, r in enumerate(spots[:k]):
            rows[r] = _flip(world[w], rng.choice(nbits, int(rng.integers(0, 21)), replace=False))
        if i % 2 == 1 and n >= 120:   # a second copy of world rows 0 .. 9 (see the module's docstring)
            for w, r in enumerate(spots[k:k + 10]):
                rows[r] = _flip(world[w], rng.choice(nbits, int(rng.integers(0, 21)), replace=False))
        sets.append(rows)
    return sets


def pack(bits):
    return np.packbits(bits, axis=1, bitorder="big")


@functools.lru_cache(maxsize=None)
def sets_64():
    return [pack(b) for b in make_bit_sets(11, COUNTS_64, 512)]


@functools.lru_cache(maxsize=None)
def sets_32():
    return [pack(b) for b in make_bit_sets(12, COUNTS_32, 256)]


@functools.lru_cache(maxsize=None)
def sets_odd_bits():
    return make_bit_sets(13, COUNTS_BITS, NBITS_ODD)


@functools.lru_cache(maxsize=None)
def planted():
    """(A bits, B bits, {name: 0-based A row}) of 512-bit rows, one planted row or two per decision of the rule; every other
    distance is that of unrelated random rows (about 256)."""
    rng = np.random.default_rng(14)
    R = rng.integers(0, 2, (8, 512)).astype(bool)
    A, B, rows = [], [], {}
    # B rows 0, 1 equal.  A row 0: 10 bits from both - a tie for the best (lower index wins) and d1 == d2.
    B += [R[0], R[0]]
    rows["best_tie"] = len(A)
    A.append(_flip(R[0], range(10)))
    # A row equal to both: d1 = d2 = 0, the second patched to nBits.  It also takes column 1 from the row above.
    rows["zero_second"] = len(A)
    A.append(R[0])
    # two A rows, 20 bits each from B row 2 and from nothing else: one column, equal distance, the lower row wins
    B.append(R[1])
    rows["column_tie_lo"], rows["column_tie_hi"] = len(A), len(A) + 1
    A += [_flip(R[1], range(20)), _flip(R[1], range(20, 40))]
    # d = 64 of 512 = 12.5 percent: exactly on MatchThreshold = 12.5
    B.append(R[2])
    rows["on_threshold"] = len(A)
    A.append(_flip(R[2], range(64)))
    # 64 against 128: exactly on MaxRatio = 0.5 (and on the threshold)
    B += [R[3], _flip(R[3], list(range(32, 64)) + list(range(64, 160)))]
    rows["on_ratio"] = len(A)
    A.append(_flip(R[3], range(64)))
    # one bit beyond the threshold
    B.append(R[4])
    rows["beyond_threshold"] = len(A)
    A.append(_flip(R[4], range(65)))
    # 63 against 125: one bit beyond the ratio 0.5 (63 > 62.5), inside the threshold
    B += [R[5], _flip(R[5], list(range(31, 63)) + list(range(63, 157)))]
    rows["beyond_ratio"] = len(A)
    A.append(_flip(R[5], range(63)))
    return np.array(A), np.array(B), rows


# ---- the NumPy restatement: brute-force XOR / popcount 2-NN with the mex's tie rule, then the package's host filter --------
def hamming(A, B):
    return _POP[A[:, None, :] ^ B[None, :, :]].sum(-1)


def two_nn(A, B):
    """nearest2HammingExhaustiveMEX.cpp:52-74, the scan itself: strict < moves the best, <= the second; a single candidate
    gives second = 8 * nbytes.  (idx2 1-based, d1, d2) as the mex returns them."""
    D = hamming(A, B)
    idx2, d1, d2 = np.zeros(len(A), np.uint32), np.zeros(len(A), np.float32), np.zeros(len(A), np.float32)
    for i in range(len(A)):
        best, second, ib = 1 << 30, 1 << 30, -1
        for j in range(len(B)):
            h = int(D[i, j])
            if h < best:
                second, best, ib = best, h, j
            elif h <= second:
                second = h
        if len(B) == 1:
            second = 8 * A.shape[1]
        idx2[i], d1[i], d2[i] = ib + 1, best, second
    return idx2, d1, d2


def match(fm, A, B, nbits, MaxRatio, MatchThreshold, Unique, nn=None):
    """matchFeaturesScratch.m:84-88,118-121,170-211,318 on packed rows; fm.filter_matches is the package's host filter."""
    if len(A) == 0 or len(B) == 0:
        return np.zeros((0, 2), np.uint32), np.zeros(0, np.float32)
    idx2, d1, d2 = nn if nn is not None else two_nn(A, B)
    d2 = np.where(d2 == 0, np.float32(nbits), d2).astype(np.float32)
    nb = np.float32(nbits)
    return fm.filter_matches(idx2, (d1 / nb) * np.float32(100), (d2 / nb) * np.float32(100), len(B), MaxRatio, MatchThreshold, Unique, binary=True)


_NN = {}


def expected_csr(fm, name, sets, nbits, pairs, MaxRatio, MatchThreshold, Unique):
    """The restatement over a pair list as (pair_ptr, idx_a, idx_b, metric); the 2-NN of a (data set, pair) is computed once
    and shared by the tests."""
    ptr, ia, ib, met = [0], [], [], []
    for (a, b) in pairs:
        key = (name, int(a), int(b))
        if key not in _NN and len(sets[a]) and len(sets[b]):
            _NN[key] = two_nn(sets[a], sets[b])
        m, d = match(fm, sets[a], sets[b], nbits, MaxRatio, MatchThreshold, Unique, _NN.get(key))
        ia.append(m[:, 0])
        ib.append(m[:, 1])
        met.append(d)
        ptr.append(ptr[-1] + len(m))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    return np.asarray(ptr, np.int64), cat(ia, np.uint32), cat(ib, np.uint32), cat(met, np.float32)


def per_pair_csr(fm, descs, pairs, MaxRatio, MatchThreshold, Unique):
    """The per-pair loop the batched call replaces: matchFeaturesScratch pair after pair (one device search each)."""
    ptr, ia, ib, met = [0], [], [], []
    for (a, b) in pairs:
        m, d = fm.matchFeaturesScratch(descs[a], descs[b], MatchThreshold=MatchThreshold, MaxRatio=MaxRatio, Unique=Unique)
        ia.append(m[:, 0])
        ib.append(m[:, 1])
        met.append(d)
        ptr.append(ptr[-1] + len(m))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    return np.asarray(ptr, np.int64), cat(ia, np.uint32), cat(ib, np.uint32), cat(met, np.float32)


def same_csr(got, want):
    """Every offset, every index, every metric bit, and with them the order."""
    gp, ga, gb, gm = [np.asarray(x) for x in got]
    wp, wa, wb, wm = want
    return (np.array_equal(gp, wp) and np.array_equal(ga.astype(np.uint32), wa) and np.array_equal(gb.astype(np.uint32), wb)
            and gm.dtype == np.float32 and np.array_equal(gm.view(np.uint32), wm.view(np.uint32)))
