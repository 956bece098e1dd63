"""The global matcher's parameter space of test_global_space_gpu.py (helper, not a test): seeded pools, the synthetic filter
tables and the arm of csrc/knn.hip / match.hip each one is there for.  numpy only; the oracle is imported where a function
needs it, the product never.  test_global_cases.py holds every fixture to its arm on the CPU.

Arms (constants restated from the sources):
  SCREENED = 8192  rows from which aps_knn_global_screened (and the blocked aps_knn_global) leave the plain f32 kernel
  WAVE = 64        global_screen_reduce_kernel / global_phase_b_kernel append the rows of a wave's FIRST and LAST image to the
                   per-job lists wave-wide; lanes of an image strictly inside the wave take the `edge` branch (plain atomics)
  column sets of 1, 2, 3 rows: rescore_row3 gives bound = +inf (nothing is unlisted)
  a row's certified prefix is three rows per image / block: a FOURTH near row in one image (the row's own: itself and
                   three copies; another one: four copies) cannot be certified and goes through knn_rows_block_top4_kernel +
                   knn_rows_merge_kernel
  BLOCK = 512      APS_KNN_BLOCK of the blocked tests; a last block of 1, 2, 3 rows has an own-block list with empty slots

Pools (lists of per-image descriptor arrays; rows as in test_global_gpu's screened test: a random subset of one base set per
image, noise U(0, 0.12) per row, clipped at 0, unit norm):
  mosaic   34 images of MOSAIC_SIZES rows (8307 in all): runs of tiny images, an empty one, a tiny last one
  pair2    4200 + 4100 rows sharing 1500 planted rows: n_img == 2, a1 = a2 = -1
  solo     one image of 8200 rows: no cross-image job at all
  crowded  12 images with the plants of CROWDED_PLANTS
blocked_pools(): single arrays for aps_knn_global against itself, plants at BLOCKED_PLANTS"""
import functools
from collections import namedtuple

import numpy as np

from util import sift_like

SCREENED, WAVE, BLOCK, DIM = 8192, 64, 512, 128
EPS32 = np.float32(np.finfo(np.float32).eps)
RATIOS = (0.3, 0.6, 0.95)
TINY = 64  # "an image under 64 rows"

# ---- mosaic ------------------------------------------------------------------------------------------------------------
# the sizes the issue lists, ordered so that the pool starts with a run of tiny images (wave 0 holds images 0..6: five of
# them strictly inside it), the big images sit in the middle, and a second run of tiny images with the empty one closes the
# pool: the non-live lanes of the last wave resolve to the 3-row last image
MOSAIC_SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 193, 255, 257,
                300, 511, 513, 700, 1100, 1500, 1900, 0, 1, 1, 2, 62, 1, 64, 3)
# (seed: the first of 2024, 2025, 2026 with which this order meets every floor of test_global_cases.py with a margin)
MOSAIC_SEED, BASE_ROWS, NOISE_MAX = 2026, 2600, 0.12

PAIR2_SIZES, PAIR2_COMMON = (4200, 4100), 1500
SOLO_SIZES = (8200,)

# ---- crowded -----------------------------------------------------------------------------------------------------------
CROWDED_SIZES = (40, 1200, 7, 1500, 7, 1800, 900, 20, 1400, 1100, 300, 5)
CROWDED_RESERVED = 8  # base rows 0..7 enter no image's random subset: a plant's row exists only where it is planted
NEAR_NOISE, CLEAR_NOISE = (1e-3, 2e-3, 3e-3), 5e-3
# (image, local row) 0-based
CROWDED_PLANTS = {
    # r and its three near-copies in r's OWN image, one clear copy elsewhere: self + three copies are r's four nearest, the
    # own image's certified prefix of three cannot certify the fourth -> exact-rows repair.  All four lie in r's image, so
    # the filter keeps nothing of r (fewer than two cross-image rows); the clear copy makes r's two nearest cross-image
    # rows a clear match, so no correct screen may dismiss r
    "own": {"row": (3, 10), "copies": ((3, 400), (3, 800), (3, 1200)), "clear": (5, 77)},
    # the same with the three near-copies in ANOTHER image: a clear match that the filter accepts
    "other": {"row": (1, 20), "copies": ((8, 100), (8, 600), (8, 1300)), "clear": (6, 33)},
    # five exact duplicates in five images: ties resolve by pool index; the last one does not see itself in its four nearest
    "dups": ((0, 5), (1, 1000), (4, 3), (9, 50), (11, 2)),
    "zero": (6, 500),            # an all-zero row: aps_global_normalize gives 0 / sqrt(eps) = 0
    "twins": (2, 4),             # image 4's rows (but the duplicate planted above) are exact copies of image 2's
}

# ---- blocked pools -----------------------------------------------------------------------------------------------------
BLOCKED_MASTER = 8704 + 77
BLOCKED_UNIT_ROWS = (8192, 8193, 8194, 8195, 8704 + 77)  # last block of 512, 1, 2, 3, 77 rows
BLOCKED_SCALES = (1e-4, 300.0, 7e4)
BLOCKED_PLANTS = {
    "three": {"row": 100, "copies": (2600, 2700, 2800)},             # block 0 -> three near-copies in block 5
    # block 1 -> four near rows in block 9; the fourth is an exact copy of the third, so the third's distance is not
    # strictly below block 9's bound whatever the f16 screen's error term is: the row is recomputed against the whole pool
    "four": {"row": 700, "copies": (4700, 4710, 4720, 4730)},
    "dups": (1500, 1501, 6000, 6001, 7700),                          # blocks 2, 2, 11, 11, 15
    "zero": 5555,
}
BlockedPool = namedtuple("BlockedPool", "name x last_rows")

# ---- pinned statistics of the generators above (oracle chain, k = 4; test_global_cases.py recomputes them) -----------------
# pool -> rows, {ratio: (accepted matches, those with an endpoint in an image under 64 rows)}
PINNED = {
    "mosaic": (8307, {0.3: (749, 41), 0.6: (2310, 146), 0.95: (6719, 403)}),
    "pair2": (8300, {0.3: (1018, 0), 0.6: (1828, 0), 0.95: (2928, 0)}),
    "solo": (8200, {0.3: (0, 0), 0.6: (0, 0), 0.95: (0, 0)}),
    "crowded": (8279, {0.3: (866, 33), 0.6: (2356, 60), 0.95: (6830, 122)}),
}
# ---- pinned work of the device chain (measured on the library BEFORE its merge / proof / append steps were stated once; a
# refactor that screens or certifies less leaves every table bit-exact and only these counts move) ---------------------------
# pool -> {ratio: rows aps_knn_global_screen_stats reports as survivors of phase 0's proof, k = 4}
SCREEN_SURVIVORS = {
    "mosaic": {0.3: 1239, 0.6: 3239, 0.95: 8307},
    "pair2": {0.3: 1492, 0.6: 2565, 0.95: 8298},
    "solo": {0.3: 8200, 0.6: 8200, 0.95: 8200},
    "crowded": {0.3: 7538, 0.6: 7750, 0.95: 8279},
}
# rows the merge kernels could not certify (APS_TRACE's counts): crowded through aps_knn_global_screened at ratio 0.6,
# unit8193 through the blocked aps_knn_global at APS_KNN_BLOCK = BLOCK
RECOMPUTED = {"crowded": 8, "unit8193": 2}
MOSAIC_TINY_IMAGES_MATCHED = 13  # distinct images under 64 rows that take part in a match at ratio 0.6


def _freeze(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


def _unit(v):
    v = np.maximum(np.asarray(v, np.float32), 0)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _noisy_subset(rng, base, keep):
    """test_global_gpu's recipe: the kept base rows plus noise of a per-row amplitude U(0, NOISE_MAX), clipped, unit norm."""
    noise = rng.uniform(0.0, NOISE_MAX, len(keep))[:, None]
    d = np.maximum(base[keep] + noise * rng.standard_normal((len(keep), DIM)).astype(np.float32), 0)
    if len(keep) == 0:
        return np.zeros((0, DIM), np.float32)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _near(rng, row, amp):
    return _unit(row + np.float32(amp) * rng.standard_normal(DIM).astype(np.float32))


@functools.lru_cache(maxsize=None)
def mosaic():
    rng = np.random.default_rng(MOSAIC_SEED)
    base = sift_like(rng, BASE_ROWS)
    return _freeze([_noisy_subset(rng, base, rng.permutation(BASE_ROWS)[:n]) for n in MOSAIC_SIZES])


@functools.lru_cache(maxsize=None)
def pair2():
    rng = np.random.default_rng(2025)
    a, b = sift_like(rng, PAIR2_SIZES[0]), sift_like(rng, PAIR2_SIZES[1])
    ia, ib = rng.permutation(PAIR2_SIZES[0])[:PAIR2_COMMON], rng.permutation(PAIR2_SIZES[1])[:PAIR2_COMMON]
    b[ib] = _noisy_subset(rng, a, ia)
    return _freeze([a, b])


@functools.lru_cache(maxsize=None)
def solo():
    rng = np.random.default_rng(2026)
    x = sift_like(rng, SOLO_SIZES[0])
    x[4000:4300] = _noisy_subset(rng, x, np.arange(300))  # near rows inside the one image
    x[8199] = x[0]
    return _freeze([x])


@functools.lru_cache(maxsize=None)
def crowded():
    rng = np.random.default_rng(2027)
    base = sift_like(rng, BASE_ROWS)
    free = np.arange(CROWDED_RESERVED, BASE_ROWS)
    imgs = [_noisy_subset(rng, base, rng.permutation(free)[:n]) for n in CROWDED_SIZES]
    P = CROWDED_PLANTS
    for b, key in ((0, "own"), (1, "other")):
        (i, r) = P[key]["row"]
        imgs[i][r] = base[b]
        for (ci, cr), amp in zip(P[key]["copies"], NEAR_NOISE):
            imgs[ci][cr] = _near(rng, base[b], amp)
        ci, cr = P[key]["clear"]
        imgs[ci][cr] = _near(rng, base[b], CLEAR_NOISE)
    a, b = P["twins"]
    imgs[b][:] = imgs[a]
    for i, r in P["dups"]:
        imgs[i][r] = base[2]
    i, r = P["zero"]
    imgs[i][r] = 0
    return _freeze(imgs)


POOLS = {"mosaic": mosaic, "pair2": pair2, "solo": solo, "crowded": crowded}
POOL_SIZES = {"mosaic": MOSAIC_SIZES, "pair2": PAIR2_SIZES, "solo": SOLO_SIZES, "crowded": CROWDED_SIZES}


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def pool_row(name, image, local):
    """0-based pool index of (image, local row)."""
    return int(offsets(POOL_SIZES[name])[image]) + local


# ---- blocked pools -----------------------------------------------------------------------------------------------------
def _plant_blocked(rng, x, raw):
    """The plants of BLOCKED_PLANTS into x (in place).  raw: integer-valued rows (copies differ by +1 in 1, 2, 3 entries)."""
    P = BLOCKED_PLANTS
    for key in ("three", "four"):
        src = x[P[key]["row"]]
        for e, dst in enumerate(P[key]["copies"]):
            if key == "four" and e == 3:
                x[dst] = x[P[key]["copies"][2]]
            elif raw:
                v = src.copy()
                v[rng.permutation(DIM)[:e + 1]] += 1
                x[dst] = v
            else:
                x[dst] = _near(rng, src, NEAR_NOISE[e])
    for dst in P["dups"][1:]:
        x[dst] = x[P["dups"][0]]
    x[P["zero"]] = 0


@functools.lru_cache(maxsize=None)
def _blocked_master():
    rng = np.random.default_rng(2028)
    x = sift_like(rng, BLOCKED_MASTER)
    _plant_blocked(rng, x, False)
    x.setflags(write=False)
    return x


def _cut(x, n):
    """The first n rows, the last of them an exact duplicate of row 0 (in the last, possibly 1-row, block)."""
    y = np.array(x[:n])
    y[n - 1] = y[0]
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def blocked_pools():
    out = []
    for n in BLOCKED_UNIT_ROWS:
        out.append(BlockedPool(f"unit{n}", _cut(_blocked_master(), n), (n - 1) % BLOCK + 1))
    rng = np.random.default_rng(2029)
    raw = sift_like(rng, 8193, unit=False)
    _plant_blocked(rng, raw, True)
    out.append(BlockedPool("raw8193", _cut(raw, 8193), 1))
    for s in BLOCKED_SCALES:
        y = (_cut(_blocked_master(), 8193) * np.float32(s)).astype(np.float32)
        y.setflags(write=False)
        out.append(BlockedPool(f"unit8193x{s:g}", y, 1))
    return tuple(out)


def blocked_pool(name):
    return next(p for p in blocked_pools() if p.name == name)


@functools.lru_cache(maxsize=None)
def blocked_knn(name):
    """oracle.knn of a blocked pool against itself, k = 4 (a smaller k is its prefix: the list is (distance, index) ascending)."""
    import oracle

    x = blocked_pool(name).x
    i, d = oracle.knn(x, x, 4)
    i.setflags(write=False)
    d.setflags(write=False)
    return i, d


# ---- the oracle chain --------------------------------------------------------------------------------------------------
def normalize(pool):
    """featureMatchingGlobal.m:83-85 in single: k-ascending separate multiply and add, eps inside the root."""
    pool = np.ascontiguousarray(pool, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = np.zeros(len(pool), np.float32)
        for kk in range(pool.shape[1]):
            sq = sq + pool[:, kk] * pool[:, kk]
        return (pool / np.sqrt(sq + EPS32)[:, None]).astype(np.float32)


def image_tables(counts):
    """(img_idx, local_idx) of a pool, 1-based uint32."""
    img = np.repeat(np.arange(1, len(counts) + 1, dtype=np.uint32), counts)
    loc = np.concatenate([np.arange(1, c + 1, dtype=np.uint32) for c in counts] + [np.zeros(0, np.uint32)])
    return img, loc.astype(np.uint32)


def oracle_knn_pool(descs, k):
    """(normalised pool, nn_idx, nn_dist, img_idx, local_idx): normalise -> oracle.knn of the pool against itself."""
    import oracle

    pool = normalize(np.concatenate([np.asarray(d, np.float32).reshape(-1, DIM) for d in descs]))
    img, loc = image_tables([len(d) for d in descs])
    ni, nd = oracle.knn(pool, pool, k)
    return pool, ni, nd, img, loc


def oracle_chain(descs, ratio, k):
    """normalise -> oracle.knn -> oracle.global_filter: rows (image i, image j, local i, local j), 1-based, query order."""
    import oracle

    _, ni, nd, img, loc = oracle_knn_pool(descs, k)
    return oracle.global_filter(ni, nd, img, loc, ratio)


@functools.lru_cache(maxsize=None)
def _pool_knn4(name):
    out = oracle_knn_pool(POOLS[name](), 4)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pool_knn(name, k):
    """oracle_knn_pool of a named pool, once per (pool, k).  oracle.knn's list is the (distance, index)-ascending head of the
    pool whatever k is, so k < 4 is the prefix of the one k = 4 search (test_global_cases.py checks that on a sample)."""
    pool, ni, nd, img, loc = _pool_knn4(name)
    ni, nd = np.ascontiguousarray(ni[:, :k]), np.ascontiguousarray(nd[:, :k])
    ni.setflags(write=False)
    nd.setflags(write=False)
    return pool, ni, nd, img, loc


@functools.lru_cache(maxsize=None)
def pool_chain(name, ratio, k):
    """oracle_chain of a named pool on the cached k-NN."""
    import oracle

    _, ni, nd, img, loc = pool_knn(name, k)
    rows = oracle.global_filter(ni, nd, img, loc, ratio)
    rows.setflags(write=False)
    return rows


def accepted_queries(name, ratio, k):
    """Pool rows (0-based, ascending) for which the oracle chain accepts a match: the filter's decision restated per row."""
    _, ni, nd, img, _ = pool_knn(name, k)
    return filter_accepts(ni, nd, img, ratio)


def filter_accepts(nn_idx, nn_dist, img_idx, ratio):
    """featureMatchingGlobal.m:129-147 per query in numpy (single arithmetic): the 0-based queries that keep a match.
    test_global_cases.py holds it to oracle.global_filter's count."""
    f, k = nn_idx.shape
    ids = nn_idx.astype(np.int64)
    valid = (ids != 0) & (ids != np.arange(1, f + 1)[:, None]) & (img_idx[np.maximum(ids, 1) - 1] != img_idx[:, None])
    rank = np.cumsum(valid, axis=1)
    has2 = rank[:, -1] >= 2
    d = np.asarray(nn_dist, np.float32)
    d0 = np.where(valid & (rank == 1), d, 0).sum(axis=1, dtype=np.float32)  # (one term per row: exact)
    d1 = np.where(valid & (rank == 2), d, 0).sum(axis=1, dtype=np.float32)
    with np.errstate(all="ignore"):
        r = (d0 / np.maximum(d1, EPS32)).astype(np.float32)
    return np.flatnonzero(has2 & ~(r > np.float32(ratio)))


def csr_of(rows, n_img, pair_order):
    """Oracle filter rows -> (pair_ptr, idx_i, idx_j) in the given pair order, query order within a pair."""
    pp, oi, oj = [0], [], []
    for i, j in pair_order:
        sel = rows[(rows[:, 0] == i + 1) & (rows[:, 1] == j + 1)]
        oi.append(sel[:, 2])
        oj.append(sel[:, 3])
        pp.append(pp[-1] + len(sel))
    cat = lambda parts: np.concatenate(parts + [np.zeros(0, np.uint32)]).astype(np.uint32)  # noqa: E731
    return np.asarray(pp, np.int64), cat(oi), cat(oj)


def touches_tiny(rows, sizes):
    """Mask of the oracle filter rows with an endpoint in an image of fewer than TINY rows."""
    s = np.asarray(sizes)
    return (s[rows[:, 0].astype(np.int64) - 1] < TINY) | (s[rows[:, 1].astype(np.int64) - 1] < TINY)


# ---- aps_global_filter tables --------------------------------------------------------------------------------------------
FilterCase = namedtuple("FilterCase", "name nn_idx nn_dist img_idx local_idx n_img ratio k")


def _next(x, n):
    """x moved by n ulp (n may be negative), in single."""
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return x


def _boundary_case(name, ratio, seed):
    """Two images; every query has its two cross-image neighbours in slots 1 and 2 (slot 0 is itself), the first distance
    scattered within +-3 ulp of float32(ratio) * d1: rows on both sides of the single-precision boundary, and rows where the
    double quotient of the same singles decides differently."""
    rng = np.random.default_rng(seed)
    n = 400
    f = 2 * n
    img = np.repeat(np.array([1, 2], np.uint32), n)
    loc = np.tile(np.arange(1, n + 1, dtype=np.uint32), 2)
    idx = np.zeros((f, 4), np.uint32)
    dist = np.zeros((f, 4), np.float32)
    d1 = rng.uniform(0.05, 1.5, f).astype(np.float32)
    for q in range(f):
        other = (n if q < n else 0)
        a, b = rng.permutation(n)[:2] + other
        idx[q] = (q + 1, a + 1, b + 1, (q + 1) % n + (0 if q < n else n) + 1)
        d0 = _next(np.float32(ratio) * d1[q], int(rng.integers(-3, 4)))
        dist[q] = (0, d0, d1[q], d1[q] + np.float32(0.25))
    return FilterCase(name, idx, dist, img, loc, 2, ratio, 4)


def boundary_split(case):
    """(single decision, double decision) per query of a boundary case: accept = not (d0 / d1 > ratio)."""
    d0, d1 = case.nn_dist[:, 1], case.nn_dist[:, 2]
    single = ~((d0 / d1).astype(np.float32) > np.float32(case.ratio))
    double = ~((d0.astype(np.float64) / d1.astype(np.float64)) > float(np.float32(case.ratio)))
    return single, double


def _random_table(rng, counts, k, self_first=True):
    """A plausible table: slot 0 the query itself, the others random rows of the pool, ascending random distances."""
    img, loc = image_tables(counts)
    f = len(img)
    idx = rng.integers(1, f + 1, (f, k)).astype(np.uint32)
    if self_first:
        idx[:, 0] = np.arange(1, f + 1)
    dist = np.sort(rng.uniform(0.0, 1.0, (f, k)).astype(np.float32), axis=1)
    if self_first:
        dist[:, 0] = 0
    return idx, dist, img, loc


@functools.lru_cache(maxsize=None)
def filter_tables():
    cases = []
    # k = 1 .. 8 on five images (one empty, one of a single row)
    for k in range(1, 9):
        rng = np.random.default_rng(3000 + k)
        counts = [120, 0, 1, 77, 200]
        idx, dist, img, loc = _random_table(rng, counts, k)
        odd = np.arange(len(img)) % 2 == 1  # every other query does not list itself (k = 2 could accept nothing otherwise)
        idx[odd, 0] = rng.integers(1, len(img) + 1, int(odd.sum()))
        cases.append(FilterCase(f"k{k}", idx, dist, img, loc, len(counts), 0.6, k))
    # a missing neighbour (index 0) in any slot, slot 0 included; self in slot 1 or 2 (exact duplicates with a lower index)
    rng = np.random.default_rng(3100)
    counts = [150, 90, 60, 3]
    idx, dist, img, loc = _random_table(rng, counts, 4)
    f = len(img)
    for q in range(f):
        m = q % 8
        if m < 4:
            idx[q, m] = 0
        elif m < 6:  # a lower-indexed duplicate ahead of the query itself
            s = m - 3
            idx[q, s] = q + 1
            idx[q, 0] = rng.integers(1, f + 1)
            dist[q, :s + 1] = 0
        elif m == 6:
            idx[q, :] = 0
    cases.append(FilterCase("holes_and_self", idx, dist, img, loc, len(counts), 0.8, 4))
    # all neighbours in the query's own image; exactly one cross-image neighbour; exactly two in the last slots
    rng = np.random.default_rng(3200)
    counts = [100, 100, 100]
    idx, dist, img, loc = _random_table(rng, counts, 4)
    off = offsets(counts)
    for q in range(len(img)):
        i = int(img[q]) - 1
        own = lambda: int(rng.integers(off[i], off[i + 1])) + 1  # noqa: E731
        oth = lambda: int(rng.integers(off[(i + 1) % 3], off[(i + 1) % 3 + 1])) + 1  # noqa: E731
        m = q % 3
        idx[q, 1:] = (own(), own(), own()) if m == 0 else (own(), oth(), own()) if m == 1 else (own(), oth(), oth())
    cases.append(FilterCase("own_image", idx, dist, img, loc, 3, 0.9, 4))
    # the divisor: d1 == 0, 0 < d1 < eps('single'), d1 == eps, d0 == d1 (ratio 1 > 0.6; 0 / eps with both zero passes)
    counts = [64, 64]
    img, loc = image_tables(counts)
    f = 128
    idx = np.zeros((f, 4), np.uint32)
    dist = np.zeros((f, 4), np.float32)
    tiny = (np.float32(0), np.float32(1e-45), np.float32(3e-8), _next(EPS32, -1), EPS32, _next(EPS32, 1), np.float32(1e-5))
    for q in range(f):
        o = 64 if q < 64 else 0
        idx[q] = (q + 1, o + (q * 7) % 64 + 1, o + (q * 11 + 3) % 64 + 1, o + (q * 13 + 5) % 64 + 1)
        d1 = tiny[q % 7]
        d0 = (np.float32(0), d1, np.float32(0.5) * d1, np.float32(0.6) * min(d1, EPS32) if d1 > 0 else d1)[(q // 7) % 4]
        dist[q] = (0, d0, d1, max(d1, np.float32(0.1)))
    cases.append(FilterCase("divisor", idx, dist, img, loc, 2, 0.6, 4))
    counts = [50, 50]
    img, loc = image_tables(counts)
    idx = np.zeros((100, 3), np.uint32)
    dist = np.zeros((100, 3), np.float32)
    for q in range(100):
        o = 50 if q < 50 else 0
        idx[q] = (q + 1, o + q % 50 + 1, o + (q + 1) % 50 + 1)
        dist[q] = (0, 0.25 + q / 400, 0.25 + q / 400)
    cases.append(FilterCase("d0_eq_d1_ratio1", idx, dist, img, loc, 2, 1.0, 3))
    cases.append(FilterCase("d0_eq_d1", idx, dist, img, loc, 2, 0.6, 3))
    # the single-precision ratio boundary
    cases.append(_boundary_case("boundary0.6", 0.6, 3300))
    cases.append(_boundary_case("boundary0.1", 0.1, 3301))
    # 40 images (780 pairs), some without rows and some with one: the pair key (b-1)(b-2)/2 + (a-1)
    rng = np.random.default_rng(3400)
    counts = [int(c) for c in rng.integers(5, 60, 40)]
    for i in (0, 7, 8, 39):
        counts[i] = 0
    for i in (1, 20, 38):
        counts[i] = 1
    idx, dist, img, loc = _random_table(rng, counts, 4)
    dist[:, 1] *= np.float32(0.3)  # most queries pass
    cases.append(FilterCase("images40", idx, dist, img, loc, 40, 0.6, 4))
    # matches only in the last pair (images 5 and 6 of six); the other images' queries have own-image neighbours only
    rng = np.random.default_rng(3500)
    counts = [30, 30, 30, 30, 45, 55]
    img, loc = image_tables(counts)
    off = offsets(counts)
    f = len(img)
    idx = np.zeros((f, 4), np.uint32)
    dist = np.sort(rng.uniform(0, 1, (f, 4)).astype(np.float32), axis=1)
    dist[:, 0] = 0
    dist[:, 1] *= np.float32(0.2)
    for q in range(f):
        i = int(img[q]) - 1
        j = {4: 5, 5: 4}.get(i, i)
        idx[q] = (q + 1, *(rng.integers(off[j], off[j + 1], 3) + 1))
    cases.append(FilterCase("last_pair_only", idx, dist, img, loc, 6, 0.6, 4))
    for c in cases:
        for a in (c.nn_idx, c.nn_dist, c.img_idx, c.local_idx):
            a.setflags(write=False)
    return tuple(cases)


# ---- aps_global_normalize -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def normalize_rows():
    """300 raw rows: ordinary 0..255 ones, zero rows, rows of subnormal entries, a row of 1e19 entries (its sum of squares
    overflows: the row normalises to zeros).  No input whose result is NaN (an infinite entry would give inf / inf)."""
    rng = np.random.default_rng(3600)
    x = sift_like(rng, 300, unit=False)
    x[0] = 0
    x[150] = 0
    x[299] = 0
    x[7] = np.float32(1e-45)
    x[8] = rng.integers(0, 5, DIM).astype(np.float32) * np.float32(1e-42)
    x[9] = np.float32(1e-39)
    x[10] = np.float32(1e19)
    x[11, ::2] = np.float32(1e-20)
    x[12] = x[12] * np.float32(1e-3)
    x.setflags(write=False)
    return x
