"""CPU keeper of global_cases.py: every fixture still is what its GPU test (test_global_space_gpu.py) needs, by the oracle
alone.  A change to a generator fails here instead of silently hollowing out the GPU test."""
import numpy as np
import pytest

import global_cases as gc
import oracle
from util import bits

STATED_SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 193, 255, 257, 0, 1, 1, 2, 62, 1, 64, 3, 300, 511,
                513, 700, 1100, 1500, 1900)


def test_size_lists_and_the_screened_threshold():
    assert sorted(gc.MOSAIC_SIZES) == sorted(STATED_SIZES) and len(gc.MOSAIC_SIZES) == 34 and sum(gc.MOSAIC_SIZES) == 8307
    assert gc.PAIR2_SIZES == (4200, 4100) and gc.PAIR2_COMMON == 1500 and gc.SOLO_SIZES == (8200,)
    for name, make in gc.POOLS.items():
        descs = make()
        assert tuple(len(d) for d in descs) == gc.POOL_SIZES[name], name
        assert all(d.dtype == np.float32 and d.shape[1] == 128 for d in descs), name
        rows = sum(len(d) for d in descs)
        assert rows >= gc.SCREENED and rows == gc.PINNED[name][0], name   # the screened path, not the small-pool shortcut
    assert sum(gc.MOSAIC_SIZES) < 9000


def test_mosaic_shape_properties():
    sizes = gc.MOSAIC_SIZES
    off = gc.offsets(sizes)
    img = np.repeat(np.arange(len(sizes)), sizes)
    # a wave of 64 pooled rows (aligned from the pool's first row) with at least four images, i.e. at least two strictly inside
    spans = [len(np.unique(img[w:w + gc.WAVE])) for w in range(0, len(img), gc.WAVE)]
    assert max(spans) >= 4
    assert spans[0] >= 4 and max(spans[1:]) >= 4  # the first wave, and one that begins inside a large image
    assert spans[-1] >= 2                         # the last (partly non-live) wave ends in another image than it began
    for n in (1, 2, 3, 63, 64, 65):
        assert n in sizes
    assert 0 in sizes and sizes.index(0) not in (0, len(sizes) - 1)
    assert 0 < sizes[-1] <= 3                   # the non-live lanes of the last wave resolve to a tiny image
    assert off[-1] % gc.WAVE != 0               # ... and there are such lanes
    # runs of tiny images next to each other, at both ends
    assert all(s < gc.TINY for s in sizes[:8]) and sum(s < gc.TINY for s in sizes[-8:]) >= 6


@pytest.mark.parametrize("name", list(gc.POOLS))
def test_oracle_match_counts_are_the_pinned_ones(name):
    sizes = gc.POOL_SIZES[name]
    for ratio in gc.RATIOS:
        rows = gc.pool_chain(name, ratio, 4)
        tiny = int(gc.touches_tiny(rows, sizes).sum()) if len(rows) else 0
        assert (len(rows), tiny) == gc.PINNED[name][1][ratio], (name, ratio)
        # the per-row restatement of the filter that the GPU table test uses
        assert len(gc.accepted_queries(name, ratio, 4)) == len(rows)
    for k in (1, 2, 3):
        for ratio in gc.RATIOS:
            assert len(gc.accepted_queries(name, ratio, k)) == len(gc.pool_chain(name, ratio, k))
    assert len(gc.pool_chain(name, 0.6, 1)) == 0   # k = 1: never two candidates


def test_mosaic_floors():
    """Floors, not measurements: enough accepted matches touch images smaller than a wave for a wrong list append to show."""
    sizes = np.asarray(gc.MOSAIC_SIZES)
    r06, r03 = gc.pool_chain("mosaic", 0.6, 4), gc.pool_chain("mosaic", 0.3, 4)
    assert gc.touches_tiny(r06, sizes).sum() >= 100
    assert gc.touches_tiny(r03, sizes).sum() >= 30
    tiny = set((np.flatnonzero(sizes < gc.TINY) + 1).tolist())
    seen = (set(r06[:, 0].tolist()) | set(r06[:, 1].tolist())) & tiny
    assert len(seen) >= 10 and len(seen) == gc.MOSAIC_TINY_IMAGES_MATCHED
    assert len(gc.pool_chain("solo", 0.95, 4)) == 0 and len(gc.pool_chain("pair2", 0.6, 4)) > 500


def test_prefix_property_of_the_oracle_knn():
    """pool_knn serves k < 4 as the prefix of one k = 4 search."""
    pool = gc.pool_knn("crowded", 4)[0][::9]
    i4, d4 = oracle.knn(pool, pool, 4)
    for k in (1, 2, 3):
        ik, dk = oracle.knn(pool, pool, k)
        assert np.array_equal(ik, i4[:, :k]) and np.array_equal(bits(dk), bits(d4[:, :k]))


def test_oracle_chain_is_the_written_out_chain():
    """oracle_chain against the chain test_global_gpu.py used to write out, on a small pool."""
    rng = np.random.default_rng(5)
    descs = [gc.sift_like(rng, n) for n in (40, 0, 25)]
    descs[2][3] = descs[0][7]
    pool = np.concatenate(descs)
    sq = np.zeros(len(pool), np.float32)
    for kk in range(128):
        sq = sq + pool[:, kk] * pool[:, kk]
    pool = (pool / np.sqrt(sq + np.float32(np.finfo(np.float32).eps))[:, None]).astype(np.float32)
    img = np.repeat(np.arange(1, 4, dtype=np.uint32), [40, 0, 25])
    loc = np.concatenate([np.arange(1, c + 1, dtype=np.uint32) for c in (40, 0, 25)])
    ni, nd = oracle.knn(pool, pool, 4)
    want = oracle.global_filter(ni, nd, img, loc, 0.95)
    assert np.array_equal(gc.oracle_chain(descs, 0.95, 4), want) and len(want) > 0


def _cross_ratio(pool, img, q):
    """d(first) / d(second) of q's two nearest rows of OTHER images, in double."""
    d = ((pool.astype(np.float64) - pool[q].astype(np.float64)) ** 2).sum(axis=1)
    d = np.sort(d[img != img[q]])
    return d[0] / d[1]


def test_crowded_plants():
    pool, ni, nd, img, _ = gc.pool_knn("crowded", 4)
    P = gc.CROWDED_PLANTS
    row = lambda il: gc.pool_row("crowded", *il)  # noqa: E731
    acc = set(gc.accepted_queries("crowded", 0.6, 4).tolist())
    for key in ("own", "other"):
        q = row(P[key]["row"])
        copies = [row(c) for c in P[key]["copies"]]
        assert ni[q].tolist() == [q + 1] + [c + 1 for c in copies], key  # (noise 1e-3 < 2e-3 < 3e-3: in planting order)
        assert np.all(np.diff(nd[q]) > 0) and nd[q, 3] < 3e-3
        # the fifth nearest is the clear copy, in an image that holds no other row near q
        d = ((pool.astype(np.float64) - pool[q].astype(np.float64)) ** 2).sum(axis=1)
        assert np.argsort(d, kind="stable")[4] == row(P[key]["clear"])
        assert img[row(P[key]["clear"])] not in (img[q], img[copies[0]])
    q_own, q_other = row(P["own"]["row"]), row(P["other"]["row"])
    # own: itself and three copies in ONE image - the fourth of them is beyond the image's certified prefix of three
    assert len({int(img[i - 1]) for i in ni[q_own]}) == 1
    # other: three copies in one other image; the filter accepts the row
    assert len({int(img[i - 1]) for i in ni[q_other][1:]}) == 1 and img[ni[q_other, 1] - 1] != img[q_other]
    assert q_other in acc
    # own: all four nearest lie in the row's image, so the filter can keep nothing of it; what keeps the row from being
    # dismissed is the clear copy: its two nearest cross-image rows pass every ratio of the sweep by a wide margin
    assert q_own not in acc
    assert _cross_ratio(pool, img, q_own) < 0.05 and _cross_ratio(pool, img, q_other) < 0.5
    # five exact duplicates: ascending index, equal distance bits, whichever of them asks
    dups = [row(d) for d in P["dups"]]
    assert dups == sorted(dups) and len({int(img[d]) for d in dups}) == 5
    for q in dups:
        assert ni[q].tolist() == [d + 1 for d in dups[:4]]
        assert len(set(bits(nd[q]).tolist())) == 1
        assert q in acc
    assert dups[4] + 1 not in ni[dups[4]]        # the last duplicate is not among its own four nearest
    # the zero row normalises to zeros; the twins are bitwise copies
    z = row(P["zero"])
    assert not pool[z].any() and ni[z, 0] == z + 1
    a, b = P["twins"]
    da, db = gc.crowded()[a], gc.crowded()[b]
    keep = [r for r in range(len(da)) if (b, r) not in P["dups"]]
    assert len(da) == len(db) < gc.TINY and np.array_equal(bits(da[keep]), bits(db[keep])) and len(keep) >= 5


@pytest.mark.parametrize("name", [p.name for p in gc.blocked_pools()])
def test_blocked_pool_plants(name):
    p = gc.blocked_pool(name)
    x, n = p.x, len(p.x)
    idx, dist = gc.blocked_knn(name)
    blk = lambda r: r // gc.BLOCK  # noqa: E731
    assert n >= gc.SCREENED and x.dtype == np.float32
    assert p.last_rows == n - (n - 1) // gc.BLOCK * gc.BLOCK and (n - 1) // gc.BLOCK + 1 >= 16
    B = gc.BLOCKED_PLANTS
    for key in ("three", "four"):
        q, c = B[key]["row"], B[key]["copies"]
        assert idx[q].tolist() == [q + 1, c[0] + 1, c[1] + 1, c[2] + 1], key
        assert len({blk(r) for r in c}) == 1 and blk(c[0]) != blk(q)
    c = B["four"]["copies"]
    assert np.array_equal(bits(x[c[3]]), bits(x[c[2]])) and not np.array_equal(x[c[2]], x[c[1]])
    d = B["dups"]
    assert len({blk(r) for r in d}) == 3
    for q in d:
        assert idx[q].tolist() == [r + 1 for r in d[:4]] and len(set(bits(dist[q]).tolist())) == 1
    assert not x[B["zero"]].any()
    # an exact duplicate of row 0 in the last block: row 0 sees it second, it sees row 0 first
    assert np.array_equal(bits(x[n - 1]), bits(x[0])) and blk(n - 1) == (n - 1) // gc.BLOCK
    assert idx[0, :2].tolist() == [1, n] and idx[n - 1, :2].tolist() == [1, n]
    if name.startswith("raw"):
        assert np.array_equal(x, np.round(x)) and x.max() > 50 and dist[B["four"]["row"]].tolist() == [0, 1, 2, 3]


def test_blocked_pool_list():
    pools = gc.blocked_pools()
    assert [len(p.x) for p in pools[:5]] == [8192, 8193, 8194, 8195, 8781]
    assert [p.last_rows for p in pools] == [512, 1, 2, 3, 77, 1, 1, 1, 1]
    unit = gc.blocked_pool("unit8193").x
    assert np.allclose(np.linalg.norm(unit[:50], axis=1), 1, atol=1e-6)
    for s in gc.BLOCKED_SCALES:
        assert np.array_equal(gc.blocked_pool(f"unit8193x{s:g}").x, unit * np.float32(s))


def test_filter_tables_cover_their_arms():
    cases = {c.name: c for c in gc.filter_tables()}
    assert sorted(c.k for c in cases.values() if c.name.startswith("k")) == list(range(1, 9))
    for c in cases.values():
        assert c.nn_idx.shape == c.nn_dist.shape == (len(c.img_idx), c.k) and c.nn_idx.max() <= len(c.img_idx)
    h = cases["holes_and_self"]
    f = len(h.img_idx)
    me = np.arange(1, f + 1)
    for s in range(4):
        assert (h.nn_idx[:, s] == 0).any()
    assert (h.nn_idx[:, 1] == me).any() and (h.nn_idx[:, 2] == me).any() and (h.nn_idx == 0).all(axis=1).any()
    o = cases["own_image"]
    cross = (o.img_idx[o.nn_idx[:, 1:] - 1] != o.img_idx[:, None]).sum(axis=1)
    assert set(cross.tolist()) == {0, 1, 2}
    dv = cases["divisor"]
    d1 = dv.nn_dist[:, 2]
    assert (d1 == 0).any() and ((d1 > 0) & (d1 < gc.EPS32)).any() and (d1 == gc.EPS32).any() and (d1 > gc.EPS32).any()
    assert np.array_equal(cases["d0_eq_d1"].nn_dist[:, 1], cases["d0_eq_d1"].nn_dist[:, 2])
    for name, ratio in (("boundary0.6", 0.6), ("boundary0.1", 0.1)):
        c = cases[name]
        assert c.ratio == ratio
        single, double = gc.boundary_split(c)
        assert single.any() and (~single).any()            # rows on both sides of float32(ratio)
        assert (single != double).sum() >= 5               # a double comparison decides differently from MATLAB's single one
        want = oracle.global_filter(c.nn_idx, c.nn_dist, c.img_idx, c.local_idx, c.ratio)
        assert len(want) == int(single.sum())              # the oracle takes the single side
    m = cases["images40"]
    counts = np.bincount(m.img_idx, minlength=41)[1:]
    assert m.n_img == 40 and (counts == 0).sum() >= 3 and (counts == 1).sum() >= 3 and counts[39] == 0 and counts[0] == 0
    rows = oracle.global_filter(m.nn_idx, m.nn_dist, m.img_idx, m.local_idx, m.ratio)
    assert len({(int(a), int(b)) for a, b in rows[:, :2]}) > 300 and rows[:, 1].max() == 39
    lp = cases["last_pair_only"]
    rows = oracle.global_filter(lp.nn_idx, lp.nn_dist, lp.img_idx, lp.local_idx, lp.ratio)
    assert len(rows) > 20 and {(int(a), int(b)) for a, b in rows[:, :2]} == {(5, 6)}
    # every case has accepted and rejected queries, but for k = 1 (nothing passes) and d0 == d1: a quotient of exactly 1,
    # which passes ratio 1 (the test is `> ratio`) and fails 0.6, whole table each time
    for c in cases.values():
        n = len(oracle.global_filter(c.nn_idx, c.nn_dist, c.img_idx, c.local_idx, c.ratio))
        if c.k == 1 or c.name == "d0_eq_d1":
            assert n == 0, c.name
        elif c.name == "d0_eq_d1_ratio1":
            assert n == len(c.img_idx)
        else:
            assert 0 < n < len(c.img_idx), c.name


def test_normalize_rows_cover_their_arms():
    x = gc.normalize_rows()
    y = gc.normalize(x)
    assert x.shape == (300, 128) and not np.isnan(y).any()
    tiny = np.finfo(np.float32).tiny
    assert (~x.any(axis=1)).sum() >= 3
    assert ((np.abs(x) < tiny) & (x != 0)).all(axis=1).sum() >= 2          # rows of subnormal entries
    big = np.flatnonzero((x == np.float32(1e19)).all(axis=1))
    assert len(big) == 1 and not y[big[0]].any()                           # the sum overflows: the row normalises to zeros
    assert ((x == np.round(x)) & (x >= 0) & (x <= 255)).all(axis=1).sum() > 250
