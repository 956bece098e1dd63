"""GPU tests of the grouped SIFT selections (aps_sift_extract_batch_strongest, aps_sift_extract_batch_uniform): the rows of every
view of a group are, bit for bit, those of the single-view call (aps_sift_extract_strongest / aps_sift_extract_uniform, which
test_strongest_gpu.py and test_uniform_gpu.py hold to the mirrors) on that view, whatever the other views contain.  Images: the
97 x 131 and 35 x 47 views of test_sift_batch_gpu.py (252-285 and 22-28 rows), the 97 x 131 case of strongest_cases.py (281 rows,
cuts inside an orientation tie at N = 4, 7, 8) and a flat view without rows.  The single-view results are computed once per
(image, selection) and shared."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import strongest_cases as sc
import strongest_mirror as stm
import uniform_mirror as um
from test_sift_batch_gpu import INPUT, ref, same, view
from util import fetch, place, same_bits, sentinel_buffer

pytestmark = pytest.mark.gpu

H, W = 97, 131
KINDS = [("strongest", None), ("uniform", (8, 8))]
KIND_IDS = ["strongest", "uniform8x8"]
_IMG, _SINGLE = {}, {}


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def image(key):
    """key: (k, h, w) - view k of test_sift_batch_gpu.py; "flat"; "case" - strongest_cases' 97 x 131 image"""
    if key not in _IMG:
        _IMG[key] = np.full((H, W, 3), 128, np.uint8) if key == "flat" else np.array(sc.sift_image("97x131")) if key == "case" else view(*key)
    return _IMG[key]


def v97(k):
    return (k, H, W)


def inputs(kind, N, grid=None):
    if kind == "strongest":
        return dict(INPUT, NumStrongest=N)
    return dict(INPUT, NumUniform=N) if grid is None else dict(INPUT, NumUniform=N, UniformGrid=grid)


def single(fm, key, kind=None, N=None, grid=None):
    """The single-view call on the image (kind None: without selection), computed once."""
    ck = (key, kind, N, grid)
    if ck not in _SINGLE:
        _SINGLE[ck] = fm.sift_extract(INPUT if kind is None else inputs(kind, N, grid), image(key), want_aux=True)
    return _SINGLE[ck]


def rows_of(fm, keys):
    return [len(single(fm, k)[0]) for k in keys]


def check_group(fm, keys, kind, N, grid=None):
    got = fm.sift_extract_batch(inputs(kind, N, grid), [image(k) for k in keys], want_aux=True)
    assert len(got) == len(keys)
    for v, (k, g) in enumerate(zip(keys, got)):
        want = single(fm, k, kind, N, grid)
        assert len(want[0]) == min(N, len(single(fm, k)[0]))
        assert same(g, want), f"view {v} ({k}) differs from its single-view call"
    return got


# ---- 1. groups against the single-view calls -----------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [1, 2, 3, 16])
@pytest.mark.parametrize("kind,grid", KINDS, ids=KIND_IDS)
def test_groups_of_1_2_3_and_16_views(fm, kind, grid, g):
    """(16 views: group index 15, the top of the 4-bit field.)  Every view is cut, and the views' row ranges do not end on the
    64-row words of the group's bitmap."""
    keys = [v97(k) for k in range(g)]
    counts = rows_of(fm, keys)
    assert min(counts) > 100
    if g > 1:
        assert any(int(e) % 64 != 0 for e in np.cumsum(counts)[:-1])
    got = check_group(fm, keys, kind, 100, grid)
    assert [len(r[0]) for r in got] == [100] * g


@pytest.mark.parametrize("pos", [0, 1, 2])
@pytest.mark.parametrize("kind,grid", KINDS, ids=KIND_IDS)
def test_flat_view_first_in_the_middle_and_last(fm, kind, grid, pos):
    keys = [v97(0), v97(2)]
    assert len(set(rows_of(fm, keys))) == 2   # views of different row counts
    keys.insert(pos, "flat")
    got = check_group(fm, keys, kind, 100, grid)
    assert [len(r[0]) for r in got] == [0 if k == "flat" else 100 for k in keys]
    assert got[pos][0].shape == (0, 128) and got[pos][1].shape == (0, 2)


@pytest.mark.parametrize("N", [1, 4, 7, 8])
@pytest.mark.parametrize("kind,grid", KINDS + [("uniform", (1, 1))], ids=KIND_IDS + ["uniform1x1"])
def test_one_row_and_cuts_inside_an_orientation_tie(fm, kind, grid, N):
    """N = 4, 7, 8 fall inside the tie of one keypoint's orientations on strongest_cases' 97 x 131 image (the middle view)."""
    assert N == 1 or N in sc.SIFT_TIE_CUTS["97x131"]
    ref_case = sc.sift_reference("97x131")
    if N > 1:
        assert N in stm.tie_cuts(ref_case[2], ref_case[1], cross=False)
    got = check_group(fm, [v97(0), "case", v97(2)], kind, N, grid)
    assert [len(r[0]) for r in got] == [N] * 3
    if kind == "strongest":
        assert same(got[1], stm.pick(ref_case, N))


@pytest.mark.parametrize("kind,grid", KINDS, ids=KIND_IDS)
def test_some_views_are_cut_and_others_not(fm, kind, grid):
    keys = [v97(0), v97(1), "flat", v97(2), v97(3)]
    counts = rows_of(fm, keys)
    lo, hi = min(c for c in counts if c), max(counts)
    N = (lo + hi) // 2
    assert lo < N < hi
    got = check_group(fm, keys, kind, N, grid)
    assert [len(r[0]) for r in got] == [min(c, N) for c in counts]
    assert any(c < N for c in counts if c) and any(c > N for c in counts)


@pytest.mark.parametrize("kind,grid", KINDS, ids=KIND_IDS)
def test_nothing_cut_is_the_unselected_batch(fm, kind, grid):
    keys = [v97(0), "flat", v97(1), v97(2)]
    plain = fm.sift_extract_batch(INPUT, [image(k) for k in keys], want_aux=True)
    for N in (max(rows_of(fm, keys)), 5000):
        got = check_group(fm, keys, kind, N, grid)
        assert all(same(g, p) for g, p in zip(got, plain))


def test_grid_1x1_is_the_strongest_group(fm):
    keys = [v97(0), v97(1), v97(2)]
    one = check_group(fm, keys, "uniform", 100, (1, 1))
    strongest = check_group(fm, keys, "strongest", 100)
    assert all(same(a, b) for a, b in zip(one, strongest))


def test_grid_32x32_at_16_views(fm):
    """view 15's last cell is segment 16 * 1024 - 1, the top of the 14-bit segment field"""
    got = check_group(fm, [v97(k) for k in range(16)], "uniform", 100, (32, 32))
    assert [len(r[0]) for r in got] == [100] * 16


@pytest.mark.parametrize("kind,grid", KINDS + [("uniform", (32, 32))], ids=KIND_IDS + ["uniform32x32"])
def test_small_views(fm, kind, grid):
    keys = [(k, 35, 47) for k in range(3)]
    counts = rows_of(fm, keys)
    assert min(counts) >= 20
    got = check_group(fm, keys, kind, 10, grid)
    assert [len(r[0]) for r in got] == [10] * 3


def test_two_runs_give_the_same_bytes(fm):
    keys = [v97(0), "flat", v97(1)]
    for kind, grid in KINDS:
        a, b = check_group(fm, keys, kind, 100, grid), check_group(fm, keys, kind, 100, grid)
        assert all(same(x, y) for x, y in zip(a, b))


# ---- 2. one group per selection against the mirrors ------------------------------------------------------------------------------
def test_strongest_group_equals_the_mirror(fm):
    got = fm.sift_extract_batch(inputs("strongest", 100), [image(v97(k)) for k in range(3)], want_aux=True)
    for k in range(3):
        assert same(got[k], stm.pick(ref(k, H, W), 100)), f"view {k}"


def test_uniform_group_equals_the_mirror(fm):
    got = fm.sift_extract_batch(inputs("uniform", 100, (8, 8)), [image(v97(k)) for k in range(3)], want_aux=True)
    for k in range(3):
        full = ref(k, H, W)
        at = um.sift_keep(full, (H, W), 100, (8, 8))
        assert len(at) == 100 and same(got[k], tuple(a[at] for a in full)), f"view {k}"


# ---- 3. the entries: capacity, count-only, padding, layouts, pointers ------------------------------------------------------------
def call_sel(capi, kind, grid, keys, caps, N, layout=None, ldd=128, ldl=None, where="host", with_out=True):
    """The C entry into sentinel-filled outputs, one set per view: desc cap x ldd (row-major) or 128 x ldd (column-major), loc
    2 x ldl, aux cap x 4.  Returns (rc, counts, [(desc, loc, aux)]) as those matrices."""
    import torch

    layout = capi.APS_ROWMAJOR if layout is None else layout
    rows = [max(c, 1) for c in caps]
    ldl = max(rows) if ldl is None else ldl
    st = capi.aps_sift_strongest_params(capi.aps_sift_params(*sc.SIFT_DEFAULT, 0), N)
    if kind == "strongest":
        prm, entry = st, capi.lib.aps_sift_extract_batch_strongest
    else:
        prm, entry = capi.aps_sift_uniform_params(st, *grid), capi.lib.aps_sift_extract_batch_uniform
    outer = [r if layout == capi.APS_ROWMAJOR else 128 for r in rows]
    src = [place(np.ascontiguousarray(image(k)), where) for k in keys]
    descs = [place(sentinel_buffer(o * ldd, np.float32), where) for o in outer]
    locs = [place(sentinel_buffer(2 * ldl, np.float64), where) for _ in rows]
    auxs = [place(sentinel_buffer(4 * r, np.float32), where) for r in rows]
    views = (capi.aps_sift_view * len(keys))()
    for v in range(len(keys)):
        views[v].img = capi.ptr(src[v])
        if with_out:
            views[v].desc, views[v].loc, views[v].aux = capi.ptr(descs[v]), capi.ptr(locs[v]), capi.ptr(auxs[v])
        views[v].cap, views[v].count = caps[v], -1
    torch.cuda.synchronize()
    rc = entry(views, len(keys), H, W, 3, capi.APS_IMG_U8_HWC, C.byref(prm), layout, ldd, ldl)
    capi.check(capi.lib.aps_synchronize())
    out = [(fetch(descs[v]).reshape(outer[v], ldd), fetch(locs[v]).reshape(2, ldl), fetch(auxs[v]).reshape(rows[v], 4))
           for v in range(len(keys))]
    return rc, [int(views[v].count) for v in range(len(keys))], out


def all_sentinel(*arrays):
    return all(same_bits(a.reshape(-1), sentinel_buffer(a.size, a.dtype)) for a in (np.ascontiguousarray(x) for x in arrays))


RAW_KEYS = [v97(0), "flat", v97(1), v97(2)]
RAW_N = 100
RAW_COUNTS = [100, 0, 100, 100]


@pytest.mark.parametrize("kind,grid", KINDS, ids=KIND_IDS)
def test_capacity_and_count_only(gpu, fm, kind, grid):
    capi = gpu._capi
    want = [single(fm, k, kind, RAW_N, grid) for k in RAW_KEYS]
    rc, counts, out = call_sel(capi, kind, grid, RAW_KEYS, [RAW_N] * 4, RAW_N)   # cap = N exactly
    assert rc == 0 and counts == RAW_COUNTS
    for (d, l, a), c, w in zip(out, counts, want):
        assert same((d[:c], np.ascontiguousarray(l[:, :c].T), a[:c]), w)
    caps = [RAW_N, RAW_N, RAW_N - 1, RAW_N]   # one row short on one view only: every count, nothing written anywhere
    rc, counts, out = call_sel(capi, kind, grid, RAW_KEYS, caps, RAW_N)
    assert rc == capi.APS_E_CAP and counts == RAW_COUNTS
    assert all(all_sentinel(*o) for o in out)
    rc, counts, out = call_sel(capi, kind, grid, RAW_KEYS, [0] * 4, RAW_N, with_out=False)   # count-only: no room, no outputs
    assert rc == capi.APS_E_CAP and counts == RAW_COUNTS
    rc, counts, out = call_sel(capi, kind, grid, RAW_KEYS, [0] * 4, RAW_N)
    assert rc == capi.APS_E_CAP and counts == RAW_COUNTS and all(all_sentinel(*o) for o in out)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("kind,grid", KINDS, ids=KIND_IDS)
def test_padding_column_major_host_and_device(gpu, fm, kind, grid, where):
    capi = gpu._capi
    want = [single(fm, k, kind, RAW_N, grid) for k in RAW_KEYS]
    cap = RAW_N + 3   # row-major: ldd above 128, ldl above cap, cap above the count
    rc, counts, out = call_sel(capi, kind, grid, RAW_KEYS, [cap] * 4, RAW_N, ldd=144, ldl=cap + 5, where=where)
    assert rc == 0 and counts == RAW_COUNTS
    for (d, l, a), c, w in zip(out, counts, want):
        assert same((np.ascontiguousarray(d[:c, :128]), np.ascontiguousarray(l[:, :c].T), a[:c]), w)
        assert all_sentinel(d[:, 128:], d[c:], l[:, c:], a[c:])
    ld = cap + 5   # column-major descriptors
    rc, counts, out = call_sel(capi, kind, grid, RAW_KEYS, [cap] * 4, RAW_N, layout=capi.APS_COLMAJOR, ldd=ld, ldl=ld, where=where)
    assert rc == 0 and counts == RAW_COUNTS
    for (d, l, a), c, w in zip(out, counts, want):
        assert d.shape == (128, ld)
        assert same((np.ascontiguousarray(d[:, :c].T), np.ascontiguousarray(l[:, :c].T), a[:c]), w)
        assert all_sentinel(d[:, c:], l[:, c:], a[c:])


# ---- 4. the pipeline sends resident views with a selection in groups --------------------------------------------------------------
@pytest.mark.parametrize("keys", [{"NumStrongest": 100}, {"NumUniform": 20}], ids=["strongest", "uniform"])
def test_sift_submit_groups_views_with_a_selection(gpu, fm, monkeypatch, keys):
    """5 views of 97 x 131, then 2 of 35 x 47: two calls of fm.sift_extract_batch, and every view's rows are fm.sift_extract's."""
    import torch

    pl = import_module(gpu.__name__ + ".pipeline")
    imgs = [image(v97(k)) for k in range(5)] + [image((k, 35, 47)) for k in range(2)]
    timgs = [torch.from_numpy(im).cuda() for im in imgs]
    torch.cuda.synchronize()
    inp = dict(INPUT, **keys)
    calls, batch = [], fm.sift_extract_batch

    def counted(input, images, **kw):
        calls.append((dict(input), len(images)))
        return batch(input, images, **kw)

    monkeypatch.setattr(fm, "sift_extract_batch", counted)
    got = [f.result() for f in pl.sift_submit(inp, timgs)]
    monkeypatch.undo()
    assert sorted(n for _, n in calls) == [2, 5] and all(set(keys) <= set(i) for i, _ in calls)
    N = next(iter(keys.values()))
    for k, t in enumerate(timgs):
        d, pts = fm.sift_extract(inp, t, device_out=True)
        assert len(pts) == min(N, len(fm.sift_extract(INPUT, imgs[k])[1])) and len(pts) > 0
        assert got[k][0].is_cuda and torch.equal(got[k][0], d) and np.array_equal(np.asarray(got[k][1]), pts)
