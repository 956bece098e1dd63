"""Device uniform-N selection (DESIGN.md "Uniform-N selection") for SIFT, SURF and FAST against the CPU references cut by
tests/uniform_mirror.py.  Tolerances are those of the unselected device tests: SIFT 0 everywhere, SURF 0 except angle_deg <= 1e-3
degrees, FAST byte for byte.  The references are computed once per case and shared (strongest_cases, fast_strongest_cases)."""
import ctypes as C
import threading
from importlib import import_module

import numpy as np
import pytest

import fast_strongest_cases as fsc
import strongest_cases as sc
import strongest_mirror as stm
import surf_cases
import uniform_mirror as um
from test_fast_strongest_gpu import assert_equals_mirror as assert_equals_fast_mirror
from test_fast_strongest_gpu import inputs as fast_inputs
from test_fast_strongest_gpu import params as fast_strongest_params
from test_sift_params_gpu import assert_equals_oracle
from test_strongest_gpu import _all_sentinel, _covered, _scene
from test_surf_gpu import assert_matches_mirror
from util import fetch, place, same_bits, sentinel_buffer, to_planar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


@pytest.fixture(scope="module")
def capi(gpu):
    return gpu._capi


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def uni(inp, N, grid=None):
    inp = {k: v for k, v in inp.items() if k != "NumStrongest"}
    return {**inp, "NumUniform": N} if grid is None else {**inp, "NumUniform": N, "UniformGrid": grid}


def sift_want(name, N, grid):
    ref = sc.sift_reference(name)
    at = um.sift_keep(ref, sc.sift_image(name).shape, N, grid)
    return at, tuple(a[at] for a in ref)


def surf_want(name, N, grid):
    img, ref = sc.surf_reference(name)
    at = um.surf_keep(img, ref, sc.SURF_CASES[name][1], N, grid)
    return at, tuple(a[at] for a in ref)


def tie_N(strength, segment, cells):
    """The first N at which some cell's cut falls inside a tie: the last row it keeps and the first it drops have equal strength."""
    strength, segment = np.asarray(strength), np.asarray(segment)
    counts = np.bincount(segment, minlength=cells)
    for N in range(1, len(strength)):
        for k, n in enumerate(um.waterfill(counts, N)):
            s = np.sort(strength[segment == k].astype(np.float64))[::-1]
            if 0 < n < len(s) and s[n - 1] == s[n]:
                return N
    raise AssertionError("no cut inside a tie")


# ---- 1. the selection equals the mirror ------------------------------------------------------------------------------------
SIFT_SELECTIONS = [("120x160", N, g) for N in (1, 13, 100, 418, 419, 5000) for g in ((1, 1), (3, 5), (8, 8))] + \
                  [("97x131", 100, (8, 8)), ("37x37", 3, (32, 32))]


@pytest.mark.parametrize("name,N,grid", SIFT_SELECTIONS)
def test_sift_selection_equals_the_mirror(fm, name, N, grid):
    at, want = sift_want(name, N, grid)
    assert len(at) == min(N, sc.SIFT_CASES[name][4])
    assert_equals_oracle(fm.sift_extract(uni(sc.sift_input(name), N, grid), sc.sift_image(name), want_aux=True), want)


@pytest.mark.parametrize("grid", [(1, 1), (1, 2)])
def test_sift_selection_on_ties(fm, grid):
    """The twin patches fall into one cell (1 x 1) or one each (1 x 2); N is the first cut inside a tie of some cell."""
    d, loc, aux = sc.sift_reference("twin")
    py, px, (H, W) = um.sift_pixels(loc, sc.sift_image("twin").shape)
    seg = um.cell(py, px, H, W, grid)
    assert len(set(seg.tolist())) == grid[1]
    N = tie_N(aux[:, 2], seg, grid[0] * grid[1])
    at, want = sift_want("twin", N, grid)
    assert len(at) == N
    assert_equals_oracle(fm.sift_extract(uni(sc.sift_input("twin"), N, grid), sc.sift_image("twin"), want_aux=True), want)


SURF_SELECTIONS = [("97x131", N, (8, 8)) for N in (1, 10, 63, 64, 65)] + [("pairA", 146, (8, 8)), ("pairA", 58, (3, 5)), ("twin", 9, (1, 2)),
                                                                          ("twin", 5, (8, 8))]


@pytest.mark.parametrize("name,N,grid", SURF_SELECTIONS)
def test_surf_selection_equals_the_mirror(fm, name, N, grid):
    at, want = surf_want(name, N, grid)
    assert len(at) == min(N, sc.SURF_CASES[name][2])
    d, loc, aux = fm.surf_extract(uni(sc.surf_input(name), N, grid), sc.surf_reference(name)[0], want_aux=True)
    assert_matches_mirror(d, loc, aux, *want)


# 120x160: four levels; 200x300x3: eight levels, the coarse ones short (they hand quota down) and the last one empty; 96x131: scale 1.5;
# tiled1 / twinB1: a single level, tiled1 cut inside a class of equal R
FAST_SELECTIONS = [("120x160", 400, (8, 8)), ("120x160", 100, (3, 5)), ("120x160", 1515, (8, 8)), ("120x160", 3, (32, 32)),
                   ("200x300x3", 200, (8, 8)), ("96x131", 200, (8, 8)), ("tiled1", 100, (2, 3)), ("tiled1", 100, (1, 1)), ("twinB1", 60, (8, 8))]


@pytest.mark.parametrize("name,N,grid", FAST_SELECTIONS)
def test_fast_selection_equals_the_mirror(fm, name, N, grid):
    cand = fsc.candidates(name, True)
    md, mloc, maux = um.fast_pick(cand, N, grid)
    assert 0 < len(md) <= N and len(md) < len(cand[0])
    f, loc, aux = fm.fast_extract(uni(fast_inputs(name), N, grid), fsc.spec(name)[0], want_aux=True)
    assert_equals_fast_mirror(f.Features, loc, aux, md, mloc, maux)


def test_fast_levels_hand_quota_down_and_one_is_empty():
    """The case behind ("200x300x3", 200): a short coarse level hands quota to the finer ones and the last level is empty (device-free)."""
    import fast_strongest_mirror as smir

    cand = fsc.candidates("200x300x3", True)
    M_l = np.bincount(cand[2][:, 2].astype(np.int64), minlength=len(cand[4])).tolist()
    q = smir.quotas(cand[4], 200)
    k = smir.kept_per_level(M_l, q, 200)
    assert M_l[-1] == 0 and any(m < ql for m, ql in zip(M_l, q)) and any(kl > ql for kl, ql in zip(k, q))


# ---- 2. invariants on the device's own results --------------------------------------------------------------------------------
def _extract(fm, det, name, extra=None):
    if det == "SIFT":
        inp, img = sc.sift_input(name), sc.sift_image(name)
    elif det == "SURF":
        inp, img = sc.surf_input(name), sc.surf_reference(name)[0]
    else:
        inp, img = fast_inputs(name), fsc.spec(name)[0]
    out = fm.extract_features({**inp, **(extra or {})}, img, want_aux=True)
    return (out[0].Features if det == "FAST" else out[0],) + tuple(out[1:])


def _rows_of(full, got, cols):
    """Indices of got's rows in full, by (location, aux[:, cols]) - unique per row - which must ascend."""
    key = lambda loc, aux: [tuple(u8(l).tolist()) + tuple(u8(a[cols]).tolist()) for l, a in zip(loc, aux)]  # noqa: E731
    index = {k: i for i, k in enumerate(key(full[1], full[2]))}
    assert len(index) == len(full[1])
    at = np.array([index[k] for k in key(got[1], got[2])], np.int64)
    assert (np.diff(at) > 0).all()
    return at


@pytest.mark.parametrize("det,name,N", [("SIFT", "120x160", 100), ("SURF", "pairA", 146), ("FAST", "120x160", 400)])
def test_invariants_of_the_device_result(fm, det, name, N):
    full = _extract(fm, det, name)
    got = _extract(fm, det, name, {"NumUniform": N})
    cols = slice(0, 3) if det == "FAST" else slice(0, 4)   # (FAST: aux[3] is 0 without selection, f32(R) with it)
    at = _rows_of(full, got, cols)
    assert 0 < len(at) <= N < len(full[0])
    assert np.array_equal(u8(got[0]), u8(full[0][at])) and np.array_equal(u8(got[1]), u8(full[1][at]))
    assert np.array_equal(u8(got[2][:, cols]), u8(full[2][at][:, cols]))
    # a 1 x 1 grid is the strongest-N result, every byte
    one, strongest = _extract(fm, det, name, {"NumUniform": N, "UniformGrid": (1, 1)}), _extract(fm, det, name, {"NumStrongest": N})
    assert all(a.shape == b.shape and np.array_equal(u8(a), u8(b)) for a, b in zip(one, strongest))
    # N >= candidates is the unselected result
    for big in (len(full[0]), 5000):
        same = _extract(fm, det, name, {"NumUniform": big})
        assert np.array_equal(u8(same[0]), u8(full[0])) and np.array_equal(u8(same[1]), u8(full[1]))
        assert np.array_equal(u8(same[2][:, cols]), u8(full[2][:, cols]))
    if det == "FAST":   # the rows per level are the strongest call's
        assert np.array_equal(np.bincount(got[2][:, 2].astype(int), minlength=4), np.bincount(strongest[2][:, 2].astype(int), minlength=4))
    if det == "SURF":   # pairA at N = 146: 64 cells occupied against the strongest call's 55
        img = sc.surf_reference(name)[0]
        py, px, (H, W), _ = um.surf_pixels(img, 1000.0)
        seg = um.cell(py, px, H, W, (8, 8))
        assert int((um.occupancy(seg, at, 64) > 0).sum()) == 64
        assert int((um.occupancy(seg, _rows_of(full, strongest, cols), 64) > 0).sum()) == 55


# ---- 3. the quota kernel against aps_uniform_quota ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,grid", [(146, (8, 8)), (58, (8, 8)), (300, (3, 5)), (583, (32, 32)), (40, (32, 32))])
def test_device_occupancy_is_the_host_quota(fm, capi, N, grid):
    """The cells' shares in the device's result (quota kernel) equal aps_uniform_quota of the mirror's counts (the host statement)."""
    img = sc.surf_reference("pairA")[0]
    py, px, (H, W), _ = um.surf_pixels(img, 1000.0)
    cells = grid[0] * grid[1]
    seg = um.cell(py, px, H, W, grid)
    counts = np.ascontiguousarray(np.bincount(seg, minlength=cells), np.int64)
    keep = np.zeros(cells, np.int64)
    capi.check(capi.lib.aps_uniform_quota(capi.ptr(counts), cells, N, capi.ptr(keep)))
    full, got = _extract(fm, "SURF", "pairA"), _extract(fm, "SURF", "pairA", {"NumUniform": N, "UniformGrid": grid})
    assert np.array_equal(um.occupancy(seg, _rows_of(full, got, slice(0, 4)), cells), keep) and int(keep.sum()) == N


# ---- 4. the entries: capacity, count-only, padding, layouts, pointers ----------------------------------------------------------
RAW = {"SIFT": ("120x160", 100, 128, np.float32), "SURF": ("pairA", 146, 64, np.float32), "FAST": ("120x160", 400, 64, np.uint8)}
GRID = (8, 8)


def _raw(capi, det, cap, ldd, layout=None, ldl=None, where="host", with_out=True, img_layout=None, max_features=0):
    """The uniform entry of `det` into sentinel-filled outputs: desc cap x ldd (row-major) or width x ldd (column-major), loc 2 x ldl,
    aux cap x 4.  Returns (rc, count, desc, loc, aux) as those matrices."""
    import torch

    name, N, width, dtype = RAW[det]
    layout = capi.APS_ROWMAJOR if layout is None else layout
    if det == "SIFT":
        img = sc.sift_image(name)
        prm = capi.aps_sift_uniform_params(capi.aps_sift_strongest_params(capi.aps_sift_params(*sc.SIFT_DEFAULT, max_features), N), *GRID)
        entry = capi.lib.aps_sift_extract_uniform
    elif det == "SURF":
        img = sc.surf_reference(name)[0]
        prm = capi.aps_surf_uniform_params(capi.aps_surf_strongest_params(capi.aps_surf_params(1000.0, 8, 4, 0, max_features), N), *GRID)
        entry = capi.lib.aps_surf_extract_uniform
    else:
        img = fsc.spec(name)[0]
        prm = capi.aps_fast_uniform_params(fast_strongest_params(capi, name, N, max_features), *GRID)
        entry = capi.lib.aps_fast_extract_uniform
    h, w, ch = img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3
    src = np.array(img) if img_layout is None else to_planar(img)
    rows = max(cap, 1)
    ldl = rows if ldl is None else ldl
    outer = rows if layout == capi.APS_ROWMAJOR else width
    desc = place(sentinel_buffer(outer * ldd, dtype), where)
    loc = place(sentinel_buffer(2 * ldl, np.float64), where)
    aux = place(sentinel_buffer(4 * rows, np.float32), where)
    cnt = C.c_int64(-1)
    torch.cuda.synchronize()
    pd, pl, pa = (capi.ptr(desc), capi.ptr(loc), capi.ptr(aux)) if with_out else (None, None, None)
    rc = entry(capi.ptr(place(src, where)), h, w, ch, capi.APS_IMG_U8_HWC if img_layout is None else img_layout, C.byref(prm), pd, layout, ldd,
               pl, ldl, pa, cap, C.byref(cnt))
    capi.check(capi.lib.aps_synchronize())
    return rc, int(cnt.value), fetch(desc).reshape(outer, ldd), fetch(loc).reshape(2, ldl), fetch(aux).reshape(rows, 4)


def _want(det):
    name, N, _, _ = RAW[det]
    if det == "SIFT":
        return sift_want(name, N, GRID)[1]
    if det == "SURF":
        return surf_want(name, N, GRID)[1]
    return um.fast_pick(fsc.candidates(name, True), N, GRID)


def _assert_equals(det, got, want):
    got = tuple(np.ascontiguousarray(g) for g in got)
    if det == "SIFT":
        assert_equals_oracle(got, want)
    elif det == "SURF":
        assert_matches_mirror(*got, *want)
    else:
        assert_equals_fast_mirror(*got, *want)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("det", ["SIFT", "SURF", "FAST"])
def test_capacity_count_only_padding_and_column_major(capi, det, where):
    _, K, width, _ = RAW[det]
    want = _want(det)
    assert len(want[0]) == K
    rc, cnt, desc, loc, aux = _raw(capi, det, K, width, where=where)   # cap = rows kept suffices
    assert rc == 0 and cnt == K
    _assert_equals(det, (desc, loc.T, aux), want)
    for cap in (K - 1, 0):   # one less, and cap = 0: the count, nothing written
        rc, cnt, desc, loc, aux = _raw(capi, det, cap, width, where=where)
        assert rc == capi.APS_E_CAP and cnt == K and _all_sentinel(desc, loc, aux)
    rc, cnt, *_ = _raw(capi, det, K, width, with_out=False)   # desc = NULL counts
    assert cnt == K and rc == capi.APS_E_ARG
    cap = K + 3   # padding: ldd above the width, ldl above cap, cap above the count
    rc, cnt, desc, loc, aux = _raw(capi, det, cap, width + 16, ldl=cap + 5, where=where)
    assert rc == 0 and cnt == K
    _assert_equals(det, (desc[:K, :width], loc[:, :K].T, aux[:K]), want)
    assert _all_sentinel(desc[:, width:], desc[K:], loc[:, K:], aux[K:])
    ld = cap + 5   # column-major descriptors (FAST: the leading dimensions are at least cap)
    rc, cnt, desc, loc, aux = _raw(capi, det, cap, ld, layout=capi.APS_COLMAJOR, ldl=ld, where=where)
    assert rc == 0 and cnt == K and desc.shape == (width, ld)
    _assert_equals(det, (desc[:, :K].T, loc[:, :K].T, aux[:K]), want)
    assert _all_sentinel(desc[:, K:], loc[:, K:], aux[K:])


def test_max_features_keeps_its_meaning(capi):
    """SURF: a limit on the candidates (584), whatever is kept; FAST: a limit on the rows kept."""
    K = RAW["SURF"][1]
    rc, cnt, desc, loc, aux = _raw(capi, "SURF", K, 64, max_features=583)
    assert rc == capi.APS_E_CAP and cnt == 584 and b"max_features" in capi.lib.aps_last_error() and _all_sentinel(desc, loc, aux)
    rc, cnt, *_ = _raw(capi, "SURF", K, 64, max_features=584)
    assert rc == 0 and cnt == K
    K = RAW["FAST"][1]
    rc, cnt, *_ = _raw(capi, "FAST", K, 64, max_features=K - 1)
    assert rc == capi.APS_E_CAP and cnt == K
    rc, cnt, desc, loc, aux = _raw(capi, "FAST", K, 64, max_features=K)
    assert rc == 0 and cnt == K
    _assert_equals("FAST", (desc, loc.T, aux), _want("FAST"))


@pytest.mark.parametrize("det", ["SIFT", "SURF", "FAST"])
def test_resident_output_holds_N_rows_two_runs_and_four_threads_agree(fm, det):
    import torch

    name, N, width, _ = RAW[det]
    want = _want(det)
    if det == "FAST":
        inp, img = uni(fast_inputs(name), N), fsc.spec(name)[0]
    else:
        inp, img = (uni(sc.sift_input(name), N), sc.sift_image(name)) if det == "SIFT" else (uni(sc.surf_input(name), N), sc.surf_reference(name)[0])
    extract = {"SIFT": fm.sift_extract, "SURF": fm.surf_extract, "FAST": fm.fast_extract}[det]
    dimg = torch.from_numpy(np.array(img)).cuda()
    torch.cuda.synchronize()
    f, pts = extract(inp, dimg, device_out=True, points_device=True)
    t = f.Features if det == "FAST" else f
    assert t.is_cuda and pts.is_cuda and tuple(t.shape) == (N, width)
    assert t.untyped_storage().nbytes() <= N * 128 * 4, "the descriptor tensor's storage holds more than N rows"
    ref = extract(inp, img, want_aux=True)
    ref = (ref[0].Features if det == "FAST" else ref[0],) + tuple(ref[1:])
    _assert_equals(det, ref, want)
    assert np.array_equal(u8(t.cpu().numpy()), u8(ref[0])) and np.array_equal(u8(pts.cpu().numpy()), u8(ref[1]))
    got = [None] * 4

    def work(k):
        out = extract(inp, img, want_aux=True)
        got[k] = (out[0].Features if det == "FAST" else out[0],) + tuple(out[1:])

    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for g in got:
        assert g is not None and all(np.array_equal(u8(a), u8(b)) for a, b in zip(ref, g))


# ---- 5. layouts -----------------------------------------------------------------------------------------------------------------
def test_matlab_layouts_give_the_same_rows(capi):
    """aps_sift_extract_uniform with a planar column-major image and column-major descriptors, the layouts a MATLAB gateway has."""
    _, K, width, _ = RAW["SIFT"]
    rc, cnt, desc, loc, aux = _raw(capi, "SIFT", K, K, layout=capi.APS_COLMAJOR, img_layout=capi.APS_IMG_U8_MATLAB)
    assert rc == 0 and cnt == K
    rc, cnt, rdesc, rloc, raux = _raw(capi, "SIFT", K, width)
    assert rc == 0 and same_bits(desc.T, rdesc) and same_bits(loc, rloc) and same_bits(aux, raux)
    assert_equals_oracle((rdesc, np.ascontiguousarray(rloc.T), raux), _want("SIFT"))


# ---- 6. every host entry returns the same rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", ["SIFT", "SURF", "FAST"])
def test_host_entries_return_the_same_rows(gpu, fm, det):
    import torch

    pl = import_module(gpu.__name__ + ".pipeline")
    name, N, width, _ = RAW[det]
    want = _want(det)
    if det == "FAST":
        inp, img = uni(fast_inputs(name), N), fsc.spec(name)[0]
    else:
        inp, img = (uni(sc.sift_input(name), N), sc.sift_image(name)) if det == "SIFT" else (uni(sc.surf_input(name), N), sc.surf_reference(name)[0])

    def check(d, p):
        d = d.Features if hasattr(d, "Features") else d
        d = (d.cpu().numpy() if hasattr(d, "cpu") else np.asarray(d))[:, :width]
        p = p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p)
        assert d.shape == (N, width)
        if det == "SIFT":
            assert_equals_oracle((d, p), want)
        elif det == "SURF":
            assert_matches_mirror(np.ascontiguousarray(d), p, want[2], *want)
        else:
            assert np.array_equal(d, want[0]) and np.array_equal(u8(p), u8(want[1]))

    for entry in (fm.getFeaturePoints, fm.extract_features):
        check(*entry(inp, img))
    rgb = np.array(img if img.ndim == 3 else np.repeat(img[:, :, None], 3, 2))   # (a gray triple's gray plane is the gray value)
    dimgs = [torch.from_numpy(rgb).cuda() for _ in range(3)]   # three views: the worker streams
    torch.cuda.synchronize()
    descs, kps = pl.extract_features(pl.default_input(**inp), dimgs)
    for d, p in zip(descs, kps):
        check(d, p)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------
E2E_N = 800


def test_sift_stitch_with_800_uniform_rows_per_view(gpu):
    pl = import_module(gpu.__name__ + ".pipeline")
    cams, views = _scene(gpu)
    inp = pl.default_input(bands=3, NumUniform=E2E_N)
    panos, info = pl.stitch(inp, [views[i] for i in range(6)], Ks=[c["K"] for c in cams], tile=(512, 512))
    print("n_features", list(info["n_features"]), "components", info["n_components"], "verified", info["n_pairs_verified"])
    assert list(info["n_features"]) == [E2E_N] * 6
    assert info["n_components"] == 1 and len(panos) == 1 and sorted(info["components"][0]["members"]) == list(range(6))
    assert info["n_pairs_verified"] >= 5
    assert _covered(panos[0]) > 0.5


def test_sift_stitch_distributed_with_800_uniform_rows_per_view(gpu):
    pl = import_module(gpu.__name__ + ".pipeline")
    par = import_module(gpu.__name__ + ".parallel")
    cams, views = _scene(gpu)
    inp = pl.default_input(bands=3, NumUniform=E2E_N)
    pano, info = par.stitch_distributed(inp, views, 6, [c["K"] for c in cams], (512, 512), 0, None, pano_root=0)
    print("n_features", [int(v) for v in info["n_features"]], "components", info["n_components"], "pairs", len(info["pairs"]))
    assert [int(v) for v in info["n_features"]] == [E2E_N] * 6
    assert info["n_components"] == 1 and sorted(info["members"]) == list(range(6))
    assert len(info["pairs"]) >= 5
    assert _covered(pano) > 0.5


def test_surf_pair_is_verified_with_200_uniform_rows(gpu):
    """surf_cases.pair() cut to 200 uniform rows per image: the pair is verified, and the model maps A's corners to within 1 px of
    PAIR_H.  On the mirror: 112 ratio matches at N = 200, all within 1.5 px of PAIR_H (the strongest 200 give 138)."""
    import torch

    pl = import_module(gpu.__name__ + ".pipeline")
    A, B = surf_cases.pair()
    rgb = lambda g: torch.from_numpy(np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))).cuda()  # noqa: E731
    inp = pl.default_input(detector="SURF", NumUniform=200)
    descs, kps = pl.extract_features(inp, [rgb(A), rgb(B)])
    assert [len(k) for k in kps] == [200, 200]
    res = pl.match_and_verify(inp, descs, kps, 0)
    assert res["pairs"] == [(0, 1)]
    H = np.linalg.inv(np.asarray(res["models"][0], np.float64))   # models map j -> i (B -> A), 1-based points; PAIR_H maps A -> B, 0-based
    h, w = A.shape
    for x, y in ((0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0)):
        p = H @ np.array([x + 1.0, y + 1.0, 1.0])
        q = surf_cases.PAIR_H @ np.array([x, y, 1.0])
        err = float(np.hypot(p[0] / p[2] - 1.0 - q[0] / q[2], p[1] / p[2] - 1.0 - q[1] / q[2]))
        print("corner (%g, %g): %.4f px" % (x, y, err))
        assert err <= 1.0


def test_fast_stitch_with_600_uniform_rows_runs_end_to_end(gpu):
    """The twin pair of test_fast_strongest_gpu.py's stitch, with its intrinsics: A has 4673 candidates and B 1202, and the mirror
    keeps 600 rows of each (the rows per level are the strongest call's).  The stitch ends with a non-empty panorama.  (The 3 x 2
    synthetic scene of the SIFT tests is no FAST case: its smooth views gave 0 FAST rows at the default MinContrast.)"""
    import fast_pyramid_cases as pc
    from test_fast_strongest_gpu import rgb

    pl = import_module(gpu.__name__ + ".pipeline")
    A, B = pc.twin_images()
    assert pc.TWIN_LEVELS == 3
    inp = pl.default_input(detector="FAST", NumLevels=3, NumUniform=600, MinContrast=pc.TWIN_MC, Matchingthreshold=20, resizeImage=0)
    f = 450.0   # B is A seen at 167 / 240 of the focal length, same direction
    Ks = [np.array([[f * s, 0, w / 2.0], [0, f * s, h / 2.0], [0, 0, 1.0]]) for (h, w), s in ((A.shape, 1.0), (B.shape, 167.0 / 240.0))]
    panos, info = pl.stitch(inp, [rgb(A), rgb(B)], Ks=Ks, tile=(512, 512))
    print("n_features", list(info["n_features"]), "components", info["n_components"])
    assert list(info["n_features"]) == [600, 600] and len(panos) >= 1
    pano = panos[0].cpu().numpy() if hasattr(panos[0], "cpu") else np.asarray(panos[0])
    assert pano.ndim == 3 and (pano.max(axis=2) > 0).any()
