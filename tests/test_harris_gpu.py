"""Device Harris corners (input.CornerMethod = 'Harris': aps_corner_extract, aps_corner_extract_batch, aps_harris_planes) against the
NumPy mirror of the contract (tests/harris_mirror.py) on tests/harris_cases.py: dense response, count, locations as f64 bits, aux and
every descriptor byte equal - integer arithmetic throughout, so there is no tolerance anywhere.  Then corner = APS_CORNER_FAST
through the new entries against the existing ones, byte for byte, and one stitch."""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest

import fast_cases as fc
import fast_pyramid_mirror as pmir
import fast_strongest_mirror as smir
import harris_cases as hc
import harris_mirror as hm
import uniform_mirror as umir

pytestmark = pytest.mark.gpu

FILL = 0xA5
WIDTH = {"FREAK": 64, "ORB": 32}
S12 = (1200000, 1000000)


def frozen(t):
    for a in t:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def mirror(name, descriptor):
    """The mirror's (desc, loc, aux, R, shapes) of a case, computed once and shared (read-only)."""
    c = hc.CASES[name]
    return frozen(hm.candidates(hc.image(name), fc.tables(), descriptor, c.levels, c.scale, c.quality))


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pyramid_params(capi, name=None, quality=None, levels=None, scale=None, threshold=0, max_features=0):
    c = hc.CASES[name] if name else None
    qn, qd = hm.quality_rational(c.quality if quality is None else quality)
    num, den = pmir.scale_rational(c.scale if scale is None else scale)
    return capi.aps_fast_pyramid_params(capi.aps_fast_params(threshold, qn, qd, max_features), c.levels if levels is None else levels, num, den)


def corner_params(capi, pyramid, descriptor="FREAK", corner=None, select=0, n_select=0, rows=0, cols=0):
    chain = capi.aps_fast_orb_params(pyramid, select, n_select, rows, cols)
    return capi.aps_corner_params(chain, capi.APS_CORNER_HARRIS if corner is None else corner,
                                  capi.APS_DESC_ORB if descriptor == "ORB" else capi.APS_DESC_FREAK)


def call(gpu, entry, prm, img, cap, width, colmajor=False, ldd=None, ldl=None, device=False, with_out=True):
    """A single-view entry on FILL-ed outputs of max(cap, 1) rows: (rc, count, desc, loc, aux) as numpy."""
    capi = gpu._capi
    h, w, ch = img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3
    img = np.ascontiguousarray(img)
    rows = max(cap, 1)
    ldd = (rows if colmajor else width) if ldd is None else ldd
    ldl = rows if ldl is None else ldl
    desc = np.full((width, ldd) if colmajor else (rows, ldd), FILL, np.uint8)
    loc = np.full((2, ldl), -7.5, np.float64)
    aux = np.full((rows, 4), -7.5, np.float32)
    cnt = C.c_int64(-1)
    args = [img, desc, loc, aux]
    if device:
        import torch

        args = [torch.from_numpy(a.copy()).cuda() for a in args]
        torch.cuda.synchronize()
    pi, pd, pl, pa = [capi.ptr(a) for a in args]
    if not with_out:
        pd = pl = pa = None
    rc = getattr(capi.lib, entry)(pi, h, w, ch, capi.APS_IMG_U8_HWC, C.byref(prm), pd, capi.APS_COLMAJOR if colmajor else capi.APS_ROWMAJOR,
                                  ldd, pl, ldl, pa, cap, C.byref(cnt))
    if device:
        capi.check(capi.lib.aps_synchronize())
        desc, loc, aux = [a.cpu().numpy() for a in args[1:]]
    return rc, cnt.value, desc, loc, aux


def rows_of(desc, loc, aux, n, width, colmajor=False):
    return (np.ascontiguousarray(desc[:, :n].T) if colmajor else desc[:n, :width]), np.ascontiguousarray(loc[:, :n].T), aux[:n]


def assert_rows(got, want, what=""):
    (d, loc, aux), (md, mloc, maux) = got, want
    assert d.shape == md.shape and loc.shape == mloc.shape and aux.shape == maux.shape, (what, d.shape, md.shape)
    assert np.array_equal(aux[:, 2], maux[:, 2]), (what, "levels")
    assert np.array_equal(u64(loc), u64(mloc)), (what, "locations / order")
    assert np.array_equal(u32(aux[:, 0]), u32(maux[:, 0])), (what, "f32(R)")
    assert np.array_equal(aux[:, 1], maux[:, 1]), (what, "orientation bins")
    assert np.array_equal(u32(aux[:, 3]), u32(maux[:, 3])), (what, "aux[3]")
    assert np.array_equal(d, md), (what, "descriptor bytes (%d rows differ)" % int((d != md).any(1).sum()))


def harris_planes(gpu, img, pyr, device=False):
    capi = gpu._capi
    h, w = img.shape[:2]
    cnt = C.c_int64(-1)
    capi.check(capi.lib.aps_harris_planes(capi.ptr(img), h, w, 1, capi.APS_IMG_U8_HWC, C.byref(pyr), None, 0, C.byref(cnt)))
    out = np.full(cnt.value, -3, np.int64)
    if device:
        import torch

        t = torch.from_numpy(out.copy()).cuda()
        capi.check(capi.lib.aps_harris_planes(capi.ptr(img), h, w, 1, capi.APS_IMG_U8_HWC, C.byref(pyr), capi.ptr(t), cnt.value, C.byref(cnt)))
        capi.check(capi.lib.aps_synchronize())
        return t.cpu().numpy()
    capi.check(capi.lib.aps_harris_planes(capi.ptr(img), h, w, 1, capi.APS_IMG_U8_HWC, C.byref(pyr), capi.ptr(out), cnt.value, C.byref(cnt)))
    return out


# ---- the response, then the rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hc.CASES))
def test_dense_response_equals_mirror(gpu, name):
    c = hc.CASES[name]
    img = np.ascontiguousarray(hc.image(name))
    want = hm.dense_planes(img, c.levels, c.scale, hc.MARGIN)
    got = harris_planes(gpu, img, pyramid_params(gpu._capi, name), device=name == "pyramid")
    assert got.shape == want.shape and np.array_equal(got, want), "%d pixels differ" % int((got != want).sum())


@pytest.mark.parametrize("descriptor", ["FREAK", "ORB"])
@pytest.mark.parametrize("name", list(hc.CASES))
def test_rows_equal_mirror(gpu, name, descriptor):
    md, mloc, maux, R, _ = mirror(name, descriptor)
    n, width = len(md), WIDTH[descriptor]
    assert n >= hc.CASES[name].min_rows
    prm = corner_params(gpu._capi, pyramid_params(gpu._capi, name), descriptor)
    rc, cnt, desc, loc, aux = call(gpu, "aps_corner_extract", prm, hc.image(name), n, width)
    assert rc == 0 and cnt == n
    if n:
        assert_rows(rows_of(desc, loc, aux, n, width), (md, mloc, maux), name)
    else:
        assert (desc == FILL).all() and (loc == -7.5).all() and (aux == -7.5).all()   # no rows, no error, nothing written


@pytest.mark.parametrize("descriptor", ["FREAK", "ORB"])
def test_layouts_pointers_and_the_capacity_protocol(gpu, descriptor):
    capi = gpu._capi
    name = "pyramid"
    md, mloc, maux, _, _ = mirror(name, descriptor)
    n, width, img = len(md), WIDTH[descriptor], hc.image(name)
    prm = corner_params(capi, pyramid_params(capi, name), descriptor)
    # count-only mode, then a second call with that capacity
    rc, cnt, desc, loc, aux = call(gpu, "aps_corner_extract", prm, img, 0, width)
    assert rc == capi.APS_E_CAP and cnt == n and (desc == FILL).all() and (loc == -7.5).all() and (aux == -7.5).all()
    rc, cnt, *_ = call(gpu, "aps_corner_extract", prm, img, n, width, with_out=False)
    assert cnt == n and rc == capi.APS_E_ARG   # features present and no output to put them in
    rc, cnt, desc, loc, aux = call(gpu, "aps_corner_extract", prm, img, n - 1, width)
    assert rc == capi.APS_E_CAP and cnt == n and (desc == FILL).all() and (loc == -7.5).all() and (aux == -7.5).all()   # nothing written
    rc, cnt, *_ = call(gpu, "aps_corner_extract", prm, img, n, width, ldd=width - 1)
    assert rc == capi.APS_E_DIM
    for colmajor in (False, True):
        for device in (False, True):
            cap = n + 5
            ldd = cap + 3 if colmajor else width + 7
            rc, cnt, desc, loc, aux = call(gpu, "aps_corner_extract", prm, img, cap, width, colmajor, ldd, cap + 2, device)
            assert rc == 0 and cnt == n
            assert_rows(rows_of(desc, loc, aux, n, width, colmajor), (md, mloc, maux), (colmajor, device))
            # the padding and the rows beyond the count stay the caller's
            if colmajor:
                assert (desc[:, n:] == FILL).all()
            else:
                assert (desc[:n, width:] == FILL).all() and (desc[n:] == FILL).all()
            assert (loc[:, n:] == -7.5).all() and (aux[n:] == -7.5).all()
    # max_features
    rc, cnt, desc, *_ = call(gpu, "aps_corner_extract", corner_params(capi, pyramid_params(capi, name, max_features=n - 1), descriptor), img, n, width)
    assert rc == capi.APS_E_CAP and cnt == n and (desc == FILL).all()
    rc, cnt, *_ = call(gpu, "aps_corner_extract", corner_params(capi, pyramid_params(capi, name, max_features=n), descriptor), img, n, width)
    assert rc == 0 and cnt == n


# ---- selections ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descriptor", ["FREAK", "ORB"])
def test_selections_equal_mirror(gpu, fm, descriptor):
    name = "pyramid"
    c = hc.CASES[name]
    cand = mirror(name, descriptor)
    md, mloc, maux, R, shapes = cand
    inp = {"detector": "FAST", "CornerMethod": "Harris", "DescriptorMethod": descriptor, "NumLevels": c.levels, "ScaleFactor": c.scale}
    f, loc, aux = fm.fast_extract(inp, hc.image(name), want_aux=True)   # MinQuality: the default 0.01 is the case's
    assert_rows((f.Features, loc, aux), (md, mloc, maux), "no selection")
    row_of = {(int(l), int(x), int(y)): i for i, (l, (x, y)) in enumerate(zip(maux[:, 2], u64(mloc)))}
    results = {}
    for key, N, grid in (("NumStrongest", 3, None), ("NumStrongest", len(md) + 7, None), ("NumStrongest", 11, None),
                         ("NumUniform", 11, (1, 1)), ("NumUniform", 11, (4, 4))):
        extra = {key: N, **({"UniformGrid": grid} if grid else {})}
        f, loc, aux = fm.fast_extract({**inp, **extra}, hc.image(name), want_aux=True)
        want = smir.pick(cand, N) if key == "NumStrongest" else umir.fast_pick(cand, N, grid)
        assert len(want[0]) == min(N, len(md))
        assert_rows((f.Features, loc, aux), want, extra)
        assert np.array_equal(u32(aux[:, 3]), u32(aux[:, 0]))   # both are f32(R)
        # the rows with a selection are rows of the call without it, in order
        idx = np.array([row_of[(int(l), int(x), int(y))] for l, (x, y) in zip(aux[:, 2], u64(loc))], np.int64)
        assert (np.diff(idx) > 0).all() and np.array_equal(f.Features, md[idx]) and np.array_equal(aux[:, :3], maux[idx, :3])
        results[key, N, grid] = (f.Features, loc, aux)
    for a, b in zip(results["NumStrongest", 11, None], results["NumUniform", 11, (1, 1)]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_dense_response_at_the_rows_is_the_strongest_calls_response(gpu, fm):
    """aps_harris_planes at the returned pixels = aux[:, 3] of the strongest call, whose R comes from fast_harris_kernel."""
    name = "pyramid"
    c = hc.CASES[name]
    img = np.ascontiguousarray(hc.image(name))
    planes = harris_planes(gpu, img, pyramid_params(gpu._capi, name))
    inp = {"detector": "FAST", "CornerMethod": "Harris", "NumLevels": c.levels, "ScaleFactor": c.scale, "NumStrongest": 1 << 20}
    f, loc, aux = fm.fast_extract(inp, img, want_aux=True)
    cand = mirror(name, "FREAK")
    shapes = cand[4]
    assert len(f) == len(cand[0]) >= 8
    py, px, level, _ = umir.fast_pixels((f.Features, loc, aux, None, shapes))
    start = np.concatenate([[0], np.cumsum([h * w for h, w in shapes])])
    widths = np.array([w for _, w in shapes], np.int64)
    at = start[level] + py * widths[level] + px
    assert np.array_equal(u32(planes[at].astype(np.float32)), u32(aux[:, 3])) and np.array_equal(planes[at], cand[3])


# ---- groups --------------------------------------------------------------------------------------------------------------------------
def run_batch(gpu, entry, prm, imgs, caps, width, device=False):
    capi = gpu._capi
    g, most = len(imgs), max(max(caps), 1)
    keep, bufs = [], []
    if device:
        import torch
    for k, img in enumerate(imgs):
        img = np.ascontiguousarray(img)
        cap = max(caps[k], 1)
        desc, loc, aux = np.full((cap, width), FILL, np.uint8), np.full((2, most), -7.5, np.float64), np.full((cap, 4), -7.5, np.float32)
        if device:
            img, desc, loc, aux = (torch.tensor(a).cuda() for a in (img, desc, loc, aux))
        keep.append(img)
        bufs.append((desc, loc, aux))
    if device:
        torch.cuda.synchronize()
    views = (capi.aps_fast_view * g)()
    for k in range(g):
        views[k].img, views[k].desc, views[k].loc, views[k].aux = (capi.ptr(keep[k]),) + tuple(capi.ptr(a) for a in bufs[k])
        views[k].cap, views[k].count = caps[k], -1
    h, w = imgs[0].shape[:2]
    rc = getattr(capi.lib, entry)(views, g, h, w, 1 if imgs[0].ndim == 2 else 3, capi.APS_IMG_U8_HWC, C.byref(prm), capi.APS_ROWMAJOR, width, most)
    if device:
        capi.check(capi.lib.aps_synchronize())
        bufs = [tuple(a.cpu().numpy() for a in b) for b in bufs]
    return rc, [int(views[k].count) for k in range(g)], bufs


@pytest.mark.parametrize("descriptor", ["FREAK", "ORB"])
def test_group_of_three_views_equals_the_per_view_calls(gpu, fm, descriptor):
    capi = gpu._capi
    imgs = [hc.blocks(8, 96, 128), np.full((96, 128), 140, np.uint8), hc.blocks(9, 96, 128)]
    width = WIDTH[descriptor]
    pyr = pyramid_params(capi, quality=0.01, levels=3, scale=1.2)
    prm = corner_params(capi, pyr, descriptor)
    single = []
    for img in imgs:
        rc, cnt, *_ = call(gpu, "aps_corner_extract", prm, img, 0, width)
        rc, cnt, desc, loc, aux = call(gpu, "aps_corner_extract", prm, img, cnt, width)
        assert rc == 0
        single.append((cnt, rows_of(desc, loc, aux, cnt, width)))
    counts = [s[0] for s in single]
    assert counts[0] == len(mirror("pyramid", descriptor)[0]) and counts[1] == 0 and counts[2] >= 8
    for device in (False, True):
        rc, got, bufs = run_batch(gpu, "aps_corner_extract_batch", prm, imgs, [c + 2 for c in counts], width, device)
        assert rc == 0 and got == counts
        for k in range(3):
            d, loc, aux = rows_of(*bufs[k], counts[k], width)
            assert np.array_equal(d, single[k][1][0]) and np.array_equal(u64(loc), u64(single[k][1][1]))
            assert np.array_equal(u32(aux), u32(single[k][1][2]))
            assert (bufs[k][0][counts[k]:] == FILL).all() and (bufs[k][2][counts[k]:] == -7.5).all()
    # one view that does not fit: every count is reported, nothing is written
    rc, got, bufs = run_batch(gpu, "aps_corner_extract_batch", prm, imgs, [counts[0] + 2, 4, counts[2] - 1], width)
    assert rc == capi.APS_E_CAP and got == counts and all((b[0] == FILL).all() and (b[2] == -7.5).all() for b in bufs)
    # and the wrapper
    inp = {"detector": "FAST", "CornerMethod": "Harris", "DescriptorMethod": descriptor, "NumLevels": 3}
    out = fm.fast_extract_batch(inp, imgs, want_aux=True)
    for k, (f, loc, aux) in enumerate(out):
        assert np.array_equal(f.Features, single[k][1][0]) and np.array_equal(u64(loc), u64(single[k][1][1])) and np.array_equal(u32(aux), u32(single[k][1][2]))


# ---- corner = APS_CORNER_FAST: the existing entries, byte for byte -----------------------------------------------------------------------
def test_fast_through_the_new_entries_equals_the_existing_entries(gpu):
    capi = gpu._capi
    img = fc.noise_rects(13, 70, 131)
    fast = capi.aps_fast_params(25, 100000, 1000000, 0)   # MinContrast 0.1
    p1, p3 = capi.aps_fast_pyramid_params(fast, 1, *S12), capi.aps_fast_pyramid_params(fast, 3, *S12)
    FASTC = capi.APS_CORNER_FAST

    def same(old, new, width):
        (rc0, n0, d0, l0, a0), (rc1, n1, d1, l1, a1) = old, new
        assert rc0 == rc1 == 0 and n0 == n1 >= 8
        for a, b in ((d0, d1), (l0, l1), (a0, a1)):   # the whole buffers: what is written and what is left alone
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
        return n0

    cap = 600
    n1 = same(call(gpu, "aps_fast_extract", fast, img, cap, 64), call(gpu, "aps_corner_extract", corner_params(capi, p1, "FREAK", FASTC), img, cap, 64), 64)
    n3 = same(call(gpu, "aps_fast_extract_pyramid", p3, img, cap, 64),
              call(gpu, "aps_corner_extract", corner_params(capi, p3, "FREAK", FASTC), img, cap, 64), 64)
    assert n3 > n1
    N = n3 // 3
    same(call(gpu, "aps_fast_extract_strongest", capi.aps_fast_strongest_params(p3, N), img, cap, 64),
         call(gpu, "aps_corner_extract", corner_params(capi, p3, "FREAK", FASTC, 1, N), img, cap, 64), 64)
    same(call(gpu, "aps_fast_extract_uniform", capi.aps_fast_uniform_params(capi.aps_fast_strongest_params(p3, N), 3, 5), img, cap, 64),
         call(gpu, "aps_corner_extract", corner_params(capi, p3, "FREAK", FASTC, 2, N, 3, 5), img, cap, 64), 64)
    for select, rows, cols in ((0, 0, 0), (1, 0, 0), (2, 3, 5)):
        same(call(gpu, "aps_fast_orb_extract", capi.aps_fast_orb_params(p3, select, N, rows, cols), img, cap, 32),
             call(gpu, "aps_corner_extract", corner_params(capi, p3, "ORB", FASTC, select, N, rows, cols), img, cap, 32), 32)
    imgs = [img, fc.noise_rects(14, 70, 131)]
    for old, desc, width in (("aps_fast_extract_batch", "FREAK", 64), ("aps_fast_orb_extract_batch", "ORB", 32)):
        rc0, c0, b0 = run_batch(gpu, old, p3, imgs, [cap, cap], width)
        rc1, c1, b1 = run_batch(gpu, "aps_corner_extract_batch", corner_params(capi, p3, desc, FASTC), imgs, [cap, cap], width)
        assert rc0 == rc1 == 0 and c0 == c1 and min(c0) >= 8
        for v0, v1 in zip(b0, b1):
            for a, b in zip(v0, v1):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the whole stitch --------------------------------------------------------------------------------------------------------------------
def test_stitch_end_to_end_with_harris_corners(gpu):
    """Views 0 and 1 of the FAST pipeline test's scene.  The mirror alone gives 1433 / 1471 rows, and the NumPy matcher on them 592
    matches, every one within 5.5 px of the known homography."""
    pl = import_module(gpu.__name__ + ".pipeline")
    views, cams = fc.scene()
    want = [hm.extract(v, fc.tables(), "FREAK", 1, 1.2, 0.01) for v in views[:2]]
    assert [len(w[0]) for w in want] == [1433, 1471]
    m, _ = fc.match_binary(want[0][0], want[1][0], 0.6, 20.0)
    Hm = cams[1]["K"] @ cams[1]["R"] @ cams[0]["R"].T @ np.linalg.inv(cams[0]["K"])
    p = np.concatenate([want[0][1][m[:, 0] - 1], np.ones((len(m), 1))], 1) @ Hm.T
    q = want[1][1][m[:, 1] - 1]
    assert len(m) == 592 and int((np.hypot(p[:, 0] / p[:, 2] - q[:, 0], p[:, 1] / p[:, 2] - q[:, 1]) <= 5.5).sum()) == 592
    inp = pl.default_input(detector="FAST", CornerMethod="Harris", Matchingthreshold=20, resizeImage=0)
    panos, info = pl.stitch(inp, views[:2], Ks=[c["K"] for c in cams[:2]], tile=(512, 512))
    assert info["n_features"] == [1433, 1471] and int(info["putative"][0, 1]) == 592
    assert info["n_components"] == 1 and len(panos) == 1 and sorted(info["components"][0]["members"]) == [0, 1]
    assert info["n_pairs_verified"] == 1 and len(info["result"]["inliers"][0]) > 0
    pano = panos[0].cpu().numpy() if hasattr(panos[0], "cpu") else np.asarray(panos[0])
    assert pano.ndim == 3 and (pano.max(axis=2) > 0).mean() > 0.5
