"""Device FAST/FREAK strongest-N against the NumPy mirror of the contract (tests/fast_strongest_mirror.py): the int64 Harris
responses, the rows kept, and of every kept row the location as f64 bits, score, bin, level, f32(R) and every descriptor byte
equal - integer arithmetic throughout, so there is no tolerance anywhere (the acceptance rule of test_fast_pyramid_gpu.py).
The figures per level are checked device-free in test_fast_strongest_mirror.py."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import fast_cases as fc
import fast_pyramid_cases as pc
import fast_pyramid_mirror as pmir
import fast_strongest_cases as sc

CAP_CASE, CAP_N = "120x160", 400   # 1516 candidates on four levels, 400 kept


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def pyramid_params(capi, name, max_features=0):
    _, nl, sf, mc = sc.spec(name)
    num, den = pmir.scale_rational(sf)
    return capi.aps_fast_pyramid_params(capi.aps_fast_params(int(np.floor(mc * 255)), 100000, 1000000, max_features), nl, num, den)


def params(capi, name, N, max_features=0):
    return capi.aps_fast_strongest_params(pyramid_params(capi, name, max_features), N)


def inputs(name, N=None):
    _, nl, sf, mc = sc.spec(name)
    inp = {"detector": "FAST", "MinContrast": mc, "NumLevels": nl, "ScaleFactor": sf}
    return inp if N is None else {**inp, "NumStrongest": N}


def bits(a, t):
    return np.ascontiguousarray(a).view(t)


def assert_equals_mirror(d, loc, aux, md, mloc, maux):
    assert d.shape == md.shape and loc.shape == mloc.shape and aux.shape == maux.shape, (d.shape, md.shape)
    assert d.dtype == np.uint8 and loc.dtype == np.float64 and aux.dtype == np.float32
    assert np.array_equal(aux[:, 2], maux[:, 2]), "levels"
    assert np.array_equal(bits(loc, np.uint64), bits(mloc, np.uint64)), "locations / rows kept"
    assert np.array_equal(aux[:, 0], maux[:, 0]), "scores"
    assert np.array_equal(aux[:, 1], maux[:, 1]), "orientation bins"
    assert np.array_equal(bits(aux[:, 3], np.uint32), bits(maux[:, 3], np.uint32)), "f32(R)"
    assert np.array_equal(d, md), "descriptor bytes (%d rows differ)" % int((d != md).any(1).sum())


# ---- the Harris response ---------------------------------------------------------------------------------------------------
def device_harris(gpu, name, device=False):
    capi = gpu._capi
    img = np.ascontiguousarray(sc.spec(name)[0])
    h, w, ch = img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3
    prm = pyramid_params(capi, name)
    cnt = C.c_int64(-1)
    capi.check(capi.lib.aps_fast_harris(capi.ptr(img), h, w, ch, capi.APS_IMG_U8_HWC, C.byref(prm), None, 0, C.byref(cnt)))
    n = cnt.value
    out = np.full(n + 3, -77, np.int64)
    rc = capi.lib.aps_fast_harris(capi.ptr(img), h, w, ch, capi.APS_IMG_U8_HWC, C.byref(prm), capi.ptr(out), n - 1, C.byref(cnt))
    assert rc == capi.APS_E_CAP and cnt.value == n and (out == -77).all()
    if device:
        import torch

        dimg, dout = torch.from_numpy(img.copy()).cuda(), torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        capi.check(capi.lib.aps_fast_harris(capi.ptr(dimg), h, w, ch, capi.APS_IMG_U8_HWC, C.byref(prm), capi.ptr(dout), n + 3, C.byref(cnt)))
        capi.check(capi.lib.aps_synchronize())
        out = dout.cpu().numpy()
    else:
        capi.check(capi.lib.aps_fast_harris(capi.ptr(img), h, w, ch, capi.APS_IMG_U8_HWC, C.byref(prm), capi.ptr(out), n + 3, C.byref(cnt)))
    assert cnt.value == n and (out[n:] == -77).all()
    return out[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["120x160", "96x131", "200x300x3", "planted", "tiled2"])
def test_harris_equals_the_mirror(gpu, name):
    R = sc.candidates(name, True)[3]
    got = device_harris(gpu, name)
    assert got.dtype == np.int64 and got.shape == R.shape
    assert np.array_equal(got, R), "%d of %d responses differ" % (int((got != R).sum()), len(R))
    if name == "planted":   # level 0: single pixels s above a flat field, in (row, col) order
        s = np.array([p[2] for p in fc.planted()[1]], np.int64)
        assert len(s) == 22 and np.array_equal(got[:22], 3024 * s ** 4)
    if name == "120x160":
        assert np.array_equal(device_harris(gpu, name, device=True), R)


# ---- the selection ---------------------------------------------------------------------------------------------------------
SELECTIONS = [("120x160", N) for N in (1, 3, 100, 400, 1515, 1516, 5000)] + [("200x300x3", 200), ("96x131", 200)] + \
             [(name, N) for name, (_, N) in sc.TIES.items()]


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", SELECTIONS)
def test_selection_equals_the_mirror(fm, name, N):
    md, mloc, maux = sc.mirror(name, N, True)
    f, loc, aux = fm.fast_extract(inputs(name, N), sc.spec(name)[0], want_aux=True)
    assert isinstance(f, fm.binaryFeatures) and f.NumBits == 512 and f.NumFeatures == len(md)
    assert_equals_mirror(f.Features, loc, aux, md, mloc, maux)


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", [("120x160", 400), ("200x300x3", 200), ("tiled1", 100)])
def test_kept_rows_are_rows_of_the_unselected_result(fm, name, N):
    img = sc.spec(name)[0]
    f0, l0, a0 = fm.fast_extract(inputs(name), img, want_aux=True)
    f, loc, aux = fm.fast_extract(inputs(name, N), img, want_aux=True)
    assert 0 < len(loc) < len(l0) and not a0[:, 3].any()
    rows = {(float(a[2]), x, y): i for i, (a, (x, y)) in enumerate(zip(a0, l0.tolist()))}
    at = np.array([rows[(float(a[2]), x, y)] for a, (x, y) in zip(aux, loc.tolist())])
    assert (np.diff(at) > 0).all()   # the same order
    assert np.array_equal(f.Features, f0.Features[at]) and np.array_equal(bits(loc, np.uint64), bits(l0[at], np.uint64))
    assert np.array_equal(aux[:, :3], a0[at, :3])


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", [("120x160", 1516), ("120x160", 5000), ("planted", 30), ("flat", 5)])
def test_no_more_candidates_than_N_gives_the_unselected_result(fm, name, N):
    img = sc.spec(name)[0]
    f0, l0, a0 = fm.fast_extract(inputs(name), img, want_aux=True)
    f, loc, aux = fm.fast_extract(inputs(name, N), img, want_aux=True)
    assert np.array_equal(f.Features, f0.Features) and np.array_equal(bits(loc, np.uint64), bits(l0, np.uint64))
    assert np.array_equal(aux[:, :3], a0[:, :3])
    assert np.array_equal(bits(aux[:, 3], np.uint32), bits(sc.candidates(name, True)[3].astype(np.float32), np.uint32))


# ---- capacity, padding, layouts, pointers -------------------------------------------------------------------------------------
def _raw(gpu, img, prm, cap, ldd, layout=None, ldl=None, fill=0xA5, device=False, with_out=True):
    capi = gpu._capi
    layout = capi.APS_ROWMAJOR if layout is None else layout
    h, w, ch = img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3
    img = np.ascontiguousarray(img)
    rows = max(cap, 1)
    ldl = rows if ldl is None else ldl
    desc = np.full((rows, ldd) if layout == capi.APS_ROWMAJOR else (64, ldd), fill, np.uint8)
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
    rc = capi.lib.aps_fast_extract_strongest(pi, h, w, ch, capi.APS_IMG_U8_HWC, C.byref(prm), pd, layout, ldd, pl, ldl, pa, cap, C.byref(cnt))
    if device:
        capi.check(capi.lib.aps_synchronize())
        desc, loc, aux = [a.cpu().numpy() for a in args[1:]]
    return rc, cnt.value, desc, loc, aux


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_capacity_is_the_number_kept(gpu, device):
    """cap = rows kept suffices although there are more candidates than cap; one less is APS_E_CAP with the true count and
    nothing written, for host and for device pointers; cap = 0 and desc = NULL count."""
    capi = gpu._capi
    img, prm = sc.spec(CAP_CASE)[0], params(gpu._capi, CAP_CASE, CAP_N)
    md, mloc, maux = sc.mirror(CAP_CASE, CAP_N, True)
    n = len(md)
    assert n == CAP_N < len(sc.candidates(CAP_CASE, True)[0])
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, n, 64, device=device)
    assert rc == 0 and cnt == n
    assert_equals_mirror(desc, np.ascontiguousarray(loc.T), aux, md, mloc, maux)
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, n - 1, 64, device=device)
    assert rc == capi.APS_E_CAP and cnt == n
    assert (desc == 0xA5).all() and (loc == -7.5).all() and (aux == -7.5).all()
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, 0, 64, device=device)   # cap = 0 counts
    assert rc == capi.APS_E_CAP and cnt == n and (desc == 0xA5).all()
    rc, cnt, *_ = _raw(gpu, img, prm, n, 64, with_out=False)   # desc = NULL counts
    assert cnt == n and rc == capi.APS_E_ARG    # features present and no output to put them in


@pytest.mark.gpu
def test_max_features_is_a_limit_on_the_rows_kept(gpu):
    img = sc.spec(CAP_CASE)[0]
    md, mloc, maux = sc.mirror(CAP_CASE, CAP_N, True)
    rc, cnt, *_ = _raw(gpu, img, params(gpu._capi, CAP_CASE, CAP_N, max_features=CAP_N - 1), CAP_N, 64)
    assert rc == gpu._capi.APS_E_CAP and cnt == CAP_N
    rc, cnt, desc, loc, aux = _raw(gpu, img, params(gpu._capi, CAP_CASE, CAP_N, max_features=CAP_N), CAP_N, 64)
    assert rc == 0 and cnt == CAP_N   # (the 1516 candidates are above the limit, the rows kept are not)
    assert_equals_mirror(desc, np.ascontiguousarray(loc.T), aux, md, mloc, maux)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_padded_outputs_keep_their_padding(gpu, device):
    """ldd = 80 > 64 and ldl = cap + 5 > cap, cap > count: bytes between the rows, rows count..cap and the tail of loc stay
    the caller's, for host and for device pointers."""
    img, prm = sc.spec(CAP_CASE)[0], params(gpu._capi, CAP_CASE, CAP_N)
    md, mloc, maux = sc.mirror(CAP_CASE, CAP_N, True)
    n = len(md)
    cap = n + 3
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, cap, 80, ldl=cap + 5, device=device)
    assert rc == 0 and cnt == n
    assert_equals_mirror(np.ascontiguousarray(desc[:n, :64]), np.ascontiguousarray(loc[:, :n].T), aux[:n], md, mloc, maux)
    assert (desc[:, 64:] == 0xA5).all() and (desc[n:] == 0xA5).all()
    assert (loc[:, n:] == -7.5).all() and (aux[n:] == -7.5).all()


@pytest.mark.gpu
def test_column_major_descriptors(gpu):
    capi = gpu._capi
    img, prm = sc.spec(CAP_CASE)[0], params(capi, CAP_CASE, CAP_N)
    md, mloc, maux = sc.mirror(CAP_CASE, CAP_N, True)
    n = len(md)
    ld = n + 5
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, n, ld, layout=capi.APS_COLMAJOR, ldl=ld)
    assert rc == 0 and cnt == n and desc.shape == (64, ld)
    assert np.array_equal(desc[:, :n].T, md) and (desc[:, n:] == 0xA5).all()
    assert np.array_equal(loc[:, :n].T, mloc) and (loc[:, n:] == -7.5).all()
    assert np.array_equal(bits(aux, np.uint32), bits(maux, np.uint32))


@pytest.mark.gpu
def test_resident_output_and_two_runs(fm):
    import torch

    md, mloc, maux = sc.mirror(CAP_CASE, CAP_N, True)
    inp = inputs(CAP_CASE, CAP_N)
    img = sc.spec(CAP_CASE)[0]
    dimg = torch.from_numpy(img.copy()).cuda()
    torch.cuda.synchronize()
    for compact in (False, True):
        f, pts = fm.fast_extract(inp, dimg, device_out=True, points_device=True, compact=compact)
        assert f.Features.is_cuda and pts.is_cuda and f.Features.dtype == torch.uint8
        assert np.array_equal(f.Features.cpu().numpy(), md) and np.array_equal(pts.cpu().numpy(), mloc)
    runs = [fm.fast_extract(inp, img, want_aux=True) for _ in range(2)]
    assert np.array_equal(runs[0][0].Features, runs[1][0].Features) and np.array_equal(runs[0][1], runs[1][1])
    assert np.array_equal(bits(runs[0][2], np.uint32), bits(runs[1][2], np.uint32))
    for entry in (fm.getFeaturePoints, fm.extract_features):
        f, pts = entry(inp, img)
        assert np.array_equal(f.Features, md) and np.array_equal(pts, mloc)


# ---- the twin pair: B is level 2 of A --------------------------------------------------------------------------------------
TWIN_N = 600


def rgb(g):
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))   # (rgb2gray's integer plane of a gray triple is the gray value)


@pytest.fixture(scope="module")
def twins(fm):
    """Device rows of A and B at three levels with N = 600 and of single-level B with N = 164; they equal the mirror's.
    Also [(row of A's set, row of B's set)], 1-based, of the 164 twins."""
    A, B = pc.twin_images()
    out = [fm.fast_extract(inputs(name, N), sc.spec(name)[0], want_aux=True) for name, N in (("twinA", TWIN_N), ("twinB", TWIN_N), ("twinB1", 164))]
    for (f, loc, aux), (name, N) in zip(out, (("twinA", TWIN_N), ("twinB", TWIN_N), ("twinB1", 164))):
        assert_equals_mirror(f.Features, loc, aux, *sc.mirror(name, N, True))
    (fa, la, aa), (fb, lb, ab), (f1, l1, a1) = out
    at2 = np.flatnonzero(aa[:, 2] == 2)
    rows_b = {tuple(r): i for i, r in enumerate(lb.tolist())}
    pairs = [(int(at2[t]) + 1, rows_b[tuple(l1[t].tolist())] + 1) for t in range(len(l1))]
    return out, pairs


@pytest.mark.gpu
def test_twin_pair_survives_the_selection(fm, twins):
    ((fa, la, aa), (fb, lb, ab), (f1, l1, a1)), pairs = twins
    assert pc.per_level(aa, 3) == [238, 198, 164] and pc.per_level(ab, 3) == [238, 227, 135]
    assert fm.fast_extract(inputs("twinB"), sc.spec("twinB")[0])[0].NumFeatures == 1202
    at2 = np.flatnonzero(aa[:, 2] == 2)
    assert len(f1) == 164 and np.array_equal(fa.Features[at2], f1.Features)
    assert np.array_equal(bits(aa[at2][:, [0, 1, 3]], np.uint32), bits(a1[:, [0, 1, 3]], np.uint32))
    m, d = fm.matchFeaturesScratch(fa, fb, MatchThreshold=20.0, MaxRatio=0.6)
    assert len(m) == 164
    got = {(int(i), int(j)): float(v) for (i, j), v in zip(m, d)}
    assert len(pairs) == 164 and all(got.get(p) == 0.0 for p in pairs)   # every twin, at metric 0


@pytest.mark.gpu
def test_twin_pair_through_match_and_verify(gpu, twins):
    """The pair (A, B), each cut to its 600 strongest, is verified; its inliers hold at least 95 % of the 164 twins (exact
    correspondences of one affine map, so inliers of the true model; the 5 % is the existing twin test's room for the refit's
    pull from other inliers within maxDistance), and the model maps B's corners to within 1 px of
    x_A = (x_B - 0.5) * 240 / 167 + 0.5, y_A = (y_B - 0.5) * 180 / 125 + 0.5.
    Observed on an MI355X: 164 putative matches, 164 inliers, 164 of 164 twins among them (share 1.0000); corner errors 0.0000 px."""
    pl = import_module(gpu.__name__ + ".pipeline")
    A, B = pc.twin_images()
    inp = pl.default_input(detector="FAST", NumLevels=pc.TWIN_LEVELS, NumStrongest=TWIN_N, MinContrast=pc.TWIN_MC, Matchingthreshold=20)
    descs, kps = pl.extract_features(inp, [rgb(A), rgb(B)])
    ((fa, la, aa), (fb, lb, ab), _), pairs = twins
    assert np.array_equal(np.asarray(kps[0]), la) and np.array_equal(np.asarray(kps[1]), lb)
    assert np.array_equal(descs[0].Features, fa.Features) and np.array_equal(descs[1].Features, fb.Features)
    res = pl.match_and_verify(inp, descs, kps, 0)
    assert res["pairs"] == [(0, 1)]
    inl = {(int(i), int(j)) for i, j in res["inliers"][0]}
    share = sum(p in inl for p in pairs) / 164.0
    print("twins among the inliers: %d of 164 (%.4f); inliers %d, putative %d" % (round(share * 164), share, len(inl), int(res["putative"][0, 1])))
    assert share >= 0.95
    H = np.asarray(res["models"][0], np.float64)   # B -> A
    for xb in (0.5, 167.5):
        for yb in (0.5, 125.5):
            p = H @ np.array([xb, yb, 1.0])
            want = ((xb - 0.5) * 240 / 167 + 0.5, (yb - 0.5) * 180 / 125 + 0.5)
            err = float(np.hypot(p[0] / p[2] - want[0], p[1] / p[2] - want[1]))
            print("corner (%.1f, %.1f): %.4f px" % (xb, yb, err))
            assert err <= 1.0


@pytest.mark.gpu
def test_stitch_of_the_twin_pair_ends_with_one_panorama(gpu):
    pl = import_module(gpu.__name__ + ".pipeline")
    A, B = pc.twin_images()
    inp = pl.default_input(detector="FAST", NumLevels=pc.TWIN_LEVELS, NumStrongest=TWIN_N, MinContrast=pc.TWIN_MC, Matchingthreshold=20,
                           resizeImage=0)
    f = 450.0   # B is A seen at 167 / 240 of the focal length, same direction
    Ks = [np.array([[f * s, 0, w / 2.0], [0, f * s, h / 2.0], [0, 0, 1.0]]) for (h, w), s in ((A.shape, 1.0), (B.shape, 167.0 / 240.0))]
    panos, info = pl.stitch(inp, [rgb(A), rgb(B)], Ks=Ks, tile=(512, 512))
    assert list(info["n_features"]) == [TWIN_N, TWIN_N]
    assert info["n_components"] == 1 and len(panos) == 1 and sorted(info["components"][0]["members"]) == [0, 1]
    pano = panos[0].cpu().numpy() if hasattr(panos[0], "cpu") else np.asarray(panos[0])
    assert pano.ndim == 3 and (pano.max(axis=2) > 0).mean() > 0.5
