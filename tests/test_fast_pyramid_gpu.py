"""Device FAST/FREAK over a scale pyramid against the NumPy mirror of the contract (tests/fast_pyramid_mirror.py): the level
planes, count, locations as f64 bits, score, bin, level and every descriptor byte equal - integer arithmetic throughout and
one IEEE division per coordinate, so there is no tolerance anywhere.  The cases and what each catches: fast_pyramid_cases.CASES
(their keypoints per level are checked device-free in test_fast_pyramid_mirror.py)."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import fast_cases as fc
import fast_pyramid_cases as pc
import fast_pyramid_mirror as pmir

CAP_CASE = "120x160"   # four levels: 825 / 420 / 208 / 63 keypoints


def mirror(name):
    return pc.mirror(name, True)   # (on the tables the library reports)


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def params(capi, name=None, mc=None, nl=None, sf=None, max_features=0):
    if name is not None:
        _, nl, sf, mc, _ = pc.CASES[name]
    num, den = pmir.scale_rational(sf)
    return capi.aps_fast_pyramid_params(capi.aps_fast_params(int(np.floor(mc * 255)), 100000, 1000000, max_features), nl, num, den)


def matlab_order(img):
    """Planar, column-major: element (y, x, q) at q * h * w + x * h + y."""
    return np.ascontiguousarray(img.T if img.ndim == 2 else img.transpose(2, 1, 0))


def assert_equals_mirror(d, loc, aux, md, mloc, maux):
    assert d.shape == md.shape and loc.shape == mloc.shape and aux.shape == maux.shape, (d.shape, md.shape)
    assert d.dtype == np.uint8 and loc.dtype == np.float64 and aux.dtype == np.float32
    assert np.array_equal(aux[:, 2], maux[:, 2]), "levels"
    assert np.array_equal(np.ascontiguousarray(loc).view(np.uint64), np.ascontiguousarray(mloc).view(np.uint64)), "locations / keypoint order"
    assert np.array_equal(aux[:, 0], maux[:, 0]), "scores"
    assert np.array_equal(aux[:, 1], maux[:, 1]), "orientation bins (%d differ)" % int((aux[:, 1] != maux[:, 1]).sum())
    assert not aux[:, 3].any()
    assert np.array_equal(d, md), "descriptor bytes (%d rows differ)" % int((d != md).any(1).sum())


# ---- the level planes ------------------------------------------------------------------------------------------------------
def device_planes(gpu, name, matlab=False, device=False):
    capi = gpu._capi
    img = pc.image(name)
    h, w, ch = img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3
    prm = params(capi, name)
    nbytes = C.c_int64(0)
    src = matlab_order(img) if matlab else np.ascontiguousarray(img)
    layout = capi.APS_IMG_U8_MATLAB if matlab else capi.APS_IMG_U8_HWC
    capi.check(capi.lib.aps_fast_pyramid_planes(capi.ptr(src), h, w, ch, layout, C.byref(prm), None, 0, C.byref(nbytes)))
    out = np.full(nbytes.value + 7, 0xA5, np.uint8)
    rc = capi.lib.aps_fast_pyramid_planes(capi.ptr(src), h, w, ch, layout, C.byref(prm), capi.ptr(out), nbytes.value - 1, C.byref(nbytes))
    assert rc == capi.APS_E_CAP and (out == 0xA5).all()
    if device:
        import torch

        dsrc, dout = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        capi.check(capi.lib.aps_fast_pyramid_planes(capi.ptr(dsrc), h, w, ch, layout, C.byref(prm), capi.ptr(dout), out.size, C.byref(nbytes)))
        capi.check(capi.lib.aps_synchronize())
        out = dout.cpu().numpy()
    else:
        capi.check(capi.lib.aps_fast_pyramid_planes(capi.ptr(src), h, w, ch, layout, C.byref(prm), capi.ptr(out), out.size, C.byref(nbytes)))
    assert (out[nbytes.value:] == 0xA5).all()
    return out[:nbytes.value]


def mirror_planes(name):
    _, nl, sf, _, _ = pc.CASES[name]
    return pmir.planes(pc.image(name), nl, sf, fc.tables().margin)


def assert_planes_equal(got, want):
    assert got.size == sum(p.size for p in want)
    at = 0
    for l, p in enumerate(want):
        g = got[at:at + p.size].reshape(p.shape)
        assert np.array_equal(g, p), "level %d: %d pixels differ" % (l, int((g != p).sum()))
        at += p.size


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pc.CASES))
def test_planes_equal_the_mirror(gpu, name):
    assert_planes_equal(device_planes(gpu, name), mirror_planes(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["120x160", "200x300x3"])
def test_planes_of_matlab_layout_images_and_device_pointers(gpu, name):
    assert_planes_equal(device_planes(gpu, name, matlab=True), mirror_planes(name))
    assert_planes_equal(device_planes(gpu, name, device=True), mirror_planes(name))


# ---- extraction ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pc.CASES))
def test_device_equals_mirror(fm, name):
    _, nl, sf, mc, counts = pc.CASES[name]
    md, mloc, maux = mirror(name)
    f, loc, aux = fm.fast_extract({"detector": "FAST", "MinContrast": mc, "NumLevels": nl, "ScaleFactor": sf}, pc.image(name), want_aux=True)
    assert isinstance(f, fm.binaryFeatures) and f.NumBits == 512 and f.NumFeatures == len(md) == sum(counts)
    assert_equals_mirror(f.Features, loc, aux, md, mloc, maux)
    if name == "flat":
        assert f.Features.shape == (0, 64) and loc.shape == (0, 2)


def _raw(gpu, img, prm, cap, ldd, layout=None, ldl=None, fill=0xA5, device=False, with_out=True, matlab=False, entry=None):
    capi = gpu._capi
    layout = capi.APS_ROWMAJOR if layout is None else layout
    h, w, ch = img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3
    img = matlab_order(img) if matlab else np.ascontiguousarray(img)
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
    entry = capi.lib.aps_fast_extract_pyramid if entry is None else entry
    rc = entry(pi, h, w, ch, capi.APS_IMG_U8_MATLAB if matlab else capi.APS_IMG_U8_HWC, C.byref(prm), pd, layout, ldd, pl, ldl, pa, cap,
               C.byref(cnt))
    if device:
        capi.check(capi.lib.aps_synchronize())
        desc, loc, aux = [a.cpu().numpy() for a in args[1:]]
    return rc, cnt.value, desc, loc, aux


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["129x1230", "200x300x3"])
def test_one_level_through_the_new_entry_equals_aps_fast_extract(gpu, name):
    capi = gpu._capi
    img, mc = pc.image(name), pc.CASES[name][3]
    prm = params(capi, mc=mc, nl=1, sf=1.2)
    rc0, n, d0, l0, a0 = _raw(gpu, img, prm.fast, 8192, 64, entry=capi.lib.aps_fast_extract)
    rc1, n1, d1, l1, a1 = _raw(gpu, img, prm, 8192, 64)
    assert rc0 == 0 and rc1 == 0 and n == n1 == pc.CASES[name][4][0]
    assert np.array_equal(d0, d1) and np.array_equal(l0.view(np.uint64), l1.view(np.uint64)) and np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
    assert not a0[:n, 2:].any()


@pytest.mark.gpu
def test_capacity_too_small_reports_the_count_and_count_only_mode(gpu):
    capi = gpu._capi
    img, prm = pc.image(CAP_CASE), params(gpu._capi, CAP_CASE)
    md, mloc, maux = mirror(CAP_CASE)
    n = len(md)
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, 900, 64)   # level 0 alone fits, the pyramid does not
    assert rc == capi.APS_E_CAP and cnt == n
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, 0, 64)   # cap = 0 counts
    assert rc == capi.APS_E_CAP and cnt == n and (desc == 0xA5).all()
    rc, cnt, *_ = _raw(gpu, img, prm, n, 64, with_out=False)   # desc = NULL counts
    assert cnt == n and rc == capi.APS_E_ARG    # features present and no output to put them in
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, n, 64)
    assert rc == 0 and cnt == n
    assert_equals_mirror(desc, np.ascontiguousarray(loc[:, :n].T), aux, md, mloc, maux)


@pytest.mark.gpu
def test_max_features_is_a_limit_on_the_count(gpu):
    img = pc.image(CAP_CASE)
    md, mloc, maux = mirror(CAP_CASE)
    n = len(md)
    rc, cnt, *_ = _raw(gpu, img, params(gpu._capi, CAP_CASE, max_features=n - 1), n, 64)
    assert rc == gpu._capi.APS_E_CAP and cnt == n
    rc, cnt, desc, loc, aux = _raw(gpu, img, params(gpu._capi, CAP_CASE, max_features=n), n, 64)
    assert rc == 0 and cnt == n
    assert_equals_mirror(desc, np.ascontiguousarray(loc.T), aux, md, mloc, maux)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_padded_outputs_keep_their_padding(gpu, device):
    """ldd = 80 > 64 and ldl = cap + 5 > cap, cap > count: bytes between the rows, rows count..cap and the tail of loc stay
    the caller's, for host and for device pointers."""
    img, prm = pc.image(CAP_CASE), params(gpu._capi, CAP_CASE)
    md, mloc, maux = mirror(CAP_CASE)
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
    img, prm = pc.image(CAP_CASE), params(capi, CAP_CASE)
    md, mloc, maux = mirror(CAP_CASE)
    n = len(md)
    ld = n + 5
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, n, ld, layout=capi.APS_COLMAJOR, ldl=ld)
    assert rc == 0 and cnt == n and desc.shape == (64, ld)
    assert np.array_equal(desc[:, :n].T, md) and (desc[:, n:] == 0xA5).all()
    assert np.array_equal(loc[:, :n].T, mloc) and (loc[:, n:] == -7.5).all()


@pytest.mark.gpu
def test_matlab_layout_image(gpu):
    img, prm = pc.image("200x300x3"), params(gpu._capi, "200x300x3")
    md, mloc, maux = mirror("200x300x3")
    n = len(md)
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, n, 64, matlab=True)
    assert rc == 0 and cnt == n
    assert_equals_mirror(desc, np.ascontiguousarray(loc.T), aux, md, mloc, maux)


@pytest.mark.gpu
def test_resident_output_and_getFeaturePoints_equal_the_host_result(fm):
    import torch

    md, mloc, maux = mirror(CAP_CASE)
    _, nl, sf, mc, _ = pc.CASES[CAP_CASE]
    inp = {"detector": "FAST", "MinContrast": mc, "NumLevels": nl, "ScaleFactor": sf}
    dimg = torch.from_numpy(pc.image(CAP_CASE).copy()).cuda()
    torch.cuda.synchronize()
    for compact in (False, True):
        f, pts = fm.fast_extract(inp, dimg, device_out=True, points_device=True, compact=compact)
        assert f.Features.is_cuda and pts.is_cuda and f.Features.dtype == torch.uint8
        assert np.array_equal(f.Features.cpu().numpy(), md) and np.array_equal(pts.cpu().numpy(), mloc)
    f, pts = fm.getFeaturePoints(inp, pc.image(CAP_CASE))
    assert np.array_equal(f.Features, md) and np.array_equal(pts, mloc)
    f, pts = fm.extract_features(inp, pc.image(CAP_CASE))
    assert np.array_equal(f.Features, md) and np.array_equal(pts, mloc)


# ---- the twin pair: B is level 2 of A --------------------------------------------------------------------------------------
def rgb(g):
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))   # (rgb2gray's integer plane of a gray triple is the gray value)


@pytest.fixture(scope="module")
def twins(fm):
    """Device features of three-level A, single-level A and B; they equal the mirror's."""
    A, B = pc.twin_images()
    inp = {"detector": "FAST", "MinContrast": pc.TWIN_MC}
    out = [fm.fast_extract({**inp, "NumLevels": pc.TWIN_LEVELS, "ScaleFactor": pc.TWIN_SCALE}, A, want_aux=True),
           fm.fast_extract(inp, A, want_aux=True), fm.fast_extract(inp, B, want_aux=True)]
    for (f, loc, aux), (md, mloc, maux) in zip(out, pc.twin_mirror(True)):
        assert_equals_mirror(f.Features, loc, aux, md, mloc, maux)
    return out


@pytest.mark.gpu
def test_twin_pair_is_matched_only_through_the_pyramid(fm, twins):
    (f3, l3, a3), (f1, l1, a1), (fb, lb, ab) = twins
    at2 = np.flatnonzero(a3[:, 2] == 2)
    assert len(at2) == len(fb) == 728
    m, d = fm.matchFeaturesScratch(f3, fb, MatchThreshold=10.0, MaxRatio=0.6)
    got = {(int(i), int(j)): float(v) for (i, j), v in zip(m, d)}
    assert all(got.get((int(at2[t]) + 1, t + 1)) == 0.0 for t in range(728))   # every twin, at metric 0
    m1, _ = fm.matchFeaturesScratch(f1, fb, MatchThreshold=10.0, MaxRatio=0.6)
    assert len(m1) < 0.05 * len(fb)


@pytest.mark.gpu
def test_twin_pair_through_match_and_verify(gpu, twins):
    """The pair (A, B) is verified, its inliers hold at least 95 % of the twins (exact correspondences of one affine map, so
    inliers of the true model; the 5 % is room for the refit's pull from other inliers within maxDistance), and the model
    maps B's corners to within 1 px of x_A = (x_B - 0.5) * 240 / 167 + 0.5, y_A = (y_B - 0.5) * 180 / 125 + 0.5.
    Observed on an MI355X: 729 putative matches, 728 inliers, 728 of 728 twins among them (share 1.0000); corner errors 0.0000 px."""
    pl = import_module(gpu.__name__ + ".pipeline")
    A, B = pc.twin_images()
    inp = pl.default_input(detector="FAST", NumLevels=pc.TWIN_LEVELS, MinContrast=pc.TWIN_MC, Matchingthreshold=20)
    descs, kps = pl.extract_features(inp, [rgb(A), rgb(B)])
    (f3, l3, a3), _, (fb, lb, _) = twins
    # (B gets its own three levels from the same input; its level 0, the first 728 rows, is single-level B)
    assert np.array_equal(np.asarray(kps[0]), l3) and np.array_equal(np.asarray(kps[1])[:728], lb) and len(kps[1]) > 728
    assert np.array_equal(descs[1].Features[:728], fb.Features)
    res = pl.match_and_verify(inp, descs, kps, 0)
    assert res["pairs"] == [(0, 1)]
    at2 = np.flatnonzero(a3[:, 2] == 2)
    inl = {(int(i), int(j)) for i, j in res["inliers"][0]}
    share = sum((int(at2[t]) + 1, t + 1) in inl for t in range(728)) / 728.0
    print("twins among the inliers: %d of 728 (%.4f); inliers %d, putative %d" % (round(share * 728), share, len(inl), int(res["putative"][0, 1])))
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
    inp = pl.default_input(detector="FAST", NumLevels=pc.TWIN_LEVELS, MinContrast=pc.TWIN_MC, Matchingthreshold=20, resizeImage=0)
    f = 450.0   # B is A seen at 167 / 240 of the focal length, same direction
    Ks = [np.array([[f * s, 0, w / 2.0], [0, f * s, h / 2.0], [0, 0, 1.0]]) for (h, w), s in ((A.shape, 1.0), (B.shape, 167.0 / 240.0))]
    panos, info = pl.stitch(inp, [rgb(A), rgb(B)], Ks=Ks, tile=(512, 512))
    assert info["n_features"][0] == 4673 and info["n_features"][1] > 728   # (B's own three levels)
    assert info["n_components"] == 1 and len(panos) == 1 and sorted(info["components"][0]["members"]) == [0, 1]
    pano = panos[0].cpu().numpy() if hasattr(panos[0], "cpu") else np.asarray(panos[0])
    assert pano.ndim == 3 and (pano.max(axis=2) > 0).mean() > 0.5
