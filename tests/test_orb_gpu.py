"""Device FAST/ORB (input.DescriptorMethod = 'ORB': aps_fast_orb_extract, aps_fast_orb_extract_batch) against the NumPy mirror of the
contract (tests/orb_mirror.py): count, locations as f64 bits, score, bin, level and every descriptor byte equal - integer arithmetic
throughout, so there is no tolerance anywhere.  Then the rows through selection, groups, layouts, the 32-byte matchers and the stitch."""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest

import fast_cases as fc
import fast_pyramid_cases as pc
import fast_pyramid_mirror as pmir
import fast_strongest_mirror as smir
import orb_mirror as om
import uniform_mirror as umir

# name: (image builder, MinContrast) - the single-level cases of the FAST/FREAK tests, built again from fast_cases
CASES = {
    "47x49": (lambda: fc.noise_rects(11, 47, 49), 0.05),          # one admissible pixel: the patch at both margins
    "64x64": (lambda: fc.noise_lattice(12, 64, 64), 0.05),        # one tile column, one bitmap word per row
    "70x131": (lambda: fc.noise_rects(13, 70, 131), 0.1),         # tile and 64-bit word boundaries not aligned
    "129x1030": (lambda: fc.noise_rects(14, 129, 1030), 0.2),     # crosses the 1024-px row-scan chunk
    "200x300x3": (lambda: fc.noise_rects(15, 200, 300, 3), 0.2),  # RGB
    "planted": (lambda: fc.planted()[0], 0.2),                    # first / last admissible row and column, seams; zero moments
    "flat": (lambda: np.full((90, 100), 77, np.uint8), 0.2),
}
COUNTS = {"47x49": 1, "64x64": 81, "70x131": 131, "129x1030": 1082, "200x300x3": 87, "planted": 22, "flat": 0}   # the FREAK tests' counts
CAP_CASE = "120x160"   # of fast_pyramid_cases: four levels, 825 / 420 / 208 / 63 keypoints


@functools.lru_cache(maxsize=None)
def image(name):
    img = CASES[name][0]()
    img.setflags(write=False)
    return img


def frozen(t):
    for a in t:
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def mirror(name):
    return frozen(om.extract(image(name), MinContrast=CASES[name][1]))


@functools.lru_cache(maxsize=None)
def pyramid_mirror(name):
    _, nl, sf, mc, _ = pc.CASES[name]
    return frozen(om.extract(pc.image(name), nl, sf, mc))


@functools.lru_cache(maxsize=None)
def pyramid_candidates(name):
    _, nl, sf, mc, _ = pc.CASES[name]
    desc, loc, aux, R, shapes = om.candidates(pc.image(name), nl, sf, mc)
    return frozen((desc, loc, aux, R)) + (shapes,)


def pyramid_input(name, **extra):
    _, nl, sf, mc, _ = pc.CASES[name]
    return {"detector": "FAST", "DescriptorMethod": "ORB", "MinContrast": mc, "NumLevels": nl, "ScaleFactor": sf, **extra}


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_equals_mirror(d, loc, aux, md, mloc, maux):
    assert d.shape == md.shape and loc.shape == mloc.shape and aux.shape == maux.shape, (d.shape, md.shape)
    assert d.dtype == np.uint8 and loc.dtype == np.float64 and aux.dtype == np.float32
    assert np.array_equal(aux[:, 2], maux[:, 2]), "levels"
    assert np.array_equal(u64(loc), u64(mloc)), "locations / keypoint order"
    assert np.array_equal(aux[:, 0], maux[:, 0]), "scores"
    assert np.array_equal(aux[:, 1], maux[:, 1]), "orientation bins (%d differ)" % int((aux[:, 1] != maux[:, 1]).sum())
    assert not aux[:, 3].any()
    assert np.array_equal(d, md), "descriptor bytes (%d rows differ)" % int((d != md).any(1).sum())


# ---- device equals mirror ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_mirror(fm, name):
    md, mloc, maux = mirror(name)
    assert len(md) == COUNTS[name]
    inp = {"detector": "FAST", "DescriptorMethod": "ORB", "MinContrast": CASES[name][1]}
    f, loc, aux = fm.fast_extract(inp, image(name), want_aux=True)
    assert isinstance(f, fm.binaryFeatures) and f.NumBits == 256 and f.Features.shape == (COUNTS[name], 32)
    assert_equals_mirror(f.Features, loc, aux, md, mloc, maux)
    if name == "planted":
        # a bright pixel with no other within its disc has a zero moment - every bin ties, bin 0 wins: 5 of the 22
        g = image(name).astype(np.int64)
        m10, m01 = om.moments(g, loc[:, 1].astype(np.int64) - 1, loc[:, 0].astype(np.int64) - 1)
        zero = (m10 == 0) & (m01 == 0)
        assert int(zero.sum()) == 5 and not aux[zero, 1].any()
    # everything but the descriptor and the bin is the FREAK call's, bit for bit
    ff, floc, faux = fm.fast_extract({**inp, "DescriptorMethod": "FREAK"}, image(name), want_aux=True)
    f0, loc0, aux0 = fm.fast_extract({k: v for k, v in inp.items() if k != "DescriptorMethod"}, image(name), want_aux=True)
    assert ff.Features.shape == (COUNTS[name], 64) and np.array_equal(ff.Features, f0.Features) and np.array_equal(faux, aux0)
    assert np.array_equal(u64(floc), u64(loc)) and np.array_equal(faux[:, [0, 2, 3]], aux[:, [0, 2, 3]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pc.CASES))
def test_pyramid_equals_mirror(fm, name):
    md, mloc, maux = pyramid_mirror(name)
    assert pc.per_level(maux, len(pc.CASES[name][4])) == pc.CASES[name][4]
    f, loc, aux = fm.fast_extract(pyramid_input(name), pc.image(name), want_aux=True)
    assert f.NumBits == 256 and f.NumFeatures == len(md)
    assert_equals_mirror(f.Features, loc, aux, md, mloc, maux)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["NumStrongest", "NumUniform"])
@pytest.mark.parametrize("name", list(pc.CASES))
def test_selected_rows_are_rows_of_the_unselected_result(fm, name, key):
    """Kept rows are rows of the unselected ORB result (the mirror's, by the test above), in order; which rows, their locations,
    score, level and f32(R) are the FREAK call's with the same keys."""
    md, mloc, maux = pyramid_mirror(name)
    N = max(1, len(md) // 3)
    extra = {key: N, **({"UniformGrid": (3, 5)} if key == "NumUniform" else {})}
    f, loc, aux = fm.fast_extract(pyramid_input(name, **extra), pc.image(name), want_aux=True)
    ff, floc, faux = fm.fast_extract({**pyramid_input(name, **extra), "DescriptorMethod": "FREAK"}, pc.image(name), want_aux=True)
    assert f.Features.shape == (len(ff), 32) and len(f) <= N and (len(md) == 0 or len(f) > 0)
    assert np.array_equal(u64(loc), u64(floc)) and np.array_equal(aux[:, [0, 2, 3]].view(np.uint32), faux[:, [0, 2, 3]].view(np.uint32))
    row_of = {(int(l), int(x), int(y)): i for i, (l, (x, y)) in enumerate(zip(maux[:, 2], u64(mloc)))}
    assert len(row_of) == len(md)
    idx = np.array([row_of[(int(l), int(x), int(y))] for l, (x, y) in zip(aux[:, 2], u64(loc))], np.int64)
    assert (np.diff(idx) > 0).all()
    assert np.array_equal(f.Features, md[idx]) and np.array_equal(aux[:, 1], maux[idx, 1])
    # and the whole result is the mirror's own selection from its ORB rows
    cand = pyramid_candidates(name)
    sd, sloc, saux = smir.pick(cand, N) if key == "NumStrongest" else umir.fast_pick(cand, N, (3, 5))
    assert np.array_equal(f.Features, sd) and np.array_equal(u64(loc), u64(sloc)) and np.array_equal(aux.view(np.uint32), saux.view(np.uint32))


# ---- the raw entries ---------------------------------------------------------------------------------------------------------------
def orb_params(capi, name, select=0, n_select=0, rows=0, cols=0, max_features=0):
    _, nl, sf, mc, _ = pc.CASES[name]
    num, den = pmir.scale_rational(sf)
    fast = capi.aps_fast_params(int(np.floor(mc * 255)), 100000, 1000000, max_features)
    return capi.aps_fast_orb_params(capi.aps_fast_pyramid_params(fast, nl, num, den), select, n_select, rows, cols)


def _raw(gpu, img, prm, cap, ldd, layout=None, ldl=None, fill=0xA5, device=False, with_out=True):
    capi = gpu._capi
    layout = capi.APS_ROWMAJOR if layout is None else layout
    h, w, ch = img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3
    img = np.ascontiguousarray(img)
    rows = max(cap, 1)
    ldl = rows if ldl is None else ldl
    desc = np.full((rows, ldd) if layout == capi.APS_ROWMAJOR else (32, ldd), fill, np.uint8)
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
    rc = capi.lib.aps_fast_orb_extract(pi, h, w, ch, capi.APS_IMG_U8_HWC, C.byref(prm), pd, layout, ldd, pl, ldl, pa, cap, C.byref(cnt))
    if device:
        capi.check(capi.lib.aps_synchronize())
        desc, loc, aux = [a.cpu().numpy() for a in args[1:]]
    return rc, cnt.value, desc, loc, aux


@pytest.mark.gpu
def test_capacity_too_small_reports_the_count_and_count_only_mode(gpu):
    capi = gpu._capi
    img, prm = pc.image(CAP_CASE), orb_params(gpu._capi, CAP_CASE)
    md, mloc, maux = pyramid_mirror(CAP_CASE)
    n = len(md)
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, n - 1, 32)
    assert rc == capi.APS_E_CAP and cnt == n and (desc == 0xA5).all() and (loc == -7.5).all() and (aux == -7.5).all()   # nothing written
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, 0, 32)   # cap = 0 counts
    assert rc == capi.APS_E_CAP and cnt == n and (desc == 0xA5).all()
    rc, cnt, *_ = _raw(gpu, img, prm, n, 32, with_out=False)   # desc = NULL counts
    assert cnt == n and rc == capi.APS_E_ARG    # features present and no output to put them in
    rc, cnt, *_ = _raw(gpu, img, prm, n, 31)
    assert rc == capi.APS_E_DIM   # the row width is 32
    rc, cnt, *_ = _raw(gpu, img, orb_params(capi, CAP_CASE, max_features=n - 1), n, 32)
    assert rc == capi.APS_E_CAP and cnt == n
    rc, cnt, desc, loc, aux = _raw(gpu, img, orb_params(capi, CAP_CASE, max_features=n), n, 32)
    assert rc == 0 and cnt == n
    assert_equals_mirror(desc, np.ascontiguousarray(loc[:, :n].T), aux, md, mloc, maux)
    # with a selection: cap below the rows kept writes nothing, cap = N suffices
    for select in (1, 2):
        prm = orb_params(capi, CAP_CASE, select, 100, 4, 4)
        rc, cnt, desc, loc, aux = _raw(gpu, img, prm, 99, 32)
        assert rc == capi.APS_E_CAP and cnt == 100 and (desc == 0xA5).all() and (loc == -7.5).all() and (aux == -7.5).all()
        rc, cnt, desc, loc, aux = _raw(gpu, img, prm, 100, 32)
        assert rc == 0 and cnt == 100 and not (desc == 0xA5).all(1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_padded_outputs_keep_their_padding(gpu, device):
    """ldd = 48 > 32 and ldl = cap + 5 > cap, cap > count: bytes between the rows, rows count..cap and the tail of loc stay the
    caller's, for host and for device pointers."""
    img, prm = pc.image(CAP_CASE), orb_params(gpu._capi, CAP_CASE)
    md, mloc, maux = pyramid_mirror(CAP_CASE)
    n = len(md)
    cap = n + 3
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, cap, 48, ldl=cap + 5, device=device)
    assert rc == 0 and cnt == n
    assert_equals_mirror(np.ascontiguousarray(desc[:n, :32]), np.ascontiguousarray(loc[:, :n].T), aux[:n], md, mloc, maux)
    assert (desc[:, 32:] == 0xA5).all() and (desc[n:] == 0xA5).all()
    assert (loc[:, n:] == -7.5).all() and (aux[n:] == -7.5).all()


@pytest.mark.gpu
def test_column_major_descriptors(gpu):
    capi = gpu._capi
    img, prm = pc.image(CAP_CASE), orb_params(capi, CAP_CASE)
    md, mloc, maux = pyramid_mirror(CAP_CASE)
    n = len(md)
    ld = n + 5
    rc, cnt, desc, loc, aux = _raw(gpu, img, prm, n, ld, layout=capi.APS_COLMAJOR, ldl=ld)
    assert rc == 0 and cnt == n and desc.shape == (32, ld)
    assert np.array_equal(desc[:, :n].T, md) and (desc[:, n:] == 0xA5).all()
    assert np.array_equal(loc[:, :n].T, mloc) and (loc[:, n:] == -7.5).all()
    rc, cnt, *_ = _raw(gpu, img, prm, n, n - 1, layout=capi.APS_COLMAJOR, ldl=n)
    assert rc == capi.APS_E_DIM


@pytest.mark.gpu
def test_resident_output_and_the_public_entries_equal_the_host_result(gpu, fm):
    import torch

    pl = import_module(gpu.__name__ + ".pipeline")
    par = import_module(gpu.__name__ + ".parallel")
    md, mloc, maux = pyramid_mirror(CAP_CASE)
    inp = pyramid_input(CAP_CASE)
    img = pc.image(CAP_CASE)
    dimg = torch.from_numpy(img.copy()).cuda()
    torch.cuda.synchronize()
    for compact in (False, True):
        f, pts = fm.fast_extract(inp, dimg, device_out=True, points_device=True, compact=compact)
        assert f.Features.is_cuda and pts.is_cuda and f.Features.dtype == torch.uint8 and f.NumBits == 256
        assert np.array_equal(f.Features.cpu().numpy(), md) and np.array_equal(pts.cpu().numpy(), mloc)
    for f, pts in (fm.getFeaturePoints(inp, img), fm.extract_features(inp, img)):
        assert np.array_equal(f.Features, md) and np.array_equal(pts, mloc)
    rgb = np.ascontiguousarray(np.repeat(img[:, :, None], 3, 2))
    drgb = [torch.from_numpy(rgb.copy()).cuda() for _ in range(2)]
    torch.cuda.synchronize()
    descs, kps = pl.extract_features(pl.default_input(**inp), drgb)
    many = pl.sift_many(pl.default_input(**inp), [rgb, rgb])
    futs = pl.sift_submit(pl.default_input(**inp), drgb)
    handle = par.submit_features(pl.default_input(**inp), {0: drgb[0], 1: drgb[1]})
    got = list(zip(descs, kps)) + many + [ft.result() for ft in futs] + [ft.result() for ft in handle["futures"]]
    assert len(got) == 8
    for d, p in got:
        assert isinstance(d, fm.binaryFeatures) and d.NumBits == 256
        D = d.Features.cpu().numpy() if hasattr(d.Features, "cpu") else d.Features
        P = p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p)
        assert np.array_equal(D, md) and np.array_equal(P, mloc)
    # SIFT and SURF ignore the key
    for det in ("SIFT", "SURF"):
        a, pa = fm.getFeaturePoints({"detector": det, "DescriptorMethod": "nonsense"}, rgb)
        b, pb = fm.getFeaturePoints({"detector": det}, rgb)
        assert np.array_equal(a, b) and np.array_equal(pa, pb)


# ---- groups of views -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_images():
    """Three views of one shape with very different contents: noise, the planted field, a flat field."""
    a = fc.noise_rects(41, 150, 200)
    b = fc.planted()[0].copy()
    c = np.full((150, 200), 33, np.uint8)
    return frozen((a, b, c))


def raw_batch(gpu, imgs, prm, caps, ldd=32, fill=0xA5):
    capi = gpu._capi
    g = len(imgs)
    h, w = imgs[0].shape[:2]
    views = (capi.aps_fast_view * g)()
    bufs = []
    ldl = max(max(caps), 1)   # (one ldl for the group)
    for k, img in enumerate(imgs):
        rows = max(caps[k], 1)
        bufs.append((np.ascontiguousarray(img), np.full((rows, ldd), fill, np.uint8), np.full((2, ldl), -7.5, np.float64),
                     np.full((rows, 4), -7.5, np.float32)))
        views[k].img, views[k].desc, views[k].loc, views[k].aux = [capi.ptr(a) for a in bufs[-1]]
        views[k].cap, views[k].count = caps[k], -1
    rc = capi.lib.aps_fast_orb_extract_batch(views, g, h, w, 1, capi.APS_IMG_U8_HWC, C.byref(prm), capi.APS_ROWMAJOR, ldd, ldl)
    return rc, [int(views[k].count) for k in range(g)], bufs


@pytest.mark.gpu
def test_group_of_three_views_equals_the_single_calls(gpu, fm):
    imgs = group_images()
    inp = {"detector": "FAST", "DescriptorMethod": "ORB", "MinContrast": 0.1, "NumLevels": 3}
    single = [fm.fast_extract(inp, img, want_aux=True) for img in imgs]
    for (f, loc, aux), img in zip(single, imgs):
        md, mloc, maux = om.extract(img, 3, 1.2, 0.1)
        assert_equals_mirror(f.Features, loc, aux, md, mloc, maux)
    assert [len(s[0]) for s in single][2] == 0 and all(len(s[0]) > 20 for s in single[:2])
    for order in ((0, 1, 2), (2, 1, 0), (1, 1, 0)):   # whatever the neighbours hold
        got = fm.fast_extract_batch(inp, [imgs[k] for k in order], want_aux=True)
        for k, (f, loc, aux) in zip(order, got):
            assert f.NumBits == 256 or len(f) == 0
            assert np.array_equal(f.Features, single[k][0].Features) and np.array_equal(u64(loc), u64(single[k][1]))
            assert np.array_equal(aux.view(np.uint32), single[k][2].view(np.uint32))


@pytest.mark.gpu
def test_group_with_one_view_too_small_writes_nothing_and_reports_every_count(gpu, fm):
    capi = gpu._capi
    imgs = group_images()
    need = [len(om.extract(img, 3, 1.2, 0.1)[0]) for img in imgs]
    prm = capi.aps_fast_pyramid_params(capi.aps_fast_params(25, 100000, 1000000, 0), 3, 1200000, 1000000)
    cap = max(need)
    rc, counts, bufs = raw_batch(gpu, imgs, prm, [cap, cap, cap])
    assert rc == 0 and counts == need
    good = [b[1][:n].copy() for b, n in zip(bufs, need)]
    small = min(k for k in range(3) if need[k] == cap)
    # one view a row short: nothing is written anywhere, every view reports what it needs
    rc, counts, bufs = raw_batch(gpu, imgs, prm, [cap - 1 if k == small else cap for k in range(3)], ldd=40)
    assert rc == capi.APS_E_CAP and counts == need
    for _, desc, loc, aux in bufs:
        assert (desc == 0xA5).all() and (loc == -7.5).all() and (aux == -7.5).all()
    rc, counts, bufs = raw_batch(gpu, imgs, prm, [cap, cap, cap], ldd=40)
    assert rc == 0 and counts == need
    for (_, desc, loc, aux), n, want in zip(bufs, need, good):
        assert np.array_equal(desc[:n, :32], want) and (desc[:, 32:] == 0xA5).all() and (desc[n:] == 0xA5).all()


# ---- matching at 32 bytes on real descriptors ------------------------------------------------------------------------------------------
SCENE_INP = {"detector": "FAST", "DescriptorMethod": "ORB", "MinContrast": 0.08}
THR, RATIO = 20.0, 0.6


@pytest.fixture(scope="module")
def scene_mirror():
    return [om.extract(v, MinContrast=0.08) for v in fc.scene()[0]]


@pytest.fixture(scope="module")
def scene_sets(fm, scene_mirror):
    out = [fm.getFeaturePoints(SCENE_INP, v) for v in fc.scene()[0]]
    for (f, pts), (md, mloc, _) in zip(out, scene_mirror):
        assert f.Features.shape[1] == 32 and np.array_equal(f.Features, md) and np.array_equal(pts, mloc)
    return out


@pytest.mark.gpu
def test_matchers_on_32_byte_rows_equal_the_numpy_restatements(fm, scene_sets, scene_mirror):
    assert [len(s[0]) for s in scene_mirror] == [227, 220, 220]
    descs = [s[0] for s in scene_sets]
    got = fm.featureMatchingPairwise({"Matchingthreshold": THR, "Ratiothreshold": RATIO}, descs, 3)
    for i in range(3):
        for j in range(3):
            if i < j:
                wm, _ = fc.match_binary(scene_mirror[i][0], scene_mirror[j][0], RATIO, THR)
                assert got[i][j].dtype == np.float64 and np.array_equal(got[i][j], wm.astype(np.float64)), (i, j)
            else:
                assert got[i][j] is None
    assert [len(got[0][1]), len(got[0][2]), len(got[1][2])] == [73, 41, 76]   # (FREAK: 80 / 44 / 82)
    for bf in (0, 1):
        got = fm.featureMatchingGlobal({"Ratiothreshold": 0.8, "k": 4, "BFMatch": bf}, descs, 3)
        want = fc.global_binary([s[0] for s in scene_mirror], 0.8, 4)
        assert sum(len(v) for v in want.values()) > 100
        for i in range(3):
            for j in range(3):
                if (i, j) in want:
                    assert np.array_equal(got[i][j], want[(i, j)]), (bf, i, j)
                else:
                    assert got[i][j] is None


@pytest.mark.gpu
def test_stitch_of_the_scene(gpu):
    pl = import_module(gpu.__name__ + ".pipeline")
    views, cams = fc.scene()
    inp = pl.default_input(**SCENE_INP, Matchingthreshold=THR, resizeImage=0)
    panos, info = pl.stitch(inp, views, Ks=[c["K"] for c in cams], tile=(512, 512))
    assert info["n_features"] == [227, 220, 220]
    assert info["n_components"] == 1 and len(panos) == 1 and sorted(info["components"][0]["members"]) == [0, 1, 2]
    assert [int(info["putative"][i, j]) for (i, j) in ((0, 1), (0, 2), (1, 2))] == [73, 41, 76]
    pano = panos[0].cpu().numpy() if hasattr(panos[0], "cpu") else np.asarray(panos[0])
    assert pano.ndim == 3 and (pano.max(axis=2) > 0).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [{}, {"NumStrongest": 300}, {"NumUniform": 300}], ids=["all", "strongest", "uniform"])
def test_stitch_over_three_levels_runs_with_and_without_a_selection(gpu, extra):
    pl = import_module(gpu.__name__ + ".pipeline")
    views, cams = fc.scene()
    inp = pl.default_input(detector="FAST", DescriptorMethod="ORB", NumLevels=3, Matchingthreshold=20, MinContrast=0.08, resizeImage=0, **extra)
    panos, info = pl.stitch(inp, views, Ks=[c["K"] for c in cams], tile=(512, 512))
    assert all(n > 227 for n in info["n_features"]) if not extra else all(200 < n <= 300 for n in info["n_features"])
    assert len(panos) >= 1 and info["n_components"] >= 1


# ---- the twin pair: B is level 2 of A --------------------------------------------------------------------------------------
def rgb(g):
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))   # (rgb2gray's integer plane of a gray triple is the gray value)


@pytest.mark.gpu
def test_twin_pair_matches_at_metric_zero_and_stitches_to_one_panorama(gpu, fm):
    pl = import_module(gpu.__name__ + ".pipeline")
    A, B = pc.twin_images()
    inp = {"detector": "FAST", "DescriptorMethod": "ORB", "MinContrast": pc.TWIN_MC}
    f3, l3, a3 = fm.fast_extract({**inp, "NumLevels": pc.TWIN_LEVELS, "ScaleFactor": pc.TWIN_SCALE}, A, want_aux=True)
    fb, lb, ab = fm.fast_extract(inp, B, want_aux=True)
    at2 = np.flatnonzero(a3[:, 2] == 2)
    assert len(at2) == len(fb) == 728 and np.array_equal(f3.Features[at2], fb.Features)
    m, d = fm.matchFeaturesScratch(f3, fb, MatchThreshold=10.0, MaxRatio=0.6)
    got = {(int(i), int(j)): float(v) for (i, j), v in zip(m, d)}
    assert all(got.get((int(at2[t]) + 1, t + 1)) == 0.0 for t in range(728))   # every twin, at metric 0
    sinp = pl.default_input(detector="FAST", DescriptorMethod="ORB", NumLevels=pc.TWIN_LEVELS, MinContrast=pc.TWIN_MC, Matchingthreshold=20,
                            resizeImage=0)
    f = 450.0   # B is A seen at 167 / 240 of the focal length, same direction
    Ks = [np.array([[f * s, 0, w / 2.0], [0, f * s, h / 2.0], [0, 0, 1.0]]) for (h, w), s in ((A.shape, 1.0), (B.shape, 167.0 / 240.0))]
    panos, info = pl.stitch(sinp, [rgb(A), rgb(B)], Ks=Ks, tile=(512, 512))
    assert info["n_features"][0] == 4673 and info["n_features"][1] > 728   # (the FREAK call's counts: B's own three levels)
    assert info["n_components"] == 1 and len(panos) == 1 and sorted(info["components"][0]["members"]) == [0, 1]
    pano = panos[0].cpu().numpy() if hasattr(panos[0], "cpu") else np.asarray(panos[0])
    assert pano.ndim == 3 and (pano.max(axis=2) > 0).mean() > 0.5
