"""Device FAST/FREAK against the NumPy mirror of the contract (tests/fast_mirror.py): count, locations, aux and every
descriptor byte equal - everything is integer arithmetic, so there is no tolerance anywhere.

Shapes are the smallest at which each kernel can go wrong.  Keypoints the mirror alone finds on each (checked device-free,
test_cases_have_keypoints): 47x49: 1, 64x64: 81, 70x131: 131, 129x1030: 1082, 200x300x3: 87, planted: 22, flat: 0.  Every
non-degenerate shape carries at least 50.  47x49 is the degenerate shape: pixels at least 23 from every edge are its whole
admissible area, 1 row of 3, which cannot hold 50 keypoints - it is there for that single row of candidates.  64x64 has
18 x 18 admissible pixels, too few for noise (strict 3 x 3 maxima of noise have a density near 1/9), so its image plants the
densest lattice of maxima into the noise (fast_cases.noise_lattice).  planted and flat are exact by construction."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import fast_cases as fc
import fast_mirror as fmir

DEGENERATE = "47x49"   # 1 x 3 admissible pixels: exempt from the bound of 50, it only has to have a keypoint
# name: (image builder, MinContrast, least keypoints) - what it catches
CASES = {
    "47x49": (lambda: fc.noise_rects(11, 47, 49), 0.05, None),          # barely larger than twice the margin: one row of candidates
    "64x64": (lambda: fc.noise_lattice(12, 64, 64), 0.05, 50),          # one tile column, one bitmap word per row
    "70x131": (lambda: fc.noise_rects(13, 70, 131), 0.1, 50),           # tile and 64-bit word boundaries not aligned
    "129x1030": (lambda: fc.noise_rects(14, 129, 1030), 0.2, 50),       # crosses the 1024-px row-scan chunk and the 64-row column chunk
    "200x300x3": (lambda: fc.noise_rects(15, 200, 300, 3), 0.2, 50),    # RGB
    "planted": (lambda: fc.planted()[0], 0.2, 22),                      # corners on tile seams and the first / last admissible row and column
    "flat": (lambda: np.full((90, 100), 77, np.uint8), 0.2, 0),
}
_MIRROR = {}


def mirror(name):
    """The mirror's result for a case, computed once and shared (read-only)."""
    if name not in _MIRROR:
        build, mc, _ = CASES[name]
        img = build()
        out = fmir.extract(img, fc.tables(), MinContrast=mc)
        for a in out:
            a.setflags(write=False)
        _MIRROR[name] = (img, mc) + out
    return _MIRROR[name]


@pytest.mark.parametrize("name", list(CASES))
def test_cases_have_keypoints(name):
    """Device-free: the images carry what the comparison needs."""
    n = len(mirror(name)[2])
    assert (n == 0) == (name == "flat"), n
    if name != DEGENERATE:
        assert n >= CASES[name][2], n
    if name == "planted":
        _, _, _, loc, aux = mirror(name)
        assert [(int(y - 1), int(x - 1), int(s)) for (x, y), s in zip(loc, aux[:, 0])] == fc.planted()[1]


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def assert_equals_mirror(d, loc, aux, md, mloc, maux):
    assert d.shape == md.shape and loc.shape == mloc.shape and aux.shape == maux.shape, (d.shape, md.shape)
    assert d.dtype == np.uint8 and loc.dtype == np.float64 and aux.dtype == np.float32
    assert np.array_equal(loc, mloc), "locations / keypoint order"
    assert np.array_equal(aux[:, 0], maux[:, 0]), "scores"
    assert np.array_equal(aux[:, 1], maux[:, 1]), "orientation bins (%d differ)" % int((aux[:, 1] != maux[:, 1]).sum())
    assert not aux[:, 2:].any()
    assert np.array_equal(d, md), "descriptor bytes (%d rows differ)" % int((d != md).any(1).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_mirror(fm, name):
    img, mc, md, mloc, maux = mirror(name)
    f, loc, aux = fm.fast_extract({"detector": "FAST", "MinContrast": mc}, img, want_aux=True)
    assert isinstance(f, fm.binaryFeatures) and f.NumBits == 512 and f.NumFeatures == len(md)
    assert_equals_mirror(f.Features, loc, aux, md, mloc, maux)
    if name == "flat":
        assert f.Features.shape == (0, 64) and loc.shape == (0, 2)


def _raw(gpu, img, cap, ldd, mc=0.2, layout=None, ldl=None, fill=0xA5, device=False, with_out=True, matlab=False, max_features=0):
    capi = gpu._capi
    layout = capi.APS_ROWMAJOR if layout is None else layout
    prm = capi.aps_fast_params(int(np.floor(mc * 255)), 100000, 1000000, max_features)
    h, w, ch = img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3
    if matlab:   # planar, column-major: element (y, x, q) at q * h * w + x * h + y
        img = img.T if img.ndim == 2 else img.transpose(2, 1, 0)
    rows = max(cap, 1)
    ldl = rows if ldl is None else ldl
    desc = np.full((rows, ldd) if layout == capi.APS_ROWMAJOR else (64, ldd), fill, np.uint8)
    loc = np.full((2, ldl), -7.5, np.float64)
    aux = np.full((rows, 4), -7.5, np.float32)
    cnt = C.c_int64(-1)
    img = np.ascontiguousarray(img)
    args = [img, desc, loc, aux]
    if device:
        import torch

        args = [torch.from_numpy(a).cuda() for a in args]
        torch.cuda.synchronize()
    pi, pd, pl, pa = [capi.ptr(a) for a in args]
    if not with_out:
        pd = pl = pa = None
    rc = capi.lib.aps_fast_extract(pi, h, w, ch, capi.APS_IMG_U8_MATLAB if matlab else capi.APS_IMG_U8_HWC, C.byref(prm),
                                   pd, layout, ldd, pl, ldl, pa, cap, C.byref(cnt))
    if device:
        capi.check(capi.lib.aps_synchronize())
        desc, loc, aux = [a.cpu().numpy() for a in args[1:]]
    return rc, cnt.value, desc, loc, aux


@pytest.mark.gpu
def test_capacity_too_small_reports_the_count_and_count_only_mode(gpu):
    img, mc, md, mloc, maux = mirror("200x300x3")
    n = len(md)
    rc, cnt, *_ = _raw(gpu, img, 8, 64)
    assert rc == gpu._capi.APS_E_CAP and cnt == n
    rc, cnt, desc, loc, aux = _raw(gpu, img, 0, 64)   # cap = 0 counts
    assert rc == gpu._capi.APS_E_CAP and cnt == n and (desc == 0xA5).all()
    rc, cnt, *_ = _raw(gpu, img, n, 64, with_out=False)   # desc = NULL counts
    assert cnt == n and rc == gpu._capi.APS_E_ARG    # features present and no output to put them in
    rc, cnt, desc, loc, aux = _raw(gpu, img, n, 64)
    assert rc == 0 and cnt == n
    assert_equals_mirror(desc, np.ascontiguousarray(loc[:, :n].T), aux, md, mloc, maux)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_padded_outputs_keep_their_padding(gpu, device):
    """ldd = 80 > 64 and ldl = cap + 5 > cap, cap > count: bytes between the rows, rows count..cap and the tail of loc stay
    the caller's, for host and for device pointers."""
    img, mc, md, mloc, maux = mirror("70x131")
    n = len(md)
    cap = n + 3
    rc, cnt, desc, loc, aux = _raw(gpu, img, cap, 80, mc=mc, ldl=cap + 5, device=device)
    assert rc == 0 and cnt == n
    assert_equals_mirror(np.ascontiguousarray(desc[:n, :64]), np.ascontiguousarray(loc[:, :n].T), aux[:n], md, mloc, maux)
    assert (desc[:, 64:] == 0xA5).all() and (desc[n:] == 0xA5).all()
    assert (loc[:, n:] == -7.5).all() and (aux[n:] == -7.5).all()


@pytest.mark.gpu
def test_column_major_descriptors(gpu):
    capi = gpu._capi
    img, mc, md, mloc, maux = mirror("70x131")
    n = len(md)
    ld = n + 5
    rc, cnt, desc, loc, aux = _raw(gpu, img, n, ld, mc=mc, layout=capi.APS_COLMAJOR, ldl=ld)
    assert rc == 0 and cnt == n and desc.shape == (64, ld)
    assert np.array_equal(desc[:, :n].T, md) and (desc[:, n:] == 0xA5).all()
    assert np.array_equal(loc[:, :n].T, mloc) and (loc[:, n:] == -7.5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["70x131", "200x300x3"])
def test_matlab_layout_images(gpu, name):
    """Planar, column-major pixels (gray and RGB) give what the interleaved row-major image gives."""
    img, mc, md, mloc, maux = mirror(name)
    n = len(md)
    rc, cnt, desc, loc, aux = _raw(gpu, img, n, 64, mc=mc, matlab=True)
    assert rc == 0 and cnt == n
    assert_equals_mirror(desc, np.ascontiguousarray(loc.T), aux, md, mloc, maux)


@pytest.mark.gpu
def test_max_features_is_a_limit_on_the_count(gpu):
    """params.max_features > 0 below the count: APS_E_CAP with the count, whatever the capacity; at the count: no limit hit."""
    img, mc, md, mloc, maux = mirror("70x131")
    n = len(md)
    rc, cnt, *_ = _raw(gpu, img, n, 64, mc=mc, max_features=n - 1)
    assert rc == gpu._capi.APS_E_CAP and cnt == n
    rc, cnt, desc, loc, aux = _raw(gpu, img, n, 64, mc=mc, max_features=n)
    assert rc == 0 and cnt == n
    assert_equals_mirror(desc, np.ascontiguousarray(loc.T), aux, md, mloc, maux)


@pytest.mark.gpu
def test_resident_output_equals_host_output(fm):
    import torch

    img, mc, md, mloc, maux = mirror("200x300x3")
    inp = {"detector": "FAST", "MinContrast": mc}
    dimg = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    torch.cuda.synchronize()
    for compact in (False, True):
        f, pts = fm.fast_extract(inp, dimg, device_out=True, points_device=True, compact=compact)
        assert f.Features.is_cuda and pts.is_cuda and f.Features.dtype == torch.uint8
        assert np.array_equal(f.Features.cpu().numpy(), md) and np.array_equal(pts.cpu().numpy(), mloc)
    f, pts = fm.getFeaturePoints(inp, img)
    assert np.array_equal(f.Features, md) and np.array_equal(pts, mloc)


_DENSE = []


def dense_mirror():
    """The mirror's result on sift_param_cases.dense_image() (300 x 400) at MinContrast 0.05, MinQuality 0: 4910 corners, more
    than the wrapper's first capacity max(4096, h w / 64) = 4096.  Computed once, shared, read-only."""
    if not _DENSE:
        import sift_param_cases as sc

        out = fmir.extract(sc.dense_image(), fc.tables(), MinContrast=0.05, MinQuality=0)
        for a in out:
            a.setflags(write=False)
        _DENSE.append((sc.dense_image(),) + out)
    return _DENSE[0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device_out", "device_points_compact"])
def test_wrapper_grows_its_capacity_and_retries(fm, mode):
    """More corners than the first capacity: the first call reports APS_E_CAP with the count, the wrapper allocates that many
    rows and calls again; rows, points and aux are the mirror's."""
    img, md, mloc, maux = dense_mirror()
    assert len(md) > 4096 == max(4096, img.shape[0] * img.shape[1] // 64)
    inp = {"detector": "FAST", "MinContrast": 0.05, "MinQuality": 0}
    if mode == "host":
        f, pts, aux = fm.fast_extract(inp, img, want_aux=True)
        d = f.Features
    else:
        more = dict(points_device=True, compact=True) if mode == "device_points_compact" else {}
        f, pts, aux = fm.fast_extract(inp, img, device_out=True, want_aux=True, **more)
        assert f.Features.is_cuda and (mode == "device_out" or pts.is_cuda)
        if mode == "device_points_compact":
            assert f.Features.numel() == f.Features.untyped_storage().nbytes(), "compact=True returns a right-sized buffer"
            pts = pts.cpu().numpy()
        d = f.Features.cpu().numpy()
    assert isinstance(f, fm.binaryFeatures) and f.NumFeatures == len(md)
    assert_equals_mirror(d, pts, aux, md, mloc, maux)
