"""GPU parity of aps_sift_extract_batch: a group of views through one chain gives, view by view, the bits of the oracle (and so
of aps_sift_extract).  Images: test_sift_gpu.textured seeded 1000 + k for view k.  The oracle's counts for these seeds - 97x131:
252-285 over 9 views, 120x160: 415-420, 35x47: 22-28, 64x200: 226 and 271 - so no comparison below is vacuous."""
import ctypes as C
import threading
from importlib import import_module

import numpy as np
import pytest

import oracle
from test_sift_gpu import INPUT, textured

pytestmark = pytest.mark.gpu

_ORACLE = {}


def view(k, h, w):
    return textured(np.random.default_rng(1000 + k), h, w)


def ref(k, h, w, **prm):
    """oracle.sift of view k, computed once per (view, shape, parameters)."""
    key = (k, h, w, tuple(sorted(prm.items())))
    if key not in _ORACLE:
        p = dict(INPUT, **prm)
        _ORACLE[key] = oracle.sift(view(k, h, w), p["Sigma"], p["NumLayersInOctave"], p["ContrastThreshold"], p["EdgeThreshold"])
    return _ORACLE[key]


def same(got, want):
    """descriptors, locations and aux, bit for bit"""
    f, pts, aux = got
    od, ol, oa = want
    return (f.shape == od.shape and np.array_equal(f.view(np.uint32), od.view(np.uint32)) and np.array_equal(pts, ol)
            and np.array_equal(aux.view(np.uint32), oa.view(np.uint32)))


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def call_batch(gpu, imgs, caps, prm=None, layout=None, ldd=128, ldl=None, descs=None, locs=None, auxs=None, n_views=None):
    """The C entry on host or device buffers: returns (rc, counts, descs, locs, auxs)."""
    capi = gpu._capi
    g = len(imgs)
    layout = capi.APS_ROWMAJOR if layout is None else layout
    ldl = max(caps) if ldl is None else ldl
    p = fm_params(gpu, prm or {})
    descs = descs or [np.zeros((c, 128) if layout == capi.APS_ROWMAJOR else (128, ldd), np.float32) for c in caps]
    locs = locs or [np.zeros((2, ldl), np.float64) for _ in caps]
    auxs = auxs or [np.zeros((max(c, 1), 4), np.float32) for c in caps]
    views = (capi.aps_sift_view * max(g, 1))()
    for k in range(g):
        views[k].img, views[k].desc, views[k].loc, views[k].aux = capi.ptr(imgs[k]), capi.ptr(descs[k]), capi.ptr(locs[k]), capi.ptr(auxs[k])
        views[k].cap, views[k].count = caps[k], -1
    h, w = imgs[0].shape[:2]
    rc = capi.lib.aps_sift_extract_batch(views, g if n_views is None else n_views, h, w, 3, capi.APS_IMG_U8_HWC, C.byref(p), layout, ldd, ldl)
    capi.check(capi.lib.aps_synchronize())
    return rc, [int(views[k].count) for k in range(g)], descs, locs, auxs


def fm_params(gpu, prm):
    return import_module(gpu.__name__ + ".featureMatching")._sift_params(dict(INPUT, **prm))


def rows(desc, loc, aux, n):
    return np.ascontiguousarray(desc[:n]), np.ascontiguousarray(loc[:, :n].T), aux[:n]


@pytest.mark.parametrize("h,w,g", [(97, 131, 9), (120, 160, 3), (35, 47, 3), (64, 200, 2)])
def test_batch_equals_oracle_and_groups_of_one(fm, h, w, g):
    """(97 x 131: odd sides - the scalar store branch, reflected rims, odd halved octaves - and one view more than a group of 8.)"""
    imgs = [view(k, h, w) for k in range(g)]
    got = fm.sift_extract_batch(INPUT, imgs, want_aux=True)
    for k in range(g):
        assert len(ref(k, h, w)[0]) >= 20
        assert same(got[k], ref(k, h, w)), f"view {k} differs from the oracle"
        assert same(fm.sift_extract_batch(INPUT, [imgs[k]], want_aux=True)[0], got[k]), f"view {k} differs from its group of one"


def test_constant_middle_view(fm):
    imgs = [view(0, 97, 131), np.full((97, 131, 3), 128, np.uint8), view(2, 97, 131)]
    got = fm.sift_extract_batch(INPUT, imgs, want_aux=True)
    assert got[1][0].shape == (0, 128) and got[1][1].shape == (0, 2)
    assert same(got[0], ref(0, 97, 131)) and same(got[2], ref(2, 97, 131))


@pytest.mark.parametrize("prm", [{"Sigma": 1.6, "NumLayersInOctave": 3, "ContrastThreshold": 0.0133, "EdgeThreshold": 10},
                                 {"Sigma": 2.0, "NumLayersInOctave": 2, "ContrastThreshold": 0.001, "EdgeThreshold": 12}])
def test_other_layer_counts(fm, prm):
    imgs = [view(k, 97, 131) for k in range(2)]
    got = fm.sift_extract_batch(dict(INPUT, **prm), imgs, want_aux=True)
    for k in range(2):
        assert len(ref(k, 97, 131, **prm)[0]) >= 10
        assert same(got[k], ref(k, 97, 131, **prm))


def test_capacity_reports_every_count_and_one_retry_suffices(gpu):
    imgs = [view(k, 97, 131) for k in range(3)]
    want = [len(ref(k, 97, 131)[0]) for k in range(3)]
    rc, counts, *_ = call_batch(gpu, imgs, [4096, 10, 4096])
    assert rc == gpu._capi.APS_E_CAP and counts == want
    rc, counts, descs, locs, auxs = call_batch(gpu, imgs, counts)
    assert rc == 0 and counts == want
    for k in range(3):
        assert same(rows(descs[k], locs[k], auxs[k], counts[k]), ref(k, 97, 131))


def test_candidate_capacity(gpu):
    imgs = [view(k, 97, 131) for k in range(2)]
    rc, *_ = call_batch(gpu, imgs, [4096, 4096], prm={"maxFeatures": 50})
    assert rc == gpu._capi.APS_E_CAP
    cnt = C.c_int64(0)
    p = fm_params(gpu, {"maxFeatures": 50})
    d, l = np.zeros((4096, 128), np.float32), np.zeros((2, 4096), np.float64)
    single = gpu.lib.aps_sift_extract(gpu._capi.ptr(imgs[0]), 97, 131, 3, gpu._capi.APS_IMG_U8_HWC, C.byref(p), gpu._capi.ptr(d),
                                      gpu._capi.APS_ROWMAJOR, 128, gpu._capi.ptr(l), 4096, None, 4096, C.byref(cnt))
    assert single == gpu._capi.APS_E_CAP


def test_layouts_host_device_and_padded_column_major(gpu):
    import torch

    capi = gpu._capi
    imgs = [view(k, 97, 131) for k in range(3)]
    want = [ref(k, 97, 131) for k in range(3)]
    n = [len(wk[0]) for wk in want]
    # device-resident inputs and outputs
    timgs = [torch.from_numpy(im).cuda() for im in imgs]
    td = [torch.zeros((512, 128), dtype=torch.float32, device="cuda") for _ in range(3)]
    tl = [torch.zeros((2, 512), dtype=torch.float64, device="cuda") for _ in range(3)]
    ta = [torch.zeros((512, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    rc, counts, *_ = call_batch(gpu, timgs, [512] * 3, descs=td, locs=tl, auxs=ta)
    assert rc == 0 and counts == n
    for k in range(3):
        assert same(rows(td[k].cpu().numpy(), tl[k].cpu().numpy(), ta[k].cpu().numpy(), n[k]), want[k])
    # host inputs, column-major descriptors with ldd > count and ldl > count: the padding stays the caller's
    ldd, ldl = 517, 523
    descs = [np.full((128, ldd), -7.0, np.float32) for _ in range(3)]
    locs = [np.full((2, ldl), -7.0, np.float64) for _ in range(3)]
    rc, counts, descs, locs, auxs = call_batch(gpu, imgs, [512] * 3, layout=capi.APS_COLMAJOR, ldd=ldd, ldl=ldl, descs=descs, locs=locs)
    assert rc == 0 and counts == n
    for k in range(3):
        assert same((np.ascontiguousarray(descs[k][:, :n[k]].T), np.ascontiguousarray(locs[k][:, :n[k]].T), auxs[k][:n[k]]), want[k])
        assert np.all(descs[k][:, n[k]:] == -7.0) and np.all(locs[k][:, n[k]:] == -7.0)
    # the same with the buffers on the device
    td = [torch.full((128, ldd), -7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    tl = [torch.full((2, ldl), -7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    rc, counts, *_ = call_batch(gpu, timgs, [512] * 3, layout=capi.APS_COLMAJOR, ldd=ldd, ldl=ldl, descs=td, locs=tl, auxs=ta)
    assert rc == 0 and counts == n
    for k in range(3):
        assert np.array_equal(td[k].cpu().numpy().view(np.uint32), descs[k].view(np.uint32))
        assert np.array_equal(tl[k].cpu().numpy(), locs[k])


def test_sift_many_groups_by_shape_and_repeats(gpu, fm):
    import torch

    pl = import_module(gpu.__name__ + ".pipeline")
    shapes = [(97, 131)] * 9 + [(64, 200)] * 2
    imgs = [view(k if k < 9 else k - 9, h, w) for k, (h, w) in enumerate(shapes)]
    timgs = [torch.from_numpy(im).cuda() for im in imgs]
    first = pl.sift_many(INPUT, timgs)
    again = pl.sift_many(INPUT, timgs)
    for k, t in enumerate(timgs):
        d, pts = fm.sift_extract(INPUT, t, device_out=True)
        for got in (first[k], again[k]):
            assert got[0].is_cuda and torch.equal(got[0], d) and np.array_equal(np.asarray(got[1]), pts)


def test_two_host_threads(gpu, fm):
    res = {}

    def run(t):
        gpu._capi.check(gpu.lib.aps_set_thread_device(gpu.lib.aps_get_device()))
        res[t] = fm.sift_extract_batch(INPUT, [view(4 * t + k, 97, 131) for k in range(4)], want_aux=True)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in range(2):
        for k in range(4):
            assert same(res[t][k], ref(4 * t + k, 97, 131))


def test_argument_checks(gpu):
    capi = gpu._capi
    imgs = [view(0, 35, 47)]
    assert call_batch(gpu, imgs, [64], n_views=0)[0] == capi.APS_E_ARG
    assert call_batch(gpu, imgs, [64], n_views=capi.APS_SIFT_MAX_VIEWS + 1)[0] == capi.APS_E_ARG
    p = fm_params(gpu, {})
    assert capi.lib.aps_sift_extract_batch(None, 1, 35, 47, 3, capi.APS_IMG_U8_HWC, C.byref(p), capi.APS_ROWMAJOR, 128, 64) == capi.APS_E_ARG
    views = (capi.aps_sift_view * 1)()  # (a view without an image)
    assert capi.lib.aps_sift_extract_batch(views, 1, 35, 47, 3, capi.APS_IMG_U8_HWC, C.byref(p), capi.APS_ROWMAJOR, 128, 64) == capi.APS_E_ARG


@pytest.mark.parametrize("resident", [False, True])
def test_wrapper_grows_every_view_when_one_exceeds_its_capacity(fm, resident):
    """Two 300 x 400 gray views, first capacity max(4096, h w / 64) = 4096 each: sift_param_cases.dense_image() has 6367 oracle
    features, gray_image(300, 400) 2951.  One view over its capacity makes the wrapper allocate the largest count for every view
    and call again; every view's result is sift_extract's of that view, bit for bit."""
    import sift_param_cases as sc

    imgs = [sc.dense_image(), sc.gray_image(300, 400)]
    kw = dict(device_out=True, points_device=True, compact=True) if resident else {}
    got = fm.sift_extract_batch(INPUT, imgs, want_aux=True, **kw)
    want = [fm.sift_extract(INPUT, im, want_aux=True, **kw) for im in imgs]
    if resident:
        assert all(r[0].is_cuda and r[1].is_cuda for r in got)
        assert all(r[0].numel() * 4 == r[0].untyped_storage().nbytes() for r in got), "compact=True returns right-sized buffers"
        got = [(f.cpu().numpy(), p.cpu().numpy(), a) for f, p, a in got]
        want = [(f.cpu().numpy(), p.cpu().numpy(), a) for f, p, a in want]
    assert max(len(r[0]) for r in got) > 4096 == max(4096, 300 * 400 // 64), "no view exceeds the first capacity"
    for k in range(2):
        assert len(got[k][0]) >= 20
        assert same(got[k], want[k]), f"view {k} differs from sift_extract"
