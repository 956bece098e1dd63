"""Device FAST/FREAK in groups of views (aps_fast_extract_batch) against the NumPy mirrors of the contract (tests/fast_mirror.py,
tests/fast_pyramid_mirror.py) and against the single-view entries, byte for byte: descriptors, locations as f64 bits and aux
(score, bin, level) - integer arithmetic throughout, so there is no tolerance anywhere.  Groups (views of one shape):
  seams    fast_cases.planted(150, 200) beside two noise_rects(seed, 150, 200): corners on the tile and bitmap-word seams
  nine     9 views of noise_rects at 120 x 160: one view more than 8
  lattice  noise_lattice at 64 x 64: a barely admissible plane (18 x 18 pixels are far enough from the edge)
  flat     a flat view between two textured ones: no rows, neighbours intact
Plans: NumLevels 1 and 3 at ScaleFactor 1.2, and NumLevels 4 at 1.5 on 150 x 200, where the plan ends after three levels.
Every comparison first asserts that the expected result holds at least 20 rows per view."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import fast_cases as fc
import fast_mirror as fmir
import fast_pyramid_mirror as pmir

pytestmark = pytest.mark.gpu

GROUPS = {
    "seams": lambda: [fc.planted(150, 200)[0], fc.noise_rects(11, 150, 200), fc.noise_rects(12, 150, 200)],
    "nine": lambda: [fc.noise_rects(100 + k, 120, 160) for k in range(9)],
    "lattice": lambda: [fc.noise_lattice(s) for s in (1, 2, 3)],
}
PLANS = [("seams", 1, 1.2), ("seams", 3, 1.2), ("seams", 4, 1.5), ("nine", 1, 1.2), ("nine", 3, 1.2), ("lattice", 1, 1.2), ("lattice", 3, 1.2)]
FILL = 0xA5
_IMAGES, _MIRROR = {}, {}


def images(name):
    if name not in _IMAGES:
        _IMAGES[name] = GROUPS[name]()
        for a in _IMAGES[name]:
            a.setflags(write=False)
    return _IMAGES[name]


def mirror(gpu, name, nl, sf):
    """The mirror's (desc, loc, aux) of every view of a group, computed once and shared (read-only); at least 20 rows each."""
    if (name, nl, sf) not in _MIRROR:
        tb = fmir.load_tables(gpu._capi)
        _MIRROR[name, nl, sf] = [pmir.extract(img, tb, NumLevels=nl, ScaleFactor=sf) for img in images(name)]
        for out in _MIRROR[name, nl, sf]:
            assert len(out[0]) >= 20, "the case must have keypoints to compare"
            for a in out:
                a.setflags(write=False)
    return _MIRROR[name, nl, sf]


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def assert_same_bytes(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def fast_params(capi, nl=1, sf=1.2, max_features=0):
    num, den = pmir.scale_rational(sf)
    return capi.aps_fast_pyramid_params(capi.aps_fast_params(51, 100000, 1000000, max_features), nl, num, den)


def run_batch(gpu, imgs, caps, prm, ldd=64, colmajor=False, device=False, count_only=()):
    """The raw group call on FILL-ed outputs of caps[k] rows (column-major: ldd = ldl = max cap): (rc, counts, [(desc, loc, aux)]).
    device: images and outputs are resident tensors, handed back as numpy copies.  count_only: views that pass no outputs."""
    capi = gpu._capi
    g, most = len(imgs), max(max(caps), 1)
    if colmajor:
        ldd = most
    keep, bufs = [], []
    if device:
        import torch
    for k, img in enumerate(imgs):
        img = np.ascontiguousarray(img)
        cap = max(caps[k], 1)
        desc = np.full((64, ldd) if colmajor else (cap, ldd), FILL, np.uint8)
        loc = np.full((2, most), -7.5, np.float64)
        aux = np.full((cap, 4), -7.5, np.float32)
        if device:
            img, desc, loc, aux = (torch.tensor(a).cuda() for a in (img, desc, loc, aux))
        keep.append(img)
        bufs.append((desc, loc, aux))
    if device:
        torch.cuda.synchronize()
    views = (capi.aps_fast_view * g)()
    for k in range(g):
        out = (None, None, None) if k in count_only else bufs[k]
        views[k].img, views[k].desc, views[k].loc, views[k].aux = (capi.ptr(keep[k]),) + tuple(capi.ptr(a) for a in out)
        views[k].cap, views[k].count = caps[k], -1
    h, w = imgs[0].shape[:2]
    rc = capi.lib.aps_fast_extract_batch(views, g, h, w, 1 if imgs[0].ndim == 2 else 3, capi.APS_IMG_U8_HWC, C.byref(prm),
                                         capi.APS_COLMAJOR if colmajor else capi.APS_ROWMAJOR, ldd, most)
    if device:
        capi.check(capi.lib.aps_synchronize())
        bufs = [tuple(a.cpu().numpy() for a in b) for b in bufs]
    return rc, [int(views[k].count) for k in range(g)], bufs


def rows_of(buf, n, colmajor=False):
    desc, loc, aux = buf
    return (np.ascontiguousarray(desc[:, :n].T) if colmajor else desc[:n, :64]), np.ascontiguousarray(loc[:, :n].T), aux[:n]


def run_single(gpu, prm, img, cap):
    capi = gpu._capi
    img = np.ascontiguousarray(img)
    desc, loc, aux = np.full((cap, 64), FILL, np.uint8), np.full((2, cap), -7.5, np.float64), np.full((cap, 4), -7.5, np.float32)
    cnt = C.c_int64(-1)
    capi.check(capi.lib.aps_fast_extract_pyramid(capi.ptr(img), img.shape[0], img.shape[1], 1, capi.APS_IMG_U8_HWC, C.byref(prm),
                                                 capi.ptr(desc), capi.APS_ROWMAJOR, 64, capi.ptr(loc), cap, capi.ptr(aux), cap, C.byref(cnt)))
    return rows_of((desc, loc, aux), cnt.value)


@pytest.mark.parametrize("name, nl, sf", PLANS)
def test_every_view_equals_the_mirror_and_the_single_view_entry(gpu, fm, name, nl, sf):
    imgs, want = images(name), mirror(gpu, name, nl, sf)
    need = [len(w[0]) for w in want]
    prm = fast_params(gpu._capi, nl, sf)
    rc, counts, bufs = run_batch(gpu, imgs, [n + 2 for n in need], prm)
    assert rc == 0 and counts == need
    inp = {"detector": "FAST", "NumLevels": nl, "ScaleFactor": sf}
    wrapped = fm.fast_extract_batch(inp, imgs, want_aux=True)
    for k, img in enumerate(imgs):
        got = rows_of(bufs[k], need[k])
        assert_same_bytes(got, want[k])
        assert_same_bytes(got, run_single(gpu, prm, img, need[k]))
        assert (bufs[k][0][need[k]:] == FILL).all() and (bufs[k][2][need[k]:] == -7.5).all(), "rows beyond the count belong to the caller"
        f, pts, aux = wrapped[k]
        assert isinstance(f, fm.binaryFeatures)
        assert_same_bytes((f.Features, pts, aux), got)
        f1, pts1, aux1 = fm.fast_extract(inp, img, want_aux=True)
        assert_same_bytes((f1.Features, pts1, aux1), got)
        assert_same_bytes((fm.fast_extract_batch(inp, [img], want_aux=True)[0][0].Features,), got[:1])   # the group of one


def test_the_planted_corners_on_the_seams_come_out_in_their_group(gpu):
    """Every planted pixel of view 0 is a keypoint with its score, beside two views full of corners."""
    pts = fc.planted(150, 200)[1]
    assert len(pts) >= 20
    rc, counts, bufs = run_batch(gpu, images("seams"), [400] * 3, fast_params(gpu._capi))
    assert rc == 0 and counts[0] == len(pts)
    _, loc, aux = rows_of(bufs[0], counts[0])
    assert [(int(y) - 1, int(x) - 1, int(s)) for (x, y), s in zip(loc, aux[:, 0])] == pts


@pytest.mark.parametrize("nl", [1, 3])
def test_a_flat_view_gets_no_rows_and_leaves_its_neighbours_intact(gpu, nl):
    a, b = images("nine")[:2]
    want = mirror(gpu, "nine", nl, 1.2)
    rc, counts, bufs = run_batch(gpu, [a, np.full_like(a, 90), b], [len(want[0][0]) + 1, 4, len(want[1][0]) + 1], fast_params(gpu._capi, nl))
    assert rc == 0 and counts == [len(want[0][0]), 0, len(want[1][0])]
    assert_same_bytes(rows_of(bufs[0], counts[0]), want[0])
    assert_same_bytes(rows_of(bufs[2], counts[2]), want[1])
    assert all((x == x.flat[0]).all() for x in bufs[1]), "the empty view's outputs are not written"


def test_capacity_protocol_reports_every_count_writes_nothing_and_one_retry_succeeds(gpu):
    imgs, want = images("seams"), mirror(gpu, "seams", 3, 1.2)
    need = [len(w[0]) for w in want]
    prm = fast_params(gpu._capi, 3)
    for device in (False, True):
        rc, counts, bufs = run_batch(gpu, imgs, [need[0], 10, need[2]], prm, device=device)
        assert rc == gpu._capi.APS_E_CAP and counts == need
        assert all((b[0] == FILL).all() and (b[1] == -7.5).all() and (b[2] == -7.5).all() for b in bufs), "nothing is written"
    rc, counts, bufs = run_batch(gpu, imgs, counts, prm)
    assert rc == 0 and counts == need
    for k in range(3):
        assert_same_bytes(rows_of(bufs[k], need[k]), want[k])
    # a view without outputs, or with cap = 0, only counts
    rc, counts, bufs = run_batch(gpu, imgs, [need[0], 0, need[2]], prm, count_only=(0,))
    assert rc == gpu._capi.APS_E_CAP and counts == need and all((b[0] == FILL).all() for b in bufs)
    # max_features keeps its single-view meaning, per view: the call fails when a view finds more
    rc, counts, bufs = run_batch(gpu, imgs, need, fast_params(gpu._capi, 3, max_features=need[0] + 1))
    assert rc == gpu._capi.APS_E_CAP and counts == need and all((b[0] == FILL).all() for b in bufs)


def test_column_major_layout_and_padding(gpu):
    imgs, want = images("nine"), mirror(gpu, "nine", 3, 1.2)
    need = [len(w[0]) for w in want]
    rc, counts, bufs = run_batch(gpu, imgs, [n + 3 for n in need], fast_params(gpu._capi, 3), colmajor=True)
    assert rc == 0 and counts == need
    for k, n in enumerate(need):
        assert_same_bytes(rows_of(bufs[k], n, colmajor=True), want[k])
        assert (bufs[k][0][:, n:] == FILL).all() and (bufs[k][1][:, n:] == -7.5).all(), "padding belongs to the caller"
    rc, counts, bufs = run_batch(gpu, imgs, [n + 3 for n in need], fast_params(gpu._capi, 3), ldd=80)   # row padding
    assert rc == 0 and all((b[0][:, 64:] == FILL).all() for b in bufs)
    for k, n in enumerate(need):
        assert_same_bytes(rows_of(bufs[k], n), want[k])


def test_device_pointers_and_three_channels(gpu, fm):
    import torch

    imgs, want = images("seams"), mirror(gpu, "seams", 3, 1.2)
    need = [len(w[0]) for w in want]
    rc, counts, bufs = run_batch(gpu, imgs, [n + 1 for n in need], fast_params(gpu._capi, 3), device=True)
    assert rc == 0 and counts == need
    for k, n in enumerate(need):
        assert_same_bytes(rows_of(bufs[k], n), want[k])
        assert (bufs[k][0][n:] == FILL).all()
    res = fm.fast_extract_batch({"detector": "FAST", "NumLevels": 3}, [torch.tensor(a).cuda() for a in imgs], device_out=True, points_device=True)
    for k, (f, pts) in enumerate(res):
        assert f.Features.is_cuda and pts.is_cuda
        assert_same_bytes((f.Features.cpu().numpy(), pts.cpu().numpy()), want[k][:2])
    # gray values replicated over three channels give the gray plane back: the same rows through the RGB path
    rgb = [np.repeat(a[:, :, None], 3, 2) for a in imgs]
    rc, counts, bufs = run_batch(gpu, rgb, need, fast_params(gpu._capi, 3))
    assert rc == 0 and counts == need
    for k, n in enumerate(need):
        assert_same_bytes(rows_of(bufs[k], n), want[k])
