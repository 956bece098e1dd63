"""Device SURF in groups of views (aps_surf_extract_batch and its _strongest / _uniform forms) against the NumPy mirror of the
contract (tests/surf_mirror.py) and against the single-view entries, bit for bit.  Images are surf_cases.band_limited(1000 + k, h, w).
Shapes (h x w, views):
  97 x 131, 9    odd sides, tails of every tile and wave; one view more than 8
  120 x 160, 3   a plain group
  43 x 139, 2    a one-octave plan (min side in 27..50: the second octave's largest filter, 51, does not fit): the smallest area
                 with at least 20 mirror rows in both views, searched over heights 27..50 and widths in steps of 8
Every comparison first asserts that the expected result holds at least 20 rows per view."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import strongest_mirror as stm
import surf_cases as sc
import surf_mirror as sm

pytestmark = pytest.mark.gpu

GROUPS = {"97x131": (97, 131, 9), "120x160": (120, 160, 3), "43x139": (43, 139, 2)}
FILL = np.float32(-7.5)
_IMAGES, _MIRROR = {}, {}


def images(name, channels=1):
    if (name, channels) not in _IMAGES:
        h, w, g = GROUPS[name]
        _IMAGES[name, channels] = [sc.band_limited(1000 + k, h, w, channels=channels) for k in range(g)]
        for a in _IMAGES[name, channels]:
            a.setflags(write=False)
    return _IMAGES[name, channels]


def mirror(name, channels=1, **kw):
    """The mirror's (desc, loc, aux) of every view of a group, computed once and shared (read-only); at least 20 rows each."""
    key = (name, channels, tuple(sorted(kw.items())))
    if key not in _MIRROR:
        _MIRROR[key] = [sm.extract(img, **kw) for img in images(name, channels)]
        for out in _MIRROR[key]:
            assert len(out[0]) >= 20, "the case must have keypoints to compare"
            for a in out:
                a.setflags(write=False)
    return _MIRROR[key]


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_matches_mirror(got, want):
    """Keypoint set and order, loc, scale, metric, sign and descriptors bit for bit; angle_deg passes through atan2f (1e-3 deg)."""
    (d, loc, aux), (md, mloc, maux) = got, want
    assert d.shape == md.shape and loc.shape == mloc.shape, (d.shape, md.shape)
    assert np.array_equal(np.ascontiguousarray(loc).view(np.uint64), np.ascontiguousarray(mloc).view(np.uint64)), "loc bits / keypoint order"
    for col, what in ((0, "scale"), (2, "metric"), (3, "sign of Laplacian")):
        assert np.array_equal(u32(aux[:, col]), u32(maux[:, col])), what
    da = np.abs((aux[:, 1].astype(np.float64) - maux[:, 1].astype(np.float64) + 180.0) % 360.0 - 180.0)
    assert da.size == 0 or da.max() <= 1e-3, da.max()
    assert np.array_equal(u32(d), u32(md)), "descriptor bits (%d rows differ)" % int((u32(d) != u32(md)).any(1).sum())


def assert_same_bytes(got, want):
    """Two device results: every byte, the angle included."""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def surf_params(capi, thr=1000.0, octaves=8, levels=4, upright=0):
    return capi.aps_surf_params(thr, octaves, levels, upright, 0)


def run_batch(gpu, imgs, caps, ldd=64, entry="aps_surf_extract_batch", prm=None, colmajor=False, device=False, count_only=()):
    """The raw group call on FILL-ed outputs of caps[k] rows (column-major: ldd = ldl = max cap): (rc, counts, [(desc, loc, aux)]).
    device: images and outputs are resident tensors, handed back as numpy copies.  count_only: views that pass no outputs."""
    capi = gpu._capi
    g, most = len(imgs), max(max(caps), 1)
    prm = surf_params(capi) if prm is None else prm
    if colmajor:
        ldd = most
    keep, bufs = [], []
    if device:
        import torch
    for k, img in enumerate(imgs):
        img = np.ascontiguousarray(img)
        cap = max(caps[k], 1)
        desc = np.full((64, ldd) if colmajor else (cap, ldd), FILL, np.float32)
        loc = np.full((2, most), -7.5, np.float64)
        aux = np.full((cap, 4), FILL, np.float32)
        if device:
            img, desc, loc, aux = (torch.tensor(a).cuda() for a in (img, desc, loc, aux))
        keep.append(img)
        bufs.append((desc, loc, aux))
    if device:
        torch.cuda.synchronize()
    views = (capi.aps_surf_view * g)()
    for k in range(g):
        out = (None, None, None) if k in count_only else bufs[k]
        views[k].img, views[k].desc, views[k].loc, views[k].aux = (capi.ptr(keep[k]),) + tuple(capi.ptr(a) for a in out)
        views[k].cap, views[k].count = caps[k], -1
    h, w = imgs[0].shape[:2]
    rc = getattr(capi.lib, entry)(views, g, h, w, 1 if imgs[0].ndim == 2 else 3, capi.APS_IMG_U8_HWC, C.byref(prm),
                                  capi.APS_COLMAJOR if colmajor else capi.APS_ROWMAJOR, ldd, most)
    if device:
        capi.check(capi.lib.aps_synchronize())
        bufs = [tuple(a.cpu().numpy() for a in b) for b in bufs]
    return rc, [int(views[k].count) for k in range(g)], bufs


def rows_of(buf, n, colmajor=False):
    desc, loc, aux = buf
    return (np.ascontiguousarray(desc[:, :n].T) if colmajor else desc[:n, :64]), np.ascontiguousarray(loc[:, :n].T), aux[:n]


@pytest.mark.parametrize("name", list(GROUPS))
def test_every_view_equals_the_mirror_its_group_of_one_and_the_single_call(fm, name):
    imgs, want = images(name), mirror(name)
    inp = {"detector": "SURF"}
    got = fm.surf_extract_batch(inp, imgs, want_aux=True)
    assert len(got) == len(imgs)
    for k, img in enumerate(imgs):
        assert_matches_mirror(got[k], want[k])
        assert_same_bytes(got[k], fm.surf_extract_batch(inp, [img], want_aux=True)[0])
        assert_same_bytes(got[k], fm.surf_extract(inp, img, want_aux=True))
    plain = fm.surf_extract_batch(inp, imgs)   # (without aux: two results per view)
    assert all(len(p) == 2 for p in plain)
    for k in range(len(imgs)):
        assert_same_bytes(plain[k], got[k][:2])


def test_a_constant_view_gets_no_rows_and_leaves_its_neighbours_intact(gpu):
    a, _, b = images("120x160")
    want = mirror("120x160")
    caps = [len(want[0][0]) + 2, 4, len(want[2][0]) + 2]
    rc, counts, bufs = run_batch(gpu, [a, np.full_like(a, 128), b], caps)
    assert rc == 0 and counts == [len(want[0][0]), 0, len(want[2][0])]
    assert_matches_mirror(rows_of(bufs[0], counts[0]), want[0])
    assert_matches_mirror(rows_of(bufs[2], counts[2]), want[2])
    assert all((x == x.flat[0]).all() for x in bufs[1]), "the empty view's outputs are not written"
    for k in (0, 2):   # rows count..cap belong to the caller
        assert (bufs[k][0][counts[k]:] == FILL).all() and (bufs[k][2][counts[k]:] == FILL).all() and (bufs[k][1][:, counts[k]:] == -7.5).all()


def test_capacity_protocol_reports_every_count_writes_nothing_and_one_retry_succeeds(gpu):
    imgs, want = images("120x160"), mirror("120x160")
    need = [len(w[0]) for w in want]
    for device in (False, True):
        rc, counts, bufs = run_batch(gpu, imgs, [need[0], 10, need[2]], device=device)
        assert rc == gpu._capi.APS_E_CAP and counts == need
        assert all((b[0] == FILL).all() and (b[1] == -7.5).all() and (b[2] == FILL).all() for b in bufs), "nothing is written"
    rc, counts, bufs = run_batch(gpu, imgs, counts)
    assert rc == 0 and counts == need
    for k in range(3):
        assert_matches_mirror(rows_of(bufs[k], need[k]), want[k])
    # a view without outputs, or with cap = 0, only counts
    rc, counts, bufs = run_batch(gpu, imgs, [need[0], 0, need[2]], count_only=(0,))
    assert rc == gpu._capi.APS_E_CAP and counts == need and all((b[0] == FILL).all() for b in bufs)


def test_column_major_layout_gives_the_same_rows(gpu):
    imgs, want = images("97x131"), mirror("97x131")
    caps = [len(w[0]) + 3 for w in want]
    rc, counts, bufs = run_batch(gpu, imgs, caps, colmajor=True)
    assert rc == 0 and counts == [len(w[0]) for w in want]
    for k, n in enumerate(counts):
        assert_matches_mirror(rows_of(bufs[k], n, colmajor=True), want[k])
        assert (bufs[k][0][:, n:] == FILL).all() and (bufs[k][1][:, n:] == -7.5).all(), "padding belongs to the caller"


def test_leading_dimension_128_zeroes_columns_64_to_127(gpu):
    imgs, want = images("120x160"), mirror("120x160")
    caps = [len(w[0]) + 3 for w in want]
    rc, counts, bufs = run_batch(gpu, imgs, caps, ldd=128)
    assert rc == 0
    for k, n in enumerate(counts):
        assert_matches_mirror(rows_of(bufs[k], n), want[k])
        assert not bufs[k][0][:n, 64:].any() and (bufs[k][0][n:] == FILL).all()
    rc, counts, bufs = run_batch(gpu, imgs, caps, ldd=80)   # 64 <= ldd < 128: nothing beyond column 63
    assert rc == 0 and all((b[0][:, 64:] == FILL).all() for b in bufs)


def test_device_pointers_give_the_same_rows(gpu, fm):
    import torch

    imgs, want = images("97x131"), mirror("97x131")
    caps = [len(w[0]) + 1 for w in want]
    rc, counts, bufs = run_batch(gpu, imgs, caps, ldd=128, device=True)
    assert rc == 0
    for k, n in enumerate(counts):
        assert_matches_mirror(rows_of(bufs[k], n), want[k])
        assert (bufs[k][0][n:] == FILL).all()
    res = fm.surf_extract_batch({"detector": "SURF"}, [torch.tensor(a).cuda() for a in imgs], device_out=True,
                                points_device=True, padded=True)
    for k, (d, pts) in enumerate(res):
        assert d.is_cuda and pts.is_cuda and d.shape[1] == 128 and not d[:, 64:].any()
        assert np.array_equal(u32(d[:, :64].cpu().numpy()), u32(want[k][0])) and np.array_equal(pts.cpu().numpy(), want[k][1])


def test_three_channel_views(fm):
    imgs, want = images("120x160", 3)[:2], mirror("120x160", 3)[:2]
    got = fm.surf_extract_batch({"detector": "SURF"}, imgs, want_aux=True)
    for k in range(2):
        assert_matches_mirror(got[k], want[k])


@pytest.mark.parametrize("kw, prm", [(dict(NumOctaves=2, NumScaleLevels=3), dict(octaves=2, levels=3)), (dict(upright=True), dict(upright=1))])
def test_parameters_on_a_group_of_two(gpu, kw, prm):
    imgs, want = images("120x160")[:2], mirror("120x160", **kw)[:2]
    rc, counts, bufs = run_batch(gpu, imgs, [len(w[0]) for w in want], prm=surf_params(gpu._capi, **prm))
    assert rc == 0 and counts == [len(w[0]) for w in want]
    for k in range(2):
        assert_matches_mirror(rows_of(bufs[k], counts[k]), want[k])


def run_single(gpu, entry, prm, img, cap):
    capi = gpu._capi
    img = np.ascontiguousarray(img)
    desc, loc, aux = np.full((cap, 64), FILL, np.float32), np.full((2, cap), -7.5, np.float64), np.full((cap, 4), FILL, np.float32)
    cnt = C.c_int64(-1)
    capi.check(getattr(capi.lib, entry)(capi.ptr(img), img.shape[0], img.shape[1], 1, capi.APS_IMG_U8_HWC, C.byref(prm), capi.ptr(desc),
                                        capi.APS_ROWMAJOR, 64, capi.ptr(loc), cap, capi.ptr(aux), cap, C.byref(cnt)))
    return rows_of((desc, loc, aux), cnt.value)


@pytest.mark.parametrize("name", ["97x131", "120x160"])
@pytest.mark.parametrize("rule", ["strongest", "uniform"])
def test_selection_per_view_equals_the_single_view_entry(gpu, name, rule):
    """N lies between the smallest and the largest candidate count of the group, so some views are cut and others kept whole."""
    capi = gpu._capi
    imgs, want = images(name), mirror(name)
    cand = [len(w[0]) for w in want]
    N = (min(cand) + max(cand)) // 2
    assert 20 <= min(cand) <= N < max(cand)
    strongest = capi.aps_surf_strongest_params(surf_params(capi), N)
    prm = strongest if rule == "strongest" else capi.aps_surf_uniform_params(strongest, 3, 5)
    rc, counts, bufs = run_batch(gpu, imgs, [N + 2] * len(imgs), entry="aps_surf_extract_batch_" + rule, prm=prm)
    assert rc == 0 and counts == [min(c, N) for c in cand]
    for k, img in enumerate(imgs):
        got = rows_of(bufs[k], counts[k])
        assert_same_bytes(got, run_single(gpu, "aps_surf_extract_" + rule, prm, img, N + 2))
        assert (bufs[k][0][counts[k]:] == FILL).all()
        if rule == "strongest":
            assert_matches_mirror(got, stm.pick(want[k], N))
        elif cand[k] <= N:
            assert_matches_mirror(got, want[k])
    # the capacity protocol of the selection: min(candidates, N) is what a view needs
    caps = [N + 2] * len(imgs)
    caps[1] = 10
    rc, counts2, bufs = run_batch(gpu, imgs, caps, entry="aps_surf_extract_batch_" + rule, prm=prm)
    assert rc == capi.APS_E_CAP and counts2 == counts and all((b[0] == FILL).all() for b in bufs)
