"""aps_kaze_extract_select on the device against the NumPy mirror of DESIGN.md "KAZE selection and Upright"
(tests/kaze_select_mirror.py), bit for bit under test_kaze_gpu.assert_matches_mirror's rule: the kept set and its order, loc as
uint64, scale / metric / level and the descriptors as uint32 (angle_deg passes through atan2f and may differ by 1e-3 degrees; with
Upright its bits are +0.0).  The cases are kaze_select_cases': each costs about a second of mirror time."""
import ctypes as C
import threading
from importlib import import_module

import numpy as np
import pytest

import kaze_select_cases as ksc
from test_kaze_gpu import assert_matches_mirror, u32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def check(fm, name, n_rows, **keys):
    img, md, mloc, maux = ksc.mirror(name, **keys)
    assert len(md) == n_rows, (len(md), n_rows)
    d, loc, aux = fm.kaze_extract(dict(keys, detector="KAZE"), img, want_aux=True)
    assert_matches_mirror(d, loc, aux, md, mloc, maux)
    if keys.get("Upright"):
        assert not u32(aux[:, 1]).any(), "angle_deg is +0.0"
    return d, loc, aux


@pytest.mark.parametrize("name,N,rows", [("97x131", 1, 1), ("97x131", 40, 40), ("97x131", 99, 99), ("97x131", 500, 99), ("64x64", 5, 5),
                                         ("tie", 51, 51), ("tie", 52, 52)])
def test_strongest(fm, name, N, rows):
    """N = 40 cuts, 99 is the count, 500 is above it; on the tie image 51 cuts a pair of equal metrics (the earlier row stays) and 52
    cuts none."""
    d, loc, aux = check(fm, name, rows, NumStrongest=N)
    full = fm.kaze_extract({"detector": "KAZE"}, ksc.image(name), want_aux=True)
    assert len(full[0]) == ksc.COUNTS[name]
    if N >= ksc.COUNTS[name]:
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((d, loc, aux), full)), "N >= count: the unselected result"
    else:   # every byte of a kept row is the same row's of the unselected call
        at = [int(np.flatnonzero((bits(full[1]).reshape(len(full[1]), -1) == bits(loc[k:k + 1])).all(1) & (u32(full[2][:, 3]) == u32(aux[k, 3])))[0])
              for k in range(len(loc))]
        assert at == sorted(at) and all(np.array_equal(bits(a), bits(b[at])) for a, b in zip((d, loc, aux), full))


@pytest.mark.parametrize("name,N,grid,rows", [("pairA", 146, (8, 8), 146), ("pairA", 58, (8, 8), 58), ("pairA", 400, (4, 4), 400),
                                              ("97x131", 40, (32, 32), 40), ("48x2100", 100, (3, 17), 100), ("131x97x3", 30, (8, 8), 30),
                                              ("131x97x3", 200, (8, 8), 91)])
def test_uniform(fm, name, N, grid, rows):
    """8 x 8 on pairA at the two budgets of the occupancy figures, a coarse grid with a large budget, 1024 cells that are mostly
    empty, cell division on a plane far from square, the RGB path, and a budget above the count."""
    check(fm, name, rows, NumUniform=N, UniformGrid=grid)


def test_default_grid_and_one_cell(fm):
    img = ksc.image("pairA")
    a = fm.kaze_extract({"detector": "KAZE", "NumUniform": 146}, img, want_aux=True)
    b = fm.kaze_extract({"detector": "KAZE", "NumUniform": 146, "UniformGrid": (8, 8)}, img, want_aux=True)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)), "UniformGrid defaults to (8, 8)"
    for N in (58, 400):   # a (1, 1) grid is the strongest-N result byte for byte
        u = fm.kaze_extract({"detector": "KAZE", "NumUniform": N, "UniformGrid": (1, 1)}, img, want_aux=True)
        s = fm.kaze_extract({"detector": "KAZE", "NumStrongest": N}, img, want_aux=True)
        assert len(u[0]) == N and all(np.array_equal(bits(x), bits(y)) for x, y in zip(u, s))


@pytest.mark.parametrize("name", ["97x131", "pairA"])
def test_upright_alone(fm, name):
    d, loc, aux = check(fm, name, ksc.COUNTS[name], Upright=True)
    fd, floc, faux = fm.kaze_extract({"detector": "KAZE"}, ksc.image(name), want_aux=True)
    assert np.array_equal(bits(loc), bits(floc)) and np.array_equal(bits(aux[:, [0, 2, 3]]), bits(faux[:, [0, 2, 3]]))
    assert (u32(d) != u32(fd)).any(1).mean() > 0.9
    off = fm.kaze_extract({"detector": "KAZE", "Upright": False}, ksc.image(name), want_aux=True)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(off, (fd, floc, faux)))


@pytest.mark.parametrize("keys,rows", [({"NumStrongest": 40}, 40), ({"NumUniform": 40, "UniformGrid": (5, 7)}, 40), ({"NumStrongest": 500}, 99)])
def test_upright_with_a_selection(fm, keys, rows):
    check(fm, "97x131", rows, Upright=True, **keys)


def _raw(gpu, entry, prm, img, cap, ldd=64, layout=None, fill=np.float32(-7.5), outputs=True):
    capi = gpu._capi
    layout = capi.APS_ROWMAJOR if layout is None else layout
    rows = max(cap, 1)
    desc = np.full((rows, ldd) if layout == capi.APS_ROWMAJOR else (64, ldd), fill, np.float32)
    loc = np.full((2, rows if layout == capi.APS_ROWMAJOR else ldd), -7.5, np.float64)
    aux = np.full((rows, 4), fill, np.float32)
    cnt = C.c_int64(-1)
    img = np.ascontiguousarray(img)
    rc = entry(capi.ptr(img), img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, capi.APS_IMG_U8_HWC, C.byref(prm),
               capi.ptr(desc) if outputs else None, layout, ldd, capi.ptr(loc) if outputs else None, loc.shape[1], capi.ptr(aux) if outputs else None,
               cap, C.byref(cnt))
    return rc, cnt.value, desc, loc, aux


def _params(gpu, select=0, n=0, grid=(0, 0), upright=0, max_features=0):
    capi = gpu._capi
    return capi.aps_kaze_select_params(capi.aps_kaze_params(1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_REGION, max_features), select, n, grid[0], grid[1], upright)


def test_no_selection_through_the_new_entry_is_aps_kaze_extract(gpu):
    capi = gpu._capi
    img = ksc.image("97x131")
    new = _raw(gpu, capi.lib.aps_kaze_extract_select, _params(gpu), img, 120, 128)
    old = _raw(gpu, capi.lib.aps_kaze_extract, capi.aps_kaze_params(1e-4, 3, 4, capi.APS_KAZE_DIFFUSION_REGION, 0), img, 120, 128)
    assert new[0] == old[0] == 0 and new[1] == old[1] == 99
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(new[2:], old[2:])), "every byte, the caller's beyond the rows included"


def test_capacity_protocol(gpu):
    capi = gpu._capi
    entry = capi.lib.aps_kaze_extract_select
    img, md, mloc, maux = ksc.mirror("97x131", NumStrongest=40)
    prm = _params(gpu, 1, 40)
    rc, n, desc, loc, aux = _raw(gpu, entry, prm, img, 40, 128)   # cap = N suffices although 99 candidates were found
    assert rc == 0 and n == 40
    assert_matches_mirror(desc[:, :64], np.ascontiguousarray(loc.T), aux, md, mloc, maux)
    assert not desc[:, 64:].any(), "columns 64..127 are zeroed at ldd >= 128"
    rc, n, desc, loc, aux = _raw(gpu, entry, prm, img, 39)   # cap < K: the kept count, nothing written
    assert rc == capi.APS_E_CAP and n == 40
    assert (desc == np.float32(-7.5)).all() and (loc == -7.5).all() and (aux == np.float32(-7.5)).all()
    rc, n, *_ = _raw(gpu, entry, prm, img, 0, outputs=False)   # count-only mode
    assert rc == capi.APS_E_CAP and n == 40
    rc, n, *_ = _raw(gpu, entry, _params(gpu, 2, 500, (8, 8)), img, 0, outputs=False)
    assert rc == capi.APS_E_CAP and n == 99
    rc, n, desc, *_ = _raw(gpu, entry, prm, img, 43, 80)   # rows beyond the kept count and columns beyond 63 stay the caller's
    assert rc == 0 and n == 40 and np.array_equal(u32(desc[:40, :64]), u32(md))
    assert (desc[40:] == np.float32(-7.5)).all() and (desc[:, 64:] == np.float32(-7.5)).all()
    # max_features limits the candidates found, before the selection: 99 > 50 fails although 40 rows would fit
    rc, n, desc, *_ = _raw(gpu, entry, _params(gpu, 1, 40, max_features=50), img, 64)
    assert rc == capi.APS_E_CAP and n == 99 and (desc == np.float32(-7.5)).all()
    rc, n, *_ = _raw(gpu, entry, _params(gpu, 1, 40, max_features=99), img, 64)
    assert rc == 0 and n == 40


def test_column_major_layout_with_padding(gpu):
    capi = gpu._capi
    img, md, mloc, maux = ksc.mirror("131x97x3", NumUniform=30, Upright=True)
    ld = 30 + 5
    rc, n, desc, loc, aux = _raw(gpu, capi.lib.aps_kaze_extract_select, _params(gpu, 2, 30, (8, 8), 1), img, ld, ld, capi.APS_COLMAJOR)
    assert rc == 0 and n == 30
    assert_matches_mirror(np.ascontiguousarray(desc[:, :30].T), np.ascontiguousarray(loc[:, :30].T), aux[:30], md, mloc, maux)
    assert (desc[:, 30:] == np.float32(-7.5)).all() and (loc[:, 30:] == -7.5).all() and (aux[30:] == np.float32(-7.5)).all()
    planar = np.ascontiguousarray(img.transpose(2, 1, 0))   # MATLAB's h x w x 3 in memory
    d2 = np.full((64, ld), np.float32(-7.5), np.float32)
    l2 = np.full((2, ld), -7.5, np.float64)
    cnt = C.c_int64(0)
    prm = _params(gpu, 2, 30, (8, 8), 1)
    rc = capi.lib.aps_kaze_extract_select(capi.ptr(planar), img.shape[0], img.shape[1], 3, capi.APS_IMG_U8_MATLAB, C.byref(prm), capi.ptr(d2),
                                          capi.APS_COLMAJOR, ld, capi.ptr(l2), ld, None, ld, C.byref(cnt))
    assert rc == 0 and cnt.value == 30 and np.array_equal(bits(d2), bits(desc)) and np.array_equal(bits(l2), bits(loc))


def test_resident_result_holds_n_rows(fm):
    import torch

    img, md, mloc, _ = ksc.mirror("97x131", NumStrongest=40)
    dev = torch.from_numpy(np.array(img)).cuda()
    res, pts = fm.kaze_extract({"detector": "KAZE", "NumStrongest": 40}, dev, device_out=True)
    assert res.shape == (40, 64) and res.stride(0) == 128 and np.array_equal(u32(res.cpu().numpy()), u32(md))
    assert res.untyped_storage().nbytes() == 40 * 128 * 4, "the capacity buffer holds N rows"
    assert np.array_equal(bits(np.asarray(pts)), bits(mloc))
    full, pd = fm.extract_features({"detector": "KAZE", "NumUniform": 40, "UniformGrid": (32, 32)}, dev, device_out=True, points_device=True)
    want = ksc.mirror("97x131", NumUniform=40, UniformGrid=(32, 32))
    assert full.shape == (40, 128) and not bool(full[:, 64:].any()) and np.array_equal(u32(full[:, :64].cpu().numpy()), u32(want[1]))
    assert full.untyped_storage().nbytes() == 40 * 128 * 4 and np.array_equal(bits(pd.cpu().numpy()), bits(want[2]))


def test_two_calls_and_four_threads_give_identical_bytes(fm):
    img = ksc.image("pairA")
    for inp in ({"detector": "KAZE", "NumUniform": 146, "Upright": True}, {"detector": "KAZE", "NumStrongest": 300}):
        ref = fm.kaze_extract(inp, img, want_aux=True)
        again = fm.kaze_extract(inp, img, want_aux=True)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ref, again))
        got = [None] * 4

        def work(k):
            got[k] = fm.kaze_extract(inp, img, want_aux=True)

        ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        for g in got:
            assert g is not None and all(np.array_equal(bits(a), bits(b)) for a, b in zip(ref, g))
