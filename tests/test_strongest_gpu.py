"""Device strongest-N for SIFT and SURF (DESIGN.md "Strongest-N for SIFT and SURF") against the CPU references: oracle.sift and
tests/surf_mirror.py cut by tests/strongest_mirror.py.  Tolerances are those of the unselected device tests: SIFT 0 everywhere
(u32 / u64 bits, test_sift_params_gpu.py), SURF 0 except angle_deg <= 1e-3 degrees (test_surf_gpu.py).  The cases and their
figures are strongest_cases.py's, checked device-free in test_strongest_cases.py."""
import ctypes as C
import threading
from importlib import import_module

import numpy as np
import pytest

import strongest_cases as sc
import strongest_mirror as stm
import surf_cases
from test_sift_params_gpu import assert_equals_oracle
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


_UNSELECTED = {}


def unselected(fm, det, name):
    """The device's result without the key, computed once per case and shared (read-only)."""
    if (det, name) not in _UNSELECTED:
        if det == "SIFT":
            out = fm.sift_extract(sc.sift_input(name), sc.sift_image(name), want_aux=True)
        else:
            out = fm.surf_extract(sc.surf_input(name), sc.surf_reference(name)[0], want_aux=True)
        for a in out:
            a.setflags(write=False)
        _UNSELECTED[(det, name)] = out
    return _UNSELECTED[(det, name)]


# ---- 1. the selection equals the mirror ------------------------------------------------------------------------------------
SIFT_SELECTIONS = [(name, N) for name in ("120x160", "97x131", "gray", "37x37") for N in sc.SIFT_CASES[name][6]]
SURF_SELECTIONS = [(name, N) for name in sc.SURF_CASES for N in sc.SURF_CASES[name][3]]


@pytest.mark.parametrize("name,N", SIFT_SELECTIONS)
def test_sift_selection_equals_the_mirror(fm, name, N):
    want = stm.pick(sc.sift_reference(name), N)
    assert len(want[0]) == min(N, sc.SIFT_CASES[name][4])
    assert_equals_oracle(fm.sift_extract(sc.sift_input(name, N), sc.sift_image(name), want_aux=True), want)


def test_sift_selection_on_ties_between_keypoints(fm):
    """The twin patches: the cut falls between two keypoints of equal contrast, and the copy at the lower canonical index stays."""
    Ns = sc.sift_Ns("twin")
    assert len(Ns) == 4
    for N in Ns:
        assert_equals_oracle(fm.sift_extract(sc.sift_input("twin", N), sc.sift_image("twin"), want_aux=True), stm.pick(sc.sift_reference("twin"), N))


@pytest.mark.parametrize("name,N", SURF_SELECTIONS)
def test_surf_selection_equals_the_mirror(fm, name, N):
    img, ref = sc.surf_reference(name)
    want = stm.pick(ref, N)
    assert len(want[0]) == min(N, sc.SURF_CASES[name][2])
    d, loc, aux = fm.surf_extract(sc.surf_input(name, N), img, want_aux=True)
    assert_matches_mirror(d, loc, aux, *want)


# ---- 2. kept rows are rows of the unselected device result -------------------------------------------------------------------
@pytest.mark.parametrize("det,name,N", [("SIFT", "120x160", 100), ("SIFT", "twin", 7), ("SURF", "pairA", 200), ("SURF", "twin", 9)])
def test_kept_rows_are_rows_of_the_unselected_device_result(fm, det, name, N):
    full = unselected(fm, det, name)
    inp, img = (sc.sift_input(name, N), sc.sift_image(name)) if det == "SIFT" else (sc.surf_input(name, N), sc.surf_reference(name)[0])
    got = fm.extract_features(inp, img, want_aux=True)
    at = stm.keep(full[2][:, 2], N)
    assert 0 < len(at) == N < len(full[0]) and (np.diff(at) > 0).all()
    for g, f in zip(got, full):   # descriptor, location and all four aux columns, every bit (SURF's angle included: the same kernel ran)
        assert g.dtype == f.dtype and np.array_equal(u8(g), u8(f[at]))


@pytest.mark.parametrize("det,name", [("SIFT", "120x160"), ("SURF", "97x131")])
def test_no_more_rows_than_N_gives_the_unselected_result(fm, det, name):
    full = unselected(fm, det, name)
    n = len(full[0])
    for N in (n, n + 1, 5000):
        inp, img = (sc.sift_input(name, N), sc.sift_image(name)) if det == "SIFT" else (sc.surf_input(name, N), sc.surf_reference(name)[0])
        got = fm.extract_features(inp, img, want_aux=True)
        assert all(g.shape == f.shape and np.array_equal(u8(g), u8(f)) for g, f in zip(got, full))


# ---- 3. capacity, count-only, padding, layouts, pointers of the two entries ------------------------------------------------------
RAW = {"SIFT": ("120x160", 100, 128), "SURF": ("pairA", 200, 64)}   # det: (case, N, descriptor width)


def _raw(capi, det, N, cap, ldd, layout=None, ldl=None, where="host", with_out=True, img_layout=None, max_features=0):
    """The strongest entry of `det` into sentinel-filled outputs (util.sentinel_buffer): desc cap x ldd (row-major) or width x ldd
    (column-major), loc 2 x ldl, aux cap x 4.  Returns (rc, count, desc, loc, aux) as those matrices."""
    import torch

    name, _, width = RAW[det]
    layout = capi.APS_ROWMAJOR if layout is None else layout
    if det == "SIFT":
        img = sc.sift_image(name)
        prm = capi.aps_sift_strongest_params(capi.aps_sift_params(*sc.SIFT_DEFAULT, max_features), N)
        entry = capi.lib.aps_sift_extract_strongest
    else:
        img = sc.surf_reference(name)[0]
        prm = capi.aps_surf_strongest_params(capi.aps_surf_params(sc.SURF_CASES[name][1], 8, 4, 0, max_features), N)
        entry = capi.lib.aps_surf_extract_strongest
    h, w, ch = img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3
    src = np.array(img) if img_layout is None else to_planar(img)   # (a writable copy: the shared images are read-only)
    rows = max(cap, 1)
    ldl = rows if ldl is None else ldl
    outer = rows if layout == capi.APS_ROWMAJOR else width
    desc = place(sentinel_buffer(outer * ldd, np.float32), where)
    loc = place(sentinel_buffer(2 * ldl, np.float64), where)
    aux = place(sentinel_buffer(4 * rows, np.float32), where)
    cnt = C.c_int64(-1)
    torch.cuda.synchronize()
    pd, pl, pa = (capi.ptr(desc), capi.ptr(loc), capi.ptr(aux)) if with_out else (None, None, None)
    rc = entry(capi.ptr(place(src, where)), h, w, ch, capi.APS_IMG_U8_HWC if img_layout is None else img_layout, C.byref(prm), pd, layout, ldd,
               pl, ldl, pa, cap, C.byref(cnt))
    capi.check(capi.lib.aps_synchronize())
    return rc, int(cnt.value), fetch(desc).reshape(outer, ldd), fetch(loc).reshape(2, ldl), fetch(aux).reshape(rows, 4)


def _all_sentinel(*arrays):
    return all(same_bits(a.reshape(-1), sentinel_buffer(a.size, a.dtype)) for a in (np.ascontiguousarray(x) for x in arrays))


def _want(det):
    name, N, _ = RAW[det]
    return stm.pick(sc.sift_reference(name) if det == "SIFT" else sc.surf_reference(name)[1], N)


def _assert_equals(det, got, want):
    if det == "SIFT":
        assert_equals_oracle(got, want)
    else:
        assert_matches_mirror(np.ascontiguousarray(got[0]), np.ascontiguousarray(got[1]), got[2], *want)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("det", ["SIFT", "SURF"])
def test_capacity_is_the_number_kept(capi, det, where):
    """cap = rows kept suffices although the call has more candidates; one less is APS_E_CAP with the true count and nothing written;
    cap = 0 and desc = NULL count."""
    _, K, width = RAW[det]
    want = _want(det)
    assert len(want[0]) == K
    rc, cnt, desc, loc, aux = _raw(capi, det, K, K, width, where=where)
    assert rc == 0 and cnt == K
    _assert_equals(det, (desc, loc.T, aux), want)
    rc, cnt, desc, loc, aux = _raw(capi, det, K, K - 1, width, where=where)
    assert rc == capi.APS_E_CAP and cnt == K and _all_sentinel(desc, loc, aux)
    rc, cnt, desc, loc, aux = _raw(capi, det, K, 0, width, where=where)   # cap = 0 counts
    assert rc == capi.APS_E_CAP and cnt == K and _all_sentinel(desc, loc, aux)
    rc, cnt, *_ = _raw(capi, det, K, K, width, with_out=False)   # desc = NULL counts
    assert cnt == K and rc == capi.APS_E_ARG    # features present and no output to put them in


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("det", ["SIFT", "SURF"])
def test_padded_outputs_keep_their_padding(capi, det, where):
    """ldd above the width, ldl above cap, cap above the count: the elements between the rows, rows count..cap and the tail of loc
    stay the caller's."""
    _, K, width = RAW[det]
    cap = K + 3
    rc, cnt, desc, loc, aux = _raw(capi, det, K, cap, width + 16, ldl=cap + 5, where=where)
    assert rc == 0 and cnt == K
    _assert_equals(det, (desc[:K, :width], loc[:, :K].T, aux[:K]), _want(det))
    assert _all_sentinel(desc[:, width:], desc[K:], loc[:, K:], aux[K:])


def test_surf_leading_dimension_128_is_zero_padded(capi):
    _, K, width = RAW["SURF"]
    rc, cnt, desc, loc, aux = _raw(capi, "SURF", K, K + 3, 128)
    assert rc == 0 and cnt == K
    _assert_equals("SURF", (desc[:K, :64], loc[:, :K].T, aux[:K]), _want("SURF"))
    assert not desc[:K, 64:].any() and _all_sentinel(desc[K:], loc[:, K + 3:], aux[K:])


@pytest.mark.parametrize("det", ["SIFT", "SURF"])
def test_column_major_descriptors(capi, det):
    _, K, width = RAW[det]
    ld = K + 5
    rc, cnt, desc, loc, aux = _raw(capi, det, K, K, ld, layout=capi.APS_COLMAJOR, ldl=ld)
    assert rc == 0 and cnt == K and desc.shape == (width, ld)
    _assert_equals(det, (desc[:, :K].T, loc[:, :K].T, aux), _want(det))
    assert _all_sentinel(desc[:, K:], loc[:, K:])


def test_surf_max_features_is_a_limit_on_the_candidates(capi):
    """max_features keeps its meaning: the call fails when the detection finds more, whatever n_strongest keeps."""
    name, K, width = RAW["SURF"]
    M = sc.SURF_CASES[name][2]
    rc, cnt, desc, loc, aux = _raw(capi, "SURF", K, K, width, max_features=M - 1)
    assert rc == capi.APS_E_CAP and cnt == M and b"max_features" in capi.lib.aps_last_error() and _all_sentinel(desc, loc, aux)
    rc, cnt, desc, loc, aux = _raw(capi, "SURF", K, K, width, max_features=M)
    assert rc == 0 and cnt == K
    _assert_equals("SURF", (desc, loc.T, aux), _want("SURF"))


# ---- 8. the gateway's call shape ------------------------------------------------------------------------------------------------
def test_matlab_layouts_give_the_same_rows(capi):
    """aps_sift_extract_strongest as matlab/aps_mex.cpp calls it: planar column-major image, column-major descriptors."""
    _, K, width = RAW["SIFT"]
    rc, cnt, desc, loc, aux = _raw(capi, "SIFT", K, K, K, layout=capi.APS_COLMAJOR, img_layout=capi.APS_IMG_U8_MATLAB)
    assert rc == 0 and cnt == K
    rc, cnt, rdesc, rloc, raux = _raw(capi, "SIFT", K, K, width)
    assert rc == 0 and same_bits(desc.T, rdesc) and same_bits(loc, rloc) and same_bits(aux, raux)
    assert_equals_oracle((rdesc, rloc.T, raux), _want("SIFT"))


# ---- 4. resident output ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", ["SIFT", "SURF"])
def test_resident_output_holds_N_rows_and_two_runs_agree(fm, det):
    import torch

    name, N, width = RAW[det]
    want = _want(det)
    extract = fm.sift_extract if det == "SIFT" else fm.surf_extract
    inp = sc.sift_input(name, N) if det == "SIFT" else sc.surf_input(name, N)
    img = sc.sift_image(name) if det == "SIFT" else sc.surf_reference(name)[0]
    dimg = torch.from_numpy(np.array(img)).cuda()
    torch.cuda.synchronize()
    runs = []
    for compact in (False, True, False):
        f, pts = extract(inp, dimg, device_out=True, points_device=True, compact=compact)
        assert f.is_cuda and pts.is_cuda and f.dtype == torch.float32 and tuple(f.shape) == (N, width)
        assert f.untyped_storage().nbytes() <= N * 128 * 4, "the descriptor tensor's storage holds more than N rows"
        _assert_equals(det, (f.cpu().numpy(), pts.cpu().numpy()) if det == "SIFT" else (f.cpu().numpy(), pts.cpu().numpy(), want[2]), want)
        runs.append((f.cpu().numpy(), pts.cpu().numpy()))
    assert all(np.array_equal(u8(a), u8(b)) for a, b in zip(runs[0], runs[2]))


def test_surf_from_four_threads_is_identical(fm):
    name, N, _ = RAW["SURF"]
    img, inp = sc.surf_reference(name)[0], sc.surf_input(name, N)
    ref = fm.surf_extract(inp, img, want_aux=True)
    got = [None] * 4

    def work(k):
        got[k] = fm.surf_extract(inp, img, want_aux=True)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for g in got:
        assert g is not None and all(np.array_equal(u8(a), u8(b)) for a, b in zip(ref, g))


# ---- 5. every host entry returns the same rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("det", ["SIFT", "SURF"])
def test_host_entries_return_the_same_rows(gpu, fm, det):
    import torch

    pl = import_module(gpu.__name__ + ".pipeline")
    name, N, width = RAW[det]
    want = _want(det)
    inp = sc.sift_input(name, N) if det == "SIFT" else sc.surf_input(name, N)
    img = sc.sift_image(name) if det == "SIFT" else sc.surf_reference(name)[0]
    for entry in (fm.getFeaturePoints, fm.extract_features):
        f, pts = entry(inp, img)
        _assert_equals(det, (f, pts) if det == "SIFT" else (f, pts, want[2]), want)
    rgb = np.array(img if img.ndim == 3 else np.repeat(img[:, :, None], 3, 2))   # (a gray triple's gray plane is the gray value)
    dimgs = [torch.from_numpy(rgb).cuda() for _ in range(3)]   # three views: the worker streams
    torch.cuda.synchronize()
    descs, kps = pl.extract_features(pl.default_input(**inp), dimgs)
    for d, p in zip(descs, kps):
        d = d.cpu().numpy()[:, :width]
        p = p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p)
        assert d.shape == (N, width)
        _assert_equals(det, (d, p) if det == "SIFT" else (d, p, want[2]), want)


# ---- 6. end to end, SIFT -------------------------------------------------------------------------------------------------------------
E2E_N = 800


def _scene(gpu):
    import torch

    synth = import_module(gpu.__name__ + ".synth")
    nx, ny, w, h, f = 3, 2, 640, 480, 900.0   # the scene of test_pipeline_gpu.py
    cams = synth.grid_cameras(nx, ny, w, h, f, 2 * np.arctan(w / (2 * f)) * 0.6, 2 * np.arctan(h / (2 * f)) * 0.6, 1.0, 7)
    views = {i: synth.render_view(cams[i], h, w, 7, "cuda", finest_px=6.0) for i in range(nx * ny)}
    torch.cuda.synchronize()
    return cams, views


def _covered(pano):
    pano = pano.cpu().numpy() if hasattr(pano, "cpu") else np.asarray(pano)
    return pano.ndim == 3 and float((pano.max(axis=2) > 0).mean())


def test_sift_stitch_with_the_800_strongest_rows_per_view(gpu):
    pl = import_module(gpu.__name__ + ".pipeline")
    cams, views = _scene(gpu)
    inp = pl.default_input(bands=3, NumStrongest=E2E_N)
    panos, info = pl.stitch(inp, [views[i] for i in range(6)], Ks=[c["K"] for c in cams], tile=(512, 512))
    assert list(info["n_features"]) == [E2E_N] * 6
    assert info["n_components"] == 1 and len(panos) == 1 and sorted(info["components"][0]["members"]) == list(range(6))
    assert info["n_pairs_verified"] >= 5
    assert _covered(panos[0]) > 0.5


def test_sift_stitch_distributed_with_the_800_strongest_rows_per_view(gpu):
    pl = import_module(gpu.__name__ + ".pipeline")
    par = import_module(gpu.__name__ + ".parallel")
    cams, views = _scene(gpu)
    inp = pl.default_input(bands=3, NumStrongest=E2E_N)
    pano, info = par.stitch_distributed(inp, views, 6, [c["K"] for c in cams], (512, 512), 0, None, pano_root=0)
    assert [int(v) for v in info["n_features"]] == [E2E_N] * 6
    assert info["n_components"] == 1 and sorted(info["members"]) == list(range(6))
    assert len(info["pairs"]) >= 5
    assert _covered(pano) > 0.5


# ---- 7. end to end, SURF -----------------------------------------------------------------------------------------------------------
def test_surf_pair_is_verified_with_the_200_strongest_rows(gpu):
    """surf_cases.pair() cut to 200 rows per image: the pair is verified, and the model maps A's corners to within 1 px of PAIR_H.
    On the mirror: 138 ratio matches at N = 200, all within 1.5 px of PAIR_H."""
    import torch

    pl = import_module(gpu.__name__ + ".pipeline")
    A, B = surf_cases.pair()
    rgb = lambda g: torch.from_numpy(np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))).cuda()  # noqa: E731
    inp = pl.default_input(detector="SURF", NumStrongest=200)
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
