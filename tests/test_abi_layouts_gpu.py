"""The C ABI as matlab/aps_mex.cpp calls it: APS_IMG_U8_MATLAB images, APS_COLMAJOR matrices, leading dimensions larger
than the logical extent, host pointers (and the same with resident buffers).  The Python layer passes HWC / row-major /
tight leading dimensions, so without this module the MATLAB-side branches of the kernels run nowhere.

Every case compares, with tolerance 0 on the bits,
  * the MATLAB-style call against the same entry point called HWC / row-major / tight on the same logical data, and
  * against the oracle where one computes the same bits (SIFT, k-NN, Hamming, matching, imresize, crop, BA, RANSAC).
Tolerance 0 is derived, not measured: a layout only changes addresses.

Padding contract (include/aps.h, conventions): elements outside the logical result are not written, for host and device
pointers alike.  Every output with a caller-given leading dimension or capacity is pre-filled with a sentinel (a NaN
payload, 0xA5 bytes, all-ones indices) that must survive the call outside the logical result.

Shapes: h != w, neither a multiple of the other, widths with w % 4 == 0 and without, channels that differ."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import oracle
from test_ba_oracle import _pack, _rot, _scene as _ba_scene
from test_ransac_oracle import H_TRUE, make_scene
from test_render_gpu import _scene as _render_scene
from test_sift_gpu import textured
from util import (fetch, from_planar, padded, place, planted_pair, same_bits, sentinel_buffer, sift_like, to_planar, unpad)

pytestmark = pytest.mark.gpu

WHERE = ["host", "device"]


@pytest.fixture(scope="module")
def capi(gpu):
    return gpu._capi


def _call(capi, fn, *args):
    """One ABI call bracketed the way a resident caller brackets it: torch's fills have landed, the library's stream has
    drained when the buffers are read."""
    import torch

    torch.cuda.synchronize()
    rc = fn(*args)
    capi.check(capi.lib.aps_synchronize())
    return rc


# ---- aps_sift_extract ---------------------------------------------------------------------------------------------
def _sift(capi, img, where, img_layout, desc_colmajor, ldd, ldl, cap, want_aux, sigma=1.6, img_arg=None):
    """aps_sift_extract with sentinel-filled outputs; returns (count, desc [n,128], loc [n,2], aux [n,4] or None,
    padding intact)."""
    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    if img_arg is None:
        img_arg = to_planar(img) if img_layout == capi.APS_IMG_U8_MATLAB else np.ascontiguousarray(img)
    prm = capi.aps_sift_params(sigma, 4, 0.00133, 6.0, 0)
    desc = place(sentinel_buffer(128 * ldd if desc_colmajor else cap * ldd, np.float32), where)
    loc = place(sentinel_buffer(2 * ldl, np.float64), where)
    aux = place(sentinel_buffer(4 * cap, np.float32), where) if want_aux else None
    cnt = C.c_int64(0)
    capi.check(_call(capi, capi.lib.aps_sift_extract, capi.ptr(img_arg), h, w, c, img_layout, C.byref(prm), capi.ptr(desc),
                     capi.APS_COLMAJOR if desc_colmajor else capi.APS_ROWMAJOR, ldd, capi.ptr(loc), ldl, capi.ptr(aux), cap,
                     C.byref(cnt)))
    n = int(cnt.value)
    d, ok_d = unpad(fetch(desc), n, 128, desc_colmajor, ldd)
    p, ok_l = unpad(fetch(loc), n, 2, True, ldl)
    ok_a, a = True, None
    if want_aux:
        a, ok_a = unpad(fetch(aux), n, 4, False, 4) if n else (np.zeros((0, 4), np.float32), True)
        ok_a = ok_a and same_bits(fetch(aux)[4 * n:], sentinel_buffer(4 * (cap - n), np.float32))
    return n, d, p, a, (ok_d, ok_l, ok_a)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("want_aux", [True, False], ids=["aux", "noaux"])
@pytest.mark.parametrize("h,w,c,sigma", [(97, 131, 3, 1.6), (129, 66, 3, 1.6), (96, 132, 1, 1.6), (97, 131, 1, 1.6), (97, 131, 3, 1.1)])
def test_sift_extract_as_the_gateway_calls_it(capi, h, w, c, sigma, want_aux, where):
    """aps_mex.cpp:54-55: planar image, column-major descriptors, ldd = ldl = cap > count, aux NULL (and present).
    sigma = 1.1 has no fused base kernel, so gray_up_kernel's planar reads run; the other cases run gray_u8_kernel's."""
    rng = np.random.default_rng(h * 7 + w + c)
    img = textured(rng, h, w, c)
    if c == 1:
        img = np.ascontiguousarray(img[..., 0])
    cap = h * w // 64 + 4096
    n, d, p, a, intact = _sift(capi, img, where, capi.APS_IMG_U8_MATLAB, True, cap, cap, cap, want_aux, sigma)
    assert 50 < n < cap
    # the same entry point, HWC / row-major / tight
    n0, d0, p0, a0, _ = _sift(capi, img, "host", capi.APS_IMG_U8_HWC, False, 128, n, n, want_aux, sigma)
    assert n0 == n and same_bits(d, d0) and same_bits(p, p0) and (not want_aux or same_bits(a, a0))
    od, ol, oa = oracle.sift(img, sigma)
    assert same_bits(d, od) and same_bits(p, np.ascontiguousarray(ol, np.float64)) and (not want_aux or same_bits(a, oa))
    assert intact == (True, True, True), f"padding of (desc, loc, aux) intact: {intact}"


@pytest.mark.parametrize("where", WHERE)
def test_sift_extract_row_major_with_padded_rows(capi, where):
    """desc_layout row-major with ldd > 128 and ldl > count: the other orientation of the strided copy-back."""
    rng = np.random.default_rng(77)
    img = textured(rng, 66, 129)
    cap = 4100
    n, d, p, a, intact = _sift(capi, img, where, capi.APS_IMG_U8_MATLAB, False, 128 + 7, cap + 3, cap, True)
    od, ol, oa = oracle.sift(img)
    assert n > 50 and same_bits(d, od) and same_bits(p, np.ascontiguousarray(ol, np.float64)) and same_bits(a, oa)
    assert intact == (True, True, True), f"padding of (desc, loc, aux) intact: {intact}"


def _misaligned(arr, off):
    """A resident copy of the bytes of `arr` whose base pointer is `off` bytes past a 4-byte boundary."""
    import torch

    flat = np.ascontiguousarray(arr).reshape(-1)
    big = torch.zeros(flat.size + 8, dtype=torch.uint8, device="cuda")
    view = big[off:off + flat.size]
    view.copy_(torch.from_numpy(flat))
    torch.cuda.synchronize()
    assert view.data_ptr() % 4 == off % 4
    return view


@pytest.mark.parametrize("w", [132, 131])
def test_sift_extract_from_an_unaligned_resident_image(capi, w):
    """The per-pixel path behind gray_u8_kernel's `& 3` test: an HWC image on the device whose base is 1, 2, 3 bytes off."""
    rng = np.random.default_rng(w)
    img = textured(rng, 97, w)
    od, ol, _ = oracle.sift(img)
    for off in (0, 1, 2, 3):
        n, d, p, _, _ = _sift(capi, img, "host", capi.APS_IMG_U8_HWC, False, 128, 4096, 4096, False, img_arg=_misaligned(img, off))
        assert n > 50 and same_bits(d, od) and same_bits(p, np.ascontiguousarray(ol, np.float64)), off


# ---- aps_render / aps_render_tiles / aps_render_tile_range ---------------------------------------------------------------
def _render_scene_small(rp, gray=1):
    """Three 37 x 53 views (one of them gray), a canvas that is no multiple of the tile."""
    rng = np.random.default_rng(4)
    imgs, cams = _render_scene(rng, n=3, W=53, H=37, f=70.0)
    if gray is not None:
        imgs[gray] = np.ascontiguousarray(imgs[gray][..., 1])
    sizes = [(37, 53, 3)] * 3
    opts = rp.default_opts({"anglePower": 2, "pyrLevels": 3, "pyrSigma": 1.0, "tile": (24, 40), "cropBorder": False}, cams, 1)
    geo = rp.canvas_geometry(cams, sizes, "spherical", 1, opts)
    assert geo["H"] % 24 and geo["W"] % 40 and geo["H"] != geo["W"]
    gains = [(1.0, 1.0, 1.0), (0.9, 1.1, 1.0), (1.2, 0.8, 1.05)]
    return imgs, cams, geo, opts, gains


def _structs(rp, capi, imgs, cams, gains, planar, data=None):
    arr, keep = rp.make_image_structs(imgs, cams, gains)
    if planar:
        keep = [to_planar(im) for im in imgs]
        for a, buf in zip(arr, keep):
            a.data, a.layout = capi.ptr(buf), capi.APS_IMG_U8_MATLAB
    if data is not None:
        keep = data
        for a, buf in zip(arr, keep):
            a.data = capi.ptr(buf)
    return arr, keep


def _render_entries(capi, arr, n, cv, ro, layout, H, W, where):
    """(pano, covered) bytes of the three render entry points, outputs pre-filled with 0xA5."""
    outs = []
    for entry, extra in (("aps_render", ()), ("aps_render_tiles", (1, 2)), ("aps_render_tile_range", (1, 3))):
        pano = place(sentinel_buffer(H * W * 3, np.uint8), where)
        cov = place(sentinel_buffer(H * W, np.uint8), where)
        capi.check(_call(capi, getattr(capi.lib, entry), arr, n, C.byref(cv), C.byref(ro), layout, *extra, capi.ptr(pano), capi.ptr(cov)))
        outs.append((fetch(pano).copy(), fetch(cov).copy()))
    return outs


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("legacy", [False, True], ids=["batched", "legacy"])
@pytest.mark.parametrize("blending", ["none", "linear", "multiband"])
def test_render_planar_images_and_planar_output(gpu, capi, monkeypatch, blending, legacy, where):
    """aps_mex.cpp:402-443: every image APS_IMG_U8_MATLAB (one of them gray), out_layout MATLAB, `covered` requested.
    Bytes must equal the HWC run's, transposed - all tiles, an interleaved share and a run of tiles."""
    rp = import_module(gpu.__name__ + ".renderPanorama")
    imgs, cams, geo, opts, gains = _render_scene_small(rp)
    if legacy:
        monkeypatch.setenv("APS_RENDER_LEGACY", "1")
    else:
        monkeypatch.delenv("APS_RENDER_LEGACY", raising=False)
    cv = rp.make_canvas_struct(geo)
    ro = rp.make_render_opts(dict(opts, blending=blending, tile=(24, 40)))
    H, W = geo["H"], geo["W"]
    a_hwc, keep0 = _structs(rp, capi, imgs, cams, gains, False)
    a_pl, keep1 = _structs(rp, capi, imgs, cams, gains, True)
    ref = _render_entries(capi, a_hwc, 3, cv, ro, capi.APS_IMG_U8_HWC, H, W, "host")
    got = _render_entries(capi, a_pl, 3, cv, ro, capi.APS_IMG_U8_MATLAB, H, W, where)
    mixed = _render_entries(capi, a_pl, 3, cv, ro, capi.APS_IMG_U8_HWC, H, W, where)  # planar in, HWC out
    full_p, full_c = ref[0][0].reshape(H, W, 3), ref[0][1].reshape(H, W)
    assert full_c.sum() > 1500 and (full_c == 0).sum() > 100 and set(np.unique(full_c)) == {0, 1}
    seen = full_p[full_c == 1]
    assert (seen[:, 0] != seen[:, 1]).mean() > 0.5 and (seen[:, 1] != seen[:, 2]).mean() > 0.5  # a channel swap would show
    for (rp_, rc_), (gp, gc), (mp, mc), name in zip(ref, got, mixed, ("all", "tiles 1 mod 2", "tiles 1..2")):
        assert np.array_equal(from_planar(gc, (H, W)), rc_.reshape(H, W)), name
        assert np.array_equal(from_planar(gp, (H, W, 3)), rp_.reshape(H, W, 3)), name
        assert np.array_equal(mp, rp_) and np.array_equal(mc, rc_), name
    # the shares leave the rest of the canvas to the caller: the sentinel is still there, in both layouts
    for k in (1, 2):
        assert (ref[k][1] == 0xA5).sum() > 0 and np.array_equal(from_planar(got[k][1], (H, W)) == 0xA5, ref[k][1].reshape(H, W) == 0xA5)
    del keep0, keep1


@pytest.mark.parametrize("blending", ["linear", "multiband"])
def test_render_from_unaligned_resident_images(gpu, capi, blending):
    """to_rgba_batch_kernel's byte path: HWC images on the device whose base pointers are 1, 2, 3 bytes off a dword
    (w = 53: w % 4 != 0).  Every byte equals the aligned call's."""
    rp = import_module(gpu.__name__ + ".renderPanorama")
    imgs, cams, geo, opts, gains = _render_scene_small(rp, gray=None)
    cv = rp.make_canvas_struct(geo)
    ro = rp.make_render_opts(dict(opts, blending=blending, tile=(24, 40)))
    H, W = geo["H"], geo["W"]
    arr, keep = _structs(rp, capi, imgs, cams, gains, False)
    ref = _render_entries(capi, arr, 3, cv, ro, capi.APS_IMG_U8_HWC, H, W, "host")[0]
    assert ref[1].sum() > 1500
    for offs in ((1, 2, 3), (3, 0, 1), (2, 2, 2)):
        data = [_misaligned(im, o) for im, o in zip(imgs, offs)]
        arr2, keep2 = _structs(rp, capi, imgs, cams, gains, False, data=data)
        got = _render_entries(capi, arr2, 3, cv, ro, capi.APS_IMG_U8_HWC, H, W, "host")[0]
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), offs
    del keep


# ---- gain statistics ---------------------------------------------------------------------------------------------------
def test_gain_overlap_stats_on_planar_images(gpu, capi):
    """aps_mex.cpp:446-480.  Counts equal and sums BIT-equal to the HWC call: every pixel is >= 32, so every bilinear sample
    is an f32 >= 16, a multiple of 2^-19; fewer than 2^20 of them below 2^8 sum to less than 2^28, 47 bits - the f64 sums
    are exact whatever order the atomics land in."""
    rp = import_module(gpu.__name__ + ".renderPanorama")
    imgs, cams, geo, _, _ = _render_scene_small(rp)
    imgs = [(32 + (im.astype(np.int32) * 223) // 255).astype(np.uint8) for im in imgs]
    cv = rp.make_canvas_struct(geo)
    res = []
    for planar in (False, True):
        arr, keep = _structs(rp, capi, imgs, cams, None, planar)
        N, sI, sJ = (np.zeros(9, np.float64), np.zeros(27, np.float64), np.zeros(27, np.float64))
        capi.check(_call(capi, capi.lib.aps_gain_overlap_stats, arr, 3, C.byref(cv), 1, capi.ptr(N), capi.ptr(sI), capi.ptr(sJ)))
        res.append((N, sI, sJ))
        del keep
    assert res[0][0].sum() > 500 and (res[0][0] > 0).sum() >= 2
    for a, b in zip(*res):
        assert same_bits(a, b)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("ch", [3, 1])
def test_gain_overlap_stats_warped_column_major(gpu, capi, where, ch):
    """aps_mex.cpp:506: MATLAB's planar column-major canvases.  Colours are multiples of 1/256 in [0, 1): the f64 sums are
    exact in any order, so they must equal the row-major call's and the oracle's bit for bit."""
    rng = np.random.default_rng(100 + ch)
    n, Hc, Wc, ds = 4, 35, 47, 3
    Iw = [(rng.integers(0, 256, (Hc, Wc, ch)) / 256).astype(np.float32) for _ in range(n)]
    Ww = [((rng.random((Hc, Wc)) > 0.3) * rng.random((Hc, Wc))).astype(np.float32) for _ in range(n)]
    Iw[1][::5, ::3, ch - 1] = np.nan
    Iw[2][3::7, 1::4, 0] = np.inf
    res = []
    for colmajor in (False, True):
        ia = [place(np.ascontiguousarray(a.ravel(order="F" if colmajor else "C")), where) for a in Iw]
        wa = [place(np.ascontiguousarray(a.ravel(order="F" if colmajor else "C")), where) for a in Ww]
        pi = (C.c_void_p * n)(*[capi.ptr(a) for a in ia])
        pw = (C.c_void_p * n)(*[capi.ptr(a) for a in wa])
        N, sI, sJ = (np.zeros(n * n, np.float64), np.zeros(3 * n * n, np.float64), np.zeros(3 * n * n, np.float64))
        capi.check(_call(capi, capi.lib.aps_gain_overlap_stats_warped, C.addressof(pi), C.addressof(pw), n, Hc, Wc, ch,
                         capi.APS_COLMAJOR if colmajor else capi.APS_ROWMAJOR, ds, capi.ptr(N), capi.ptr(sI), capi.ptr(sJ)))
        res.append((N, sI, sJ))
    oN, oI, oJ = oracle.gain_overlap_stats_warped(Iw, Ww, ds)
    assert oN.sum() > 50
    for a, b, o in zip(res[0], res[1], (oN, oI, oJ)):
        assert same_bits(a, b) and same_bits(b, np.ascontiguousarray(o.ravel(order="F")))


# ---- aps_imresize_u8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("method", ["bilinear", "bicubic"])
@pytest.mark.parametrize("shape,arg", [((37, 53, 3), (20, 40)),   # scale_r < scale_c: rows first
                                       ((37, 53, 3), (30, 21)),   # columns first
                                       ((35, 47), (17, 30)),      # one channel
                                       ((129, 66, 3), 0.37),      # scalar form, shrink
                                       ((35, 47, 3), 1.7)])       # scalar form, enlarge
def test_imresize_u8_planar(capi, shape, arg, method, where):
    """aps_mex.cpp:521: planar in, planar out, through u8_index in both dimension orders."""
    rng = np.random.default_rng(sum(shape) + len(method))
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    h, w = shape[:2]
    c = 1 if len(shape) == 2 else shape[2]
    ref = oracle.imresize_u8(img, arg, method)
    oh, ow = ref.shape[:2]
    sr, sc = (arg, arg) if np.isscalar(arg) else (oh / h, ow / w)
    m = capi.APS_RESIZE_BICUBIC if method == "bicubic" else capi.APS_RESIZE_BILINEAR
    outs = {}
    for layout in (capi.APS_IMG_U8_HWC, capi.APS_IMG_U8_MATLAB):
        src = place(to_planar(img) if layout == capi.APS_IMG_U8_MATLAB else np.ascontiguousarray(img).reshape(-1), where)
        out = place(sentinel_buffer(oh * ow * c + 16, np.uint8), where)
        capi.check(_call(capi, capi.lib.aps_imresize_u8, capi.ptr(src), h, w, c, layout, oh, ow, float(sr), float(sc), m, capi.ptr(out)))
        o = fetch(out)
        assert np.all(o[oh * ow * c:] == 0xA5)
        outs[layout] = from_planar(o[:oh * ow * c], ref.shape) if layout == capi.APS_IMG_U8_MATLAB else o[:oh * ow * c].reshape(ref.shape)
    assert np.array_equal(outs[capi.APS_IMG_U8_MATLAB], outs[capi.APS_IMG_U8_HWC])
    assert np.array_equal(outs[capi.APS_IMG_U8_MATLAB], ref)


# ---- crop --------------------------------------------------------------------------------------------------------------
def _pano(rng, h, w, white):
    img = np.full((h, w, 3), 255 if white else 0, np.uint8)
    img[h // 5: h - h // 3, w // 4: w - w // 6] = rng.integers(1, 250, (h - h // 3 - h // 5, w - w // 6 - w // 4, 3))
    img[h - 2, 1] = (3, 200, 90) if not white else (250, 10, 90)  # a lone pixel whose position only the right index finds
    return img


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("h,w", [(37, 53), (129, 66), (35, 48)])
def test_crop_nonzero_bbox_planar(capi, h, w, white, where):
    """aps_mex.cpp:604: crop_bbox_kernel's planar branch, both canvas colours, against the HWC call and the oracle."""
    img = _pano(np.random.default_rng(h + w), h, w, white)
    want_rect, want_did = oracle.crop_nonzero_bbox(img, white)
    assert want_did and want_rect != (1, h, 1, w)
    for layout, buf in ((capi.APS_IMG_U8_HWC, np.ascontiguousarray(img).reshape(-1)), (capi.APS_IMG_U8_MATLAB, to_planar(img))):
        rect, did = np.zeros(4, np.int64), C.c_int(0)
        src = place(buf, where)
        capi.check(_call(capi, capi.lib.aps_crop_nonzero_bbox, capi.ptr(src), h, w, layout, int(white), capi.ptr(rect), C.byref(did)))
        assert tuple(int(v) for v in rect) == want_rect and bool(did.value) == want_did, layout


@pytest.mark.parametrize("w", [53, 52])
def test_crop_nonzero_bbox_from_an_unaligned_resident_image(capi, w):
    """crop_bbox_kernel's byte path: an HWC panorama on the device, base pointer 1, 2, 3 bytes off a dword."""
    img = _pano(np.random.default_rng(w), 37, w, False)
    want_rect, want_did = oracle.crop_nonzero_bbox(img, False)
    for off in (0, 1, 2, 3):
        rect, did = np.zeros(4, np.int64), C.c_int(0)
        src = _misaligned(img, off)
        capi.check(_call(capi, capi.lib.aps_crop_nonzero_bbox, capi.ptr(src), 37, w, capi.APS_IMG_U8_HWC, 0, capi.ptr(rect), C.byref(did)))
        assert tuple(int(v) for v in rect) == want_rect and bool(did.value) == want_did, off


@pytest.mark.parametrize("where", WHERE)
def test_crop_rect_planar(capi, where):
    """aps_mex.cpp:532, on a shape where a transposed index stays in bounds."""
    rng = np.random.default_rng(5)
    img = _pano(rng, 66, 129, False)
    img[20:30, 40:50] = 0  # a hole for imfill
    want_rect, want_ok, _ = oracle.crop_rect(img)
    for layout, buf in ((capi.APS_IMG_U8_HWC, np.ascontiguousarray(img).reshape(-1)), (capi.APS_IMG_U8_MATLAB, to_planar(img))):
        rect, valid = np.zeros(4, np.int32), np.zeros(1, np.int32)
        src = place(buf, where)
        capi.check(_call(capi, capi.lib.aps_crop_rect, capi.ptr(src), 66, 129, layout, 0, 0.0, capi.ptr(rect), capi.ptr(valid)))
        assert tuple(int(v) for v in rect) == want_rect and bool(valid[0]) == want_ok, layout


# ---- k-NN, Hamming, matching: APS_COLMAJOR with ld > n ----------------------------------------------------------------------
def _knn_out(capi, fn, args_in, fq, k, colmajor, ldo, where):
    idx = place(sentinel_buffer((k if colmajor else fq) * ldo, np.uint32), where)
    dist = place(sentinel_buffer((k if colmajor else fq) * ldo, np.float32), where)
    capi.check(_call(capi, fn, *args_in, capi.APS_COLMAJOR if colmajor else capi.APS_ROWMAJOR, k, capi.ptr(idx), capi.ptr(dist), ldo))
    i, ok_i = unpad(fetch(idx, np.uint32), fq, k, colmajor, ldo)
    d, ok_d = unpad(fetch(dist), fq, k, colmajor, ldo)
    return i, d, ok_i and ok_d


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("ft,fq,k", [(257, 1000, 4), (1000, 257, 2), (3, 37, 4), (0, 5, 2)])
def test_knn_global_column_major_padded(capi, ft, fq, k, where):
    """aps_mex.cpp:232 with ldt, ldq, ldo all larger than the row counts; row counts that cross a tile, fewer train rows
    than k (index 0 / Inf in the missing slots) and none at all."""
    rng = np.random.default_rng(ft + fq)
    T, Q = sift_like(rng, ft), sift_like(rng, fq)
    Tc, Qc = place(padded(T, True, ft + 7), where), place(padded(Q, True, fq + 5), where)
    i, d, intact = _knn_out(capi, capi.lib.aps_knn_global, (capi.ptr(Tc), ft, ft + 7, capi.ptr(Qc), fq, fq + 5, 128), fq, k, True, fq + 3, where)
    Tr, Qr = np.ascontiguousarray(T), np.ascontiguousarray(Q)
    i0, d0, _ = _knn_out(capi, capi.lib.aps_knn_global, (capi.ptr(Tr) if ft else None, ft, 128, capi.ptr(Qr), fq, 128, 128), fq, k, False, k, "host")
    ir, dr, intact_r = _knn_out(capi, capi.lib.aps_knn_global, (capi.ptr(Tr) if ft else None, ft, 128, capi.ptr(Qr), fq, 128, 128), fq, k, False,
                                k + 3, where)
    oi, od = oracle.knn(T, Q, k)
    assert same_bits(i, i0) and same_bits(d, d0) and same_bits(ir, i0) and same_bits(dr, d0)
    assert same_bits(i, oi) and same_bits(d, od)
    assert intact and intact_r, "elements outside the fq x k result were written"


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("ft,fq,k,nb", [(257, 1000, 4, 32), (1000, 257, 2, 64), (3, 37, 4, 32)])
def test_knn_hamming_column_major_padded(capi, ft, fq, k, nb, where):
    """aps_mex.cpp:229."""
    rng = np.random.default_rng(ft + fq + nb)
    T, Q = rng.integers(0, 256, (ft, nb), dtype=np.uint8), rng.integers(0, 256, (fq, nb), dtype=np.uint8)
    Q[::7] = T[rng.integers(0, ft, len(Q[::7]))]  # exact hits and ties
    Tc, Qc = place(padded(T, True, ft + 7), where), place(padded(Q, True, fq + 5), where)
    i, d, intact = _knn_out(capi, capi.lib.aps_knn_hamming, (capi.ptr(Tc), ft, ft + 7, capi.ptr(Qc), fq, fq + 5, nb), fq, k, True, fq + 3, where)
    i0, d0, _ = _knn_out(capi, capi.lib.aps_knn_hamming, (capi.ptr(T), ft, nb, capi.ptr(Q), fq, nb, nb), fq, k, False, k, "host")
    ir, dr, intact_r = _knn_out(capi, capi.lib.aps_knn_hamming, (capi.ptr(T), ft, nb, capi.ptr(Q), fq, nb, nb), fq, k, False, k + 3, where)
    oi, od = oracle.knn_hamming(T, Q, k)
    assert same_bits(i, i0) and same_bits(d, d0) and same_bits(ir, i0) and same_bits(dr, d0)
    assert same_bits(i, np.ascontiguousarray(oi, np.uint32)) and same_bits(d, np.ascontiguousarray(od, np.float32))
    assert intact and intact_r, "elements outside the fq x k result were written"


def _two_nn(capi, fn, A, lda, n1, B, ldb, n2, width, layout, extra, where, tail=()):
    idx = place(sentinel_buffer(n1 + 9, np.uint32), where)
    d1, d2 = place(sentinel_buffer(n1 + 9, np.float32), where), place(sentinel_buffer(n1 + 9, np.float32), where)
    capi.check(_call(capi, fn, capi.ptr(A), n1, lda, capi.ptr(B), n2, ldb, width, layout, *extra, capi.ptr(idx), capi.ptr(d1), capi.ptr(d2), *tail))
    outs = [fetch(idx, np.uint32), fetch(d1), fetch(d2)]
    intact = all(same_bits(o[n1:], sentinel_buffer(9, o.dtype)) for o in outs)
    return [o[:n1].copy() for o in outs], intact


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n1,n2", [(257, 1000), (1000, 257), (3, 1)])
def test_hamming_2nn_column_major_padded(capi, n1, n2, where):
    """aps_mex.cpp:247."""
    rng = np.random.default_rng(n1 + n2)
    A, B = rng.integers(0, 256, (n1, 32), dtype=np.uint8), rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    A[::5] = B[rng.integers(0, n2, len(A[::5]))]
    got, intact = _two_nn(capi, capi.lib.aps_hamming_2nn, place(padded(A, True, n1 + 7), where), n1 + 7, n1, place(padded(B, True, n2 + 5), where),
                          n2 + 5, n2, 32, capi.APS_COLMAJOR, (), where)
    ref, _ = _two_nn(capi, capi.lib.aps_hamming_2nn, A, 32, n1, B, 32, n2, 32, capi.APS_ROWMAJOR, (), "host")
    pad_r, _ = _two_nn(capi, capi.lib.aps_hamming_2nn, place(padded(A, False, 32 + 7), where), 39, n1, place(padded(B, False, 32 + 5), where), 37, n2,
                       32, capi.APS_ROWMAJOR, (), where)
    want = oracle.hamming_2nn(A, B)
    for g, r, p, o in zip(got, ref, pad_r, want):
        assert same_bits(g, r) and same_bits(p, r) and same_bits(g, np.ascontiguousarray(o, g.dtype))
    assert intact


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n1,n2", [(257, 1000), (1000, 257), (5, 3)])
def test_match_pca2nn_column_major_padded(capi, n1, n2, where):
    """aps_mex.cpp:116."""
    rng = np.random.default_rng(n1 * 3 + n2)
    A, B, _, _ = planted_pair(rng, n1, n2, min(n1, n2) // 2)
    got, intact = _two_nn(capi, capi.lib.aps_match_pca2nn, place(padded(A, True, n1 + 7), where), n1 + 7, n1, place(padded(B, True, n2 + 5), where),
                          n2 + 5, n2, 128, capi.APS_COLMAJOR, (48, 1), where, tail=(None, None))  # (mu_out, coeff_out: NULL, as the gateway passes)
    ref, _ = _two_nn(capi, capi.lib.aps_match_pca2nn, A, 128, n1, B, 128, n2, 128, capi.APS_ROWMAJOR, (48, 1), "host", tail=(None, None))
    want = oracle.pca2nn(A, B, 48, True)
    for g, r, o in zip(got, ref, want):
        assert same_bits(g, r) and same_bits(g, np.ascontiguousarray(o, g.dtype))
    assert intact


def _match_features(capi, A, lda, n1, B, ldb, n2, layout, cap, where):
    o = capi.aps_match_opts(0.6, 1.5, 1, 2)
    i1, i2 = place(sentinel_buffer(cap, np.uint32), where), place(sentinel_buffer(cap, np.uint32), where)
    met = place(sentinel_buffer(cap, np.float32), where)
    cnt = C.c_int64(0)
    capi.check(_call(capi, capi.lib.aps_match_features, capi.ptr(A), n1, lda, capi.ptr(B), n2, ldb, 128, layout, C.byref(o), capi.ptr(i1),
                     capi.ptr(i2), capi.ptr(met), cap, C.byref(cnt)))
    k = int(cnt.value)
    outs = [fetch(i1, np.uint32), fetch(i2, np.uint32), fetch(met)]
    intact = all(same_bits(x[k:], sentinel_buffer(cap - k, x.dtype)) for x in outs)
    return k, [x[:k].copy() for x in outs], intact


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n1,n2", [(257, 1000), (1000, 257), (3, 5)])
def test_match_features_column_major_padded(capi, n1, n2, where):
    """aps_mex.cpp:95, and rows count..cap of the three outputs."""
    rng = np.random.default_rng(n1 + 2 * n2)
    A, B, _, _ = planted_pair(rng, n1, n2, min(n1, n2) // 2)
    k, got, intact = _match_features(capi, place(padded(A, True, n1 + 7), where), n1 + 7, n1, place(padded(B, True, n2 + 5), where), n2 + 5, n2,
                                     capi.APS_COLMAJOR, n1 + 11, where)
    k0, ref, _ = _match_features(capi, A, 128, n1, B, 128, n2, capi.APS_ROWMAJOR, n1, "host")
    om, omet = oracle.match_features(A, B, 0.6, 1.5, True, 2)
    assert k == k0 == len(om) and (n1 < 100 or k > 50)
    assert all(same_bits(g, r) for g, r in zip(got, ref))
    assert np.array_equal(np.stack(got[:2], 1), om) and same_bits(got[2], omet)
    assert intact, "rows count..cap of idx1 / idx2 / metric were written"


@pytest.mark.parametrize("where", WHERE)
def test_match_pairwise_column_major_padded(capi, where):
    """aps_mex.cpp:146: per-image column-major sets with ld[i] > counts[i] (one image empty), outputs with cap > count."""
    rng = np.random.default_rng(8)
    counts = [257, 300, 0, 129]
    base = sift_like(rng, 400)
    sets = []
    for n in counts:
        s = sift_like(rng, n)
        if n:
            take = rng.permutation(400)[: n // 2]
            s[: n // 2] = base[take]
        sets.append(s)
    n_img, n_pairs = len(sets), 6

    def run(layout, lds, bufs, cap, where_):
        ptrs = (C.c_void_p * n_img)(*[capi.ptr(b) if c else None for b, c in zip(bufs, counts)])
        cnts, ld = (C.c_int64 * n_img)(*counts), (C.c_int64 * n_img)(*lds)
        o = capi.aps_match_opts(0.6, 1.5, 1, 2)
        pp = np.zeros(n_pairs + 1, np.int64)
        ii, jj = place(sentinel_buffer(cap, np.uint32), where_), place(sentinel_buffer(cap, np.uint32), where_)
        met = place(sentinel_buffer(cap, np.float32), where_)
        cnt = C.c_int64(0)
        capi.check(_call(capi, capi.lib.aps_match_pairwise, ptrs, cnts, ld, n_img, 128, layout, C.byref(o), capi.ptr(pp), capi.ptr(ii), capi.ptr(jj),
                         capi.ptr(met), cap, C.byref(cnt)))
        k = int(cnt.value)
        outs = [fetch(ii, np.uint32), fetch(jj, np.uint32), fetch(met)]
        return k, pp, [x[:k].copy() for x in outs], all(same_bits(x[k:], sentinel_buffer(cap - k, x.dtype)) for x in outs)

    cap = sum(counts)
    k, pp, got, intact = run(capi.APS_COLMAJOR, [c + 7 for c in counts], [place(padded(s, True, len(s) + 7), where) for s in sets], cap + 13, where)
    k0, pp0, ref, _ = run(capi.APS_ROWMAJOR, [128] * n_img, sets, cap, "host")
    assert k == k0 > 50 and np.array_equal(pp, pp0) and all(same_bits(g, r) for g, r in zip(got, ref))
    p = 0
    for j in range(1, n_img):
        for i in range(j):
            om, omet = oracle.match_features(sets[i], sets[j], 0.6, 1.5, True, 2) if counts[i] and counts[j] else (np.zeros((0, 2), np.uint32), np.zeros(0, np.float32))
            s, e = int(pp[p]), int(pp[p + 1])
            assert e - s == len(om) and np.array_equal(np.stack([got[0][s:e], got[1][s:e]], 1), om) and same_bits(got[2][s:e], omet), (i, j)
            p += 1
    assert intact, "rows count..cap of idx_i / idx_j / metric were written"


# ---- RANSAC, BA blocks, the gather: leading dimensions larger than the row count -----------------------------------------------
def _pts(p, ld, where):
    return place(padded(np.ascontiguousarray(p, np.float64), True, ld), where)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("method", ["ransac", "mlesac"])
def test_ransac_homography_padded_points(gpu, capi, method, where):
    """aps_mex.cpp:280 with ldp > m: model bits, mask and verdict equal the tight call's and the oracle's; the mask's tail
    (a buffer longer than m) stays untouched."""
    im = import_module(gpu.__name__ + ".imageMatching")
    m = 257
    rng = np.random.default_rng(20 + m)
    p1, p2, _ = make_scene(rng, m, 90, H_TRUE, noise=0.3)
    s = np.ascontiguousarray(im.draw_samples([m], 564, seed=m)[0], np.uint32)
    o = capi.aps_ransac_opts(5.5, 99.9, 500, capi.APS_TFORM_PROJECTIVE, capi.APS_ROBUST_MLESAC if method == "mlesac" else capi.APS_ROBUST_RANSAC)

    def run(ldp, where_):
        model, mask = place(sentinel_buffer(9 + 3, np.float64), where_), place(sentinel_buffer(m + 9, np.uint8), where_)
        found, trials = C.c_int(0), C.c_int(0)
        a = _pts(p1, ldp, where_) if ldp > m else np.asfortranarray(p1)
        b = _pts(p2, ldp, where_) if ldp > m else np.asfortranarray(p2)
        capi.check(_call(capi, capi.lib.aps_ransac_homography, capi.ptr(a), capi.ptr(b), m, ldp, capi.ptr(s), s.shape[0], C.byref(o),
                         capi.ptr(model), capi.ptr(mask), C.byref(found), C.byref(trials)))
        mo, ma = fetch(model), fetch(mask)
        return found.value, trials.value, mo[:9].copy(), ma[:m].copy(), same_bits(mo[9:], sentinel_buffer(3, np.float64)) and np.all(ma[m:] == 0xA5)

    f1, t1, H1, m1, intact = run(m + 7, where)
    f0, t0, H0, m0, _ = run(m, "host")
    assert f1 == f0 == 1 and t1 == t0 and same_bits(H1, H0) and np.array_equal(m1, m0) and m1.sum() > 100
    if method == "ransac":
        oH, omask, ofound, _ = oracle.ransac_homography(p1, p2, s, 5.5, 99.9, 500)
    else:
        oH, omask, ofound, _ = oracle.mlesac_homography(p1, p2, s, 5.5, 99.9, 500)
    assert ofound and np.array_equal(m1.astype(bool), np.asarray(omask).astype(bool)) and same_bits(H1.reshape(3, 3).T, np.ascontiguousarray(oH))
    assert intact


@pytest.mark.parametrize("where", WHERE)
def test_ransac_homography_batch_padded_points(gpu, capi, where):
    """aps_mex.cpp:350 with ldp > total."""
    im = import_module(gpu.__name__ + ".imageMatching")
    rng = np.random.default_rng(31)
    sizes = [257, 40, 4, 129]
    P1, P2 = [], []
    for k, m in enumerate(sizes):
        a, b, _ = make_scene(rng, m, m // 3, H_TRUE, noise=0.3)
        P1.append(a)
        P2.append(b)
    p1, p2 = np.concatenate(P1), np.concatenate(P2)
    total, P = len(p1), len(sizes)
    pp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    s = np.ascontiguousarray(np.stack(im.draw_samples(sizes, 300, seed=5)), np.uint32)
    assert s.shape == (P, 300, 4)
    o = capi.aps_ransac_opts(5.5, 99.9, 200, capi.APS_TFORM_PROJECTIVE, capi.APS_ROBUST_RANSAC)

    def run(ldp, where_):
        a = _pts(p1, ldp, where_) if ldp > total else np.asfortranarray(p1)
        b = _pts(p2, ldp, where_) if ldp > total else np.asfortranarray(p2)
        models, mask = place(sentinel_buffer(9 * P + 5, np.float64), where_), place(sentinel_buffer(total + 9, np.uint8), where_)
        found, ninl = place(sentinel_buffer(P + 2, np.int32), where_), place(sentinel_buffer(P + 2, np.int32), where_)
        capi.check(_call(capi, capi.lib.aps_ransac_homography_batch, capi.ptr(a), capi.ptr(b), ldp, capi.ptr(pp), P, capi.ptr(s),
                         300, C.byref(o), capi.ptr(models), capi.ptr(mask), capi.ptr(found), capi.ptr(ninl)))
        mo, ma, fo, ni = fetch(models), fetch(mask), fetch(found), fetch(ninl)
        intact = same_bits(mo[9 * P:], sentinel_buffer(5, np.float64)) and np.all(ma[total:] == 0xA5) and np.all(fo[P:] == -1) and np.all(ni[P:] == -1)
        return mo[:9 * P].copy(), ma[:total].copy(), fo[:P].copy(), ni[:P].copy(), intact

    g = run(total + 7, where)
    r = run(total, "host")
    assert all(same_bits(x, y) for x, y in zip(g[:4], r[:4])) and g[2][0] == 1 and g[3][0] > 100
    for k in range(P):
        oH, omask, ofound, _ = oracle.ransac_homography(P1[k], P2[k], s[k], 5.5, 99.9, 200)
        assert bool(g[2][k]) == bool(ofound) and np.array_equal(g[1][pp[k]:pp[k + 1]].astype(bool), np.asarray(omask).astype(bool)), k
        if ofound:
            assert same_bits(g[0][9 * k:9 * k + 9].reshape(3, 3).T, np.ascontiguousarray(oH)), k
    assert g[4]


@pytest.mark.parametrize("where", WHERE)
def test_ba_pair_blocks_padded_points(capi, where):
    """aps_mex.cpp:554 with ldu > total."""
    rng = np.random.default_rng(10)
    packs, Uis, Ujs, ptr = [], [], [], [0]
    for m in (1, 63, 65, 0, 257):
        ci, cj, Ui, Uj = _ba_scene(rng, max(m, 1))
        li = dict(ci, f=ci["f"] + rng.normal(0, 2), R=_rot(rng, 0.01) @ ci["R"])
        lj = dict(cj, f=cj["f"] + rng.normal(0, 2), R=_rot(rng, 0.01) @ cj["R"])
        packs.append(np.stack([_pack(c) for c in (ci, cj, li, lj)]))
        Uis.append(Ui[:m])
        Ujs.append(Uj[:m])
        ptr.append(ptr[-1] + m)
    Ui, Uj, cams = np.concatenate(Uis), np.concatenate(Ujs), np.ascontiguousarray(np.stack(packs), np.float64)
    total, P = len(Ui), len(packs)
    pp = np.asarray(ptr, np.int64)

    def run(ldu, where_):
        a = _pts(Ui, ldu, where_) if ldu > total else np.asfortranarray(Ui)
        b = _pts(Uj, ldu, where_) if ldu > total else np.asfortranarray(Uj)
        out = place(sentinel_buffer(59 * P + 4, np.float64), where_)
        capi.check(_call(capi, capi.lib.aps_ba_pair_blocks, capi.ptr(a), capi.ptr(b), ldu, capi.ptr(pp), P, capi.ptr(cams), 2.0, 1,
                         capi.ptr(out)))
        o = fetch(out)
        return o[:59 * P].copy(), same_bits(o[59 * P:], sentinel_buffer(4, np.float64))

    got, intact = run(total + 7, where)
    ref, _ = run(total, "host")
    want = oracle.ba_pair_blocks(Ui, Uj, ptr, cams, 2.0, True)
    assert same_bits(got, ref) and same_bits(got, want.reshape(-1)) and got.reshape(P, 59)[4, 58] == 4 * 257 and intact


def test_gather_match_points_padded_output(capi):
    """aps_gather_match_points with ldp > total: the x column at [0, total), the y column at [ldp, ldp + total), the rest of the
    resident output untouched; values equal the tight call's and plain host indexing."""
    import torch

    rng = np.random.default_rng(3)
    kp = [np.ascontiguousarray(rng.uniform(0, 1000, (n, 2))) for n in (40, 0, 53, 37)]
    work = [(0, 2, 30), (2, 3, 35), (0, 3, 0)]
    ia = np.concatenate([rng.integers(1, len(kp[a]) + 1, m) for a, _, m in work]).astype(np.int32)
    ib = np.concatenate([rng.integers(1, len(kp[b]) + 1, m) for _, b, m in work]).astype(np.int32)
    ia[3] = 41  # outside image 0's table: NaN
    wptr = np.concatenate([[0], np.cumsum([m for _, _, m in work])]).astype(np.int64)
    starts = wptr[:-1].copy()
    total = int(wptr[-1])
    kt = [torch.from_numpy(k).cuda() for k in kp]
    tab = (C.c_void_p * 4)(*[t.data_ptr() if t.numel() else None for t in kt])
    cnt = np.asarray([len(k) for k in kp], np.int64)
    img_a, img_b = np.asarray([w[0] for w in work], np.int32), np.asarray([w[1] for w in work], np.int32)
    da, db = place(ia, "device"), place(ib, "device")

    def run(ldp):
        pa, pb = place(sentinel_buffer(2 * ldp, np.float64), "device"), place(sentinel_buffer(2 * ldp, np.float64), "device")
        capi.check(_call(capi, capi.lib.aps_gather_match_points, tab, capi.ptr(cnt), 4, capi.ptr(da), capi.ptr(db), capi.ptr(starts), capi.ptr(wptr),
                         capi.ptr(img_a), capi.ptr(img_b), len(work), capi.ptr(pa), capi.ptr(pb), ldp))
        (a, ok_a), (b, ok_b) = unpad(fetch(pa), total, 2, True, ldp), unpad(fetch(pb), total, 2, True, ldp)
        return a, b, ok_a and ok_b

    a, b, intact = run(total + 7)
    pa0, pb0 = place(np.zeros(2 * total, np.float64), "device"), place(np.zeros(2 * total, np.float64), "device")
    capi.check(_call(capi, capi.lib.aps_gather_match_points, tab, capi.ptr(cnt), 4, capi.ptr(da), capi.ptr(db), capi.ptr(starts), capi.ptr(wptr),
                     capi.ptr(img_a), capi.ptr(img_b), len(work), capi.ptr(pa0), capi.ptr(pb0), total))
    a0, b0 = fetch(pa0).reshape(2, total).T, fetch(pb0).reshape(2, total).T
    assert same_bits(a, np.ascontiguousarray(a0)) and same_bits(b, np.ascontiguousarray(b0)) and intact
    want_a = np.concatenate([kp[w[0]][np.minimum(ia[s:s + w[2]], len(kp[w[0]])) - 1] for w, s in zip(work, starts)])
    want_b = np.concatenate([kp[w[1]][ib[s:s + w[2]] - 1] for w, s in zip(work, starts)])
    ok = np.ones(total, bool)
    ok[3] = False
    assert np.isnan(a[3]).all() and same_bits(a[ok], want_a[ok]) and same_bits(b, want_b)
