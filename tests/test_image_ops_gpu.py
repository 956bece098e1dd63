"""imresize, imageWarp and resizeImagesToLimits on the device across the cases of image_ops_cases.py (test_image_ops_cases.py
holds the cases to what they were chosen for, on the CPU): block edges of the 128- and 256-lane launches, 62 and 64 taps, both
pass orders, sources and views of one pixel, rounding ties, both clamps, a zero and a clamped projective coordinate, degenerate
transforms, borders by known answer, one to four channels, planar layout and resident pointers.

Everything is compared without tolerance - uint8 by bytes, single by bits (a NaN equals a NaN: payloads are no part of the
contract) - against the oracle, whose arithmetic the kernels restate operation for operation in double.
resizeImagesToLimits is compared with image_ops_cases.limits_statement, the host statement of resizeImagesToLimits.m:17-106,
and pipeline.resize_per_component with resizeImagesToLimits(..., 'fit')."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import image_ops_cases as ic
from util import fetch, from_planar, place, same_bits, sentinel_buffer, to_planar

pytestmark = pytest.mark.gpu

WHERE = ["host", "device"]
PAD = 64  # sentinel elements behind every raw output


@pytest.fixture(scope="module")
def ip(gpu):
    return import_module(gpu.__name__ + ".imageProcessing")


@pytest.fixture(scope="module")
def capi(gpu):
    return gpu._capi


def _call(capi, fn, *args):
    """One ABI call bracketed the way a resident caller brackets it (test_abi_layouts_gpu._call)."""
    import torch

    torch.cuda.synchronize()
    rc = fn(*args)
    capi.check(capi.lib.aps_synchronize())
    return rc


# ---- every case through the Python layer ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ic.RESIZE_CASES, ids=lambda c: c.name)
def test_imresize_cases_equal_the_oracle(ip, c):
    import torch

    img, ref = ic.resize_image(c.name), ic.oracle_resize(c.name)
    out = ip.imresize(img, c.arg, c.method)
    assert same_bits(out, ref)
    res = ip.imresize(torch.from_numpy(img.copy()).cuda(), c.arg, c.method)  # resident in, resident out
    assert res.is_cuda and same_bits(res.cpu().numpy(), ref)


@pytest.mark.parametrize("c,method", ic.warp_runs(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_image_warp_cases_equal_the_oracle(ip, c, method):
    out = ip.imageWarp(ic.warp_source(c.name), np.array(c.H), ic.output_view(c), method, c.fill)
    assert ic.same_image(out, ic.oracle_warp(c.name, method))


# ---- aps_imresize_u8 as a C caller uses it ----------------------------------------------------------------------------------------------
RAW_RESIZE = [c for c in ic.RESIZE_CASES if c.name.startswith(("edge", "size", "tiny", "ch", "s15th", "s0.0646", "checker-s2-bicubic"))]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("c", RAW_RESIZE, ids=lambda c: c.name)
def test_imresize_raw_planar_and_resident(capi, c, where):
    """MATLAB planar layout in and out and the interleaved one, host and resident pointers; the bytes behind the output stay."""
    img, ref = ic.resize_image(c.name), ic.oracle_resize(c.name)
    h, w = c.shape[:2]
    ch = 1 if len(c.shape) == 2 else c.shape[2]
    oh, ow, sr, sc = ic.resize_target(c)
    m = capi.APS_RESIZE_BICUBIC if c.method == "bicubic" else capi.APS_RESIZE_BILINEAR
    n = oh * ow * ch
    for layout in (capi.APS_IMG_U8_MATLAB, capi.APS_IMG_U8_HWC):
        src = place((to_planar(img) if layout == capi.APS_IMG_U8_MATLAB else np.ascontiguousarray(img).reshape(-1)).copy(), where)
        out = place(sentinel_buffer(n + PAD, np.uint8), where)
        capi.check(_call(capi, capi.lib.aps_imresize_u8, capi.ptr(src), h, w, ch, layout, oh, ow, float(sr), float(sc), m, capi.ptr(out)))
        o = fetch(out)
        assert np.all(o[n:] == 0xA5), "bytes behind the output were written"
        got = from_planar(o[:n], ref.shape) if layout == capi.APS_IMG_U8_MATLAB else o[:n].reshape(ref.shape)
        assert same_bits(got, ref), layout


@pytest.mark.parametrize("where", WHERE)
def test_imresize_raw_refuses_what_it_does_not_build(capi, where):
    """A scale of 0.064 would need 66 taps (APS_E_ARG); five channels are no image (APS_E_DIM).  Nothing is written."""
    rng = np.random.default_rng(64)
    img = rng.integers(0, 256, (63, 32, 5), dtype=np.uint8)
    bic = capi.APS_RESIZE_BICUBIC
    for ch, s, want in ((3, 0.064, capi.APS_E_ARG), (5, 0.5, capi.APS_E_DIM)):
        src = place(np.ascontiguousarray(img[..., :ch]).reshape(-1), where)
        oh, ow = int(np.ceil(63 * s)), int(np.ceil(32 * s))
        out = place(sentinel_buffer(oh * ow * ch + PAD, np.uint8), where)
        rc = _call(capi, capi.lib.aps_imresize_u8, capi.ptr(src), 63, 32, ch, capi.APS_IMG_U8_HWC, oh, ow, s, s, bic, capi.ptr(out))
        assert rc == want, (ch, s, rc)
        assert np.all(fetch(out) == 0xA5)
    # the scale just above is built: 64 taps (case s0.0646-bicubic)
    assert 4.0 / 0.0646 + 2 <= ic.MAX_TAPS < 4.0 / 0.064 + 2


# ---- the raw warp entries ------------------------------------------------------------------------------------------------------------------
RAW_WARP = ("w257", "w257-f32", "extents-u8", "extents-f32", "persp-w0-u8", "tiny-w-f32", "nan-u8", "small-f32", "ch4-u8", "ch2-f32",
            "border-int-u8", "border-below-half-f32", "src2x2", "one-u8", "nan-src-f32")


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", RAW_WARP)
def test_warp_raw_entries_agree_and_leave_the_padding(capi, name, where):
    """aps_image_warp_h_u8 / _h_f32 are aps_image_warp_u8 / _f32 with the bilinear method; every method equals the oracle; the
    elements behind the output stay."""
    c, src_img = ic.WARP_BY_NAME[name], ic.warp_source(name)
    v = c.view
    h, w, ch = c.shape
    u8 = c.dtype == "u8"
    dt = np.uint8 if u8 else np.float32
    Hc = np.ascontiguousarray(np.array(c.H, np.float64).T)  # column-major 3 x 3, read on the host
    fill = C.c_uint8(int(c.fill)) if u8 else C.c_float(float(c.fill))
    n = v.oh * v.ow * ch
    lib = capi.lib
    full, short = (lib.aps_image_warp_u8, lib.aps_image_warp_h_u8) if u8 else (lib.aps_image_warp_f32, lib.aps_image_warp_h_f32)
    codes = {"nearest": capi.APS_WARP_NEAREST, "bilinear": capi.APS_WARP_BILINEAR, "bicubic": capi.APS_WARP_BICUBIC}

    def run(fn, *method):
        src = place(np.ascontiguousarray(src_img).reshape(-1).copy(), where)
        out = place(sentinel_buffer(n + PAD, dt), where)
        capi.check(_call(capi, fn, capi.ptr(src), h, w, ch, capi.ptr(Hc), v.oh, v.ow, v.x0, v.y0, v.sx, v.sy, fill, *method, capi.ptr(out)))
        o = fetch(out)
        assert same_bits(o[n:], sentinel_buffer(PAD, dt)), "elements behind the output were written"
        return o[:n].reshape(v.oh, v.ow, ch)

    for method in c.methods:
        assert ic.same_image(run(full, codes[method]), ic.oracle_warp(name, method)), method
    assert ic.same_image(run(short), run(full, capi.APS_WARP_BILINEAR))
    if "bilinear" in c.methods:
        assert ic.same_image(run(short), ic.oracle_warp(name, "bilinear"))


# ---- resizeImagesToLimits and pipeline.resize_per_component -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ic.LIMIT_MODES)
@pytest.mark.parametrize("s", ic.LIMIT_SETS, ids=lambda s: s.name)
def test_resize_images_to_limits_equals_the_host_statement(ip, s, mode):
    imgs = list(ic.limit_images(s.name))
    want = ic.limits_statement(imgs, s.limits[0], s.limits[1], mode)
    got = ip.resizeImagesToLimits(imgs, s.limits[0], s.limits[1], mode)
    assert len(got) == len(want)
    for g, w_ in zip(got, want):
        assert same_bits(g, w_)
    if s.name.startswith("a-"):
        assert all(g is i for g, i in zip(got, imgs))  # resizeImagesToLimits.m:29-42: the input, untouched, in every mode


def test_resize_images_to_limits_rejects_what_the_reference_rejects(ip):
    img = ic.limit_images("a-equal-within")[0]
    for bad in ([], ()):
        with pytest.raises(ValueError):
            ip.resizeImagesToLimits(bad, 40, 50, "fit")
    for HL, WL in ((0, 50), (40, 0), (-1, 50), (40, -3.5)):
        for mode in ic.LIMIT_MODES:
            with pytest.raises(ValueError):
                ip.resizeImagesToLimits([img], HL, WL, mode)


@pytest.mark.parametrize("kind", ["numpy", "cuda"])
@pytest.mark.parametrize("s", ic.LIMIT_SETS, ids=lambda s: s.name)
def test_resize_per_component_equals_resize_images_to_limits_fit(gpu, ip, s, kind):
    """pipeline.resize_per_component states the 'fit' rule a second time (one component, every image local): the same bytes,
    for numpy inputs and for resident tensors."""
    import torch

    pl = import_module(gpu.__name__ + ".pipeline")
    imgs = list(ic.limit_images(s.name))
    want = ip.resizeImagesToLimits(imgs, s.limits[0], s.limits[1], "fit")
    local = {k: (torch.from_numpy(im.copy()).cuda() if kind == "cuda" else im) for k, im in enumerate(imgs)}
    inp = {"heightLimit": s.limits[0], "widthLimit": s.limits[1]}
    got = pl.resize_per_component(inp, local, np.zeros(len(imgs), np.int64), [im.shape[:2] for im in imgs])
    assert sorted(got) == list(range(len(imgs)))
    for k, w_ in enumerate(want):
        g = got[k]
        if kind == "cuda":
            assert g.is_cuda
            g = g.cpu().numpy()
        assert same_bits(g, w_), k
    if s.name.startswith("a-"):
        assert all(got[k] is local[k] for k in local)
