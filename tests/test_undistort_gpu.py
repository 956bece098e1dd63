"""Lens distortion on the device against the NumPy mirror (tests/undistort_mirror.py), with no tolerance: undistortImage's bytes,
undistortPoints' bits, the 'valid' view's integers, and the prologue of pipeline.stitch.

The cases (undistort_mirror.CASES) are the smallest at which the image kernel takes each of its paths: 61 x 83 has 5063 pixels (not a
multiple of the four pixels whose bytes a quad of lanes packs into dwords, so the last quad stores bytes; more than one 256-pixel
workgroup), the 'small' valid view is larger than its input with an origin below 1, 70 x 131 in MATLAB layout has a width that is no
multiple of 4 or 64, and a 1030-pixel row is longer than one workgroup's span, so quads straddle row ends at every alignment."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import fast_cases as fc
import undistort_mirror as um

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ip(gpu):
    return import_module(gpu.__name__ + ".imageProcessing")


def record(ip, L):
    return ip.cameraIntrinsics((L["fx"], L["fy"], L["cx"], L["cy"]), (L["k1"], L["k2"], L["k3"]), (L["p1"], L["p2"]))


def picture(name, channels):
    h, w, L = um.case(name)
    img = fc.noise_rects(sum(map(ord, name)), h, w, channels)
    return img, L


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


# ---- undistortImage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,view,channels,fill", [("barrel", "same", 1, 0), ("pincushion", "same", 3, 7), ("small", "valid", 3, 0),
                                                     ("long-row", "same", 1, 0)])
def test_image_equals_the_mirror_byte_for_byte(ip, name, view, channels, fill):
    img, L = picture(name, channels)
    want, origin = um.undistort_image(img, L, view, fill)
    got, got_origin = ip.undistortImage(img, record(ip, L), view, fill)
    assert got_origin == origin and got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want)
    if name == "pincushion":  # the fill path is exercised, and a fill byte that no neighbour would produce by accident is there
        _, _, valid = um.sample_map(L, img.shape[0], img.shape[1], 1, 1, *img.shape[:2])
        assert 0.89 < valid.mean() < 0.91 and (got[~valid] == 7).all()
    if name == "small":
        assert origin == (-1, 0) and got.shape == (49, 52, 3)


def test_matlab_layout_through_the_raw_entry(gpu):
    """anisotropic, 'valid', planar column-major in and out (what the MATLAB gateway's arrays are)."""
    img, L = picture("anisotropic", 3)
    h, w = img.shape[:2]
    x0, y0, oh, ow = um.valid_view(L, h, w)
    want, _ = um.undistort_image(img, L, "valid")
    planar = np.ascontiguousarray(img.transpose(2, 1, 0))  # [c][column][row]
    out = np.zeros((3, ow, oh), np.uint8)
    lens = gpu._capi.aps_lens(**L)
    gpu._capi.check(gpu.lib.aps_undistort_image_u8(planar.ctypes.data, h, w, 3, gpu._capi.APS_IMG_U8_MATLAB, C.byref(lens), oh, ow, x0, y0, 0,
                                                   out.ctypes.data))
    assert np.array_equal(out.transpose(2, 1, 0), want)


@pytest.mark.parametrize("channels", [1, 3])
def test_identity_lens_returns_the_input(ip, channels):
    import torch

    h, w, _ = um.case("barrel")
    img = fc.noise_rects(5, h, w, channels)
    L = ip.cameraIntrinsics((70.0, 70.0, 43.3, 30.3))
    J, origin = ip.undistortImage(img, L)
    assert origin == (1, 1) and np.array_equal(J, img)
    R, origin = ip.undistortImage(torch.from_numpy(img).cuda(), L)
    assert origin == (1, 1) and R.is_cuda and np.array_equal(host(R), img)


@pytest.mark.parametrize("name,view,channels", [("barrel", "same", 1), ("small", "valid", 3)])
def test_resident_input_gives_a_resident_output_with_the_host_bytes(ip, name, view, channels):
    import torch

    img, L = picture(name, channels)
    J, origin = ip.undistortImage(img, record(ip, L), view, 3)
    R, r_origin = ip.undistortImage(torch.from_numpy(img).cuda(), record(ip, L), view, 3)
    assert R.is_cuda and R.dtype == torch.uint8 and r_origin == origin
    assert np.array_equal(host(R), J) and np.array_equal(J, um.undistort_image(img, L, view, 3)[0])


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("where", ["host", "device", "device_unaligned"])
def test_output_padding_is_left_alone(gpu, channels, where):
    """The raw entry writes out_h * out_w * c bytes and nothing after them: 5063 pixels end inside a quad of lanes, and a device
    buffer that is not dword-aligned takes the byte stores throughout."""
    import torch

    img, L = picture("barrel", channels)
    if channels == 1:
        img = img.reshape(img.shape[0], img.shape[1])
    h, w = img.shape[:2]
    want, _ = um.undistort_image(img, L, "same")
    n, pad, lead = h * w * channels, 37, 1 if where == "device_unaligned" else 0
    buf = np.full(lead + n + pad, 0xA5, np.uint8)
    lens = gpu._capi.aps_lens(**L)
    if where == "host":
        src, dst = np.ascontiguousarray(img), buf
        p_src, p_dst = src.ctypes.data, dst.ctypes.data
    else:
        src, dst = torch.from_numpy(np.ascontiguousarray(img)).cuda(), torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        p_src, p_dst = src.data_ptr(), dst.data_ptr() + lead
    gpu._capi.check(gpu.lib.aps_undistort_image_u8(p_src, h, w, channels, gpu._capi.APS_IMG_U8_HWC, C.byref(lens), h, w, 1, 1, 0, p_dst))
    got = host(dst)
    assert np.array_equal(got[lead:lead + n], want.ravel())
    assert (got[:lead] == 0xA5).all() and (got[lead + n:] == 0xA5).all()


# ---- undistortPoints -------------------------------------------------------------------------------------------------------------
def points(n):
    h, w, _ = um.case("barrel")
    rng = np.random.default_rng(100 + n)
    return np.stack([rng.uniform(1, w, n), rng.uniform(1, h, n)], 1)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_points_equal_the_mirror_bit_for_bit(gpu, ip, n):
    import torch

    _, _, L = um.case("barrel")
    p = points(n)
    want = um.undistort_points(L, p)
    got = ip.undistortPoints(p, record(ip, L))
    assert got.shape == (n, 2) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    res = ip.undistortPoints(torch.from_numpy(p).cuda(), record(ip, L))
    assert res.is_cuda and tuple(res.shape) == (n, 2) and np.array_equal(host(res).view(np.uint64), want.view(np.uint64))
    # a leading dimension above n through the raw entry: the padding columns keep their prefill, host and device
    ld = n + 5
    src = np.full((2, ld), np.nan)
    src[:, :n] = p.T
    lens = gpu._capi.aps_lens(**L)
    for resident in (False, True):
        dst = np.full((2, ld), -123.25)
        if resident:
            s, d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
            torch.cuda.synchronize()
            gpu._capi.check(gpu.lib.aps_undistort_points(s.data_ptr(), n, ld, C.byref(lens), d.data_ptr()))
            dst = host(d)
        else:
            gpu._capi.check(gpu.lib.aps_undistort_points(src.ctypes.data, n, ld, C.byref(lens), dst.ctypes.data))
        assert np.array_equal(dst[:, :n].view(np.uint64), np.ascontiguousarray(want.T).view(np.uint64))
        assert (dst[:, n:] == -123.25).all()


@pytest.mark.parametrize("name", list(um.CASES))
def test_valid_view_equals_the_mirror(ip, name):
    h, w, L = um.case(name)
    assert ip.undistort_valid_view((h, w), record(ip, L)) == um.valid_view(L, h, w)
    assert ip.undistort_valid_view((h, w, 3), record(ip, L)) == um.valid_view(L, h, w)


# ---- the prologue of pipeline.stitch ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def distorted_scene():
    """The three views of fast_cases.scene() as a lens with k = (-0.2, 0.05) on each view's own K would have taken them: every
    distorted pixel samples the original bilinearly at undistortPoints of its centre (mirror arithmetic, CPU)."""
    views, cams = fc.scene()
    lenses = [um.lens(c["K"][0, 0], c["K"][1, 1], c["K"][0, 2], c["K"][1, 2], (-0.2, 0.05)) for c in cams]
    return [um.distort_image(v, L) for v, L in zip(views, lenses)], lenses, [np.array(c["K"], np.float64) for c in cams]


@pytest.fixture(scope="module")
def stitched(gpu, ip, distorted_scene):
    pl = import_module(gpu.__name__ + ".pipeline")
    distorted, lenses, Ks = distorted_scene
    inp = pl.default_input(cameraIntrinsics=[record(ip, L) for L in lenses], resizeImage=0)
    return pl, pl.stitch(inp, distorted, Ks=Ks, tile=(512, 512))


def test_stitch_undistorts_first(ip, distorted_scene, stitched):
    distorted, lenses, Ks = distorted_scene
    pl, (panos, info) = stitched
    assert len(panos) == 1 and info["n_components"] == 1 and sorted(info["components"][0]["members"]) == [0, 1, 2]
    assert len(info["undistort"]) == 3 and info["times"]["undistort"] > 0
    for k, (img, L) in enumerate(zip(distorted, lenses)):
        x0, y0, oh, ow = um.valid_view(L, img.shape[0], img.shape[1])
        rec = info["undistort"][k]
        assert tuple(rec["origin"]) == (x0, y0) and tuple(rec["size"]) == (oh, ow)
        assert np.array_equal(rec["K"], pl.shift_K(record(ip, L).K, (x0, y0)))
        got = host(info["images_processed"][k])
        assert got.shape == (oh, ow, 3)
        assert np.array_equal(got, ip.undistortImage(img, record(ip, L), "valid")[0])
        assert np.array_equal(got, um.undistort_image(img, L, "valid")[0])
        want_K = Ks[k].copy()
        want_K[0, 2] -= x0 - 1
        want_K[1, 2] -= y0 - 1
        assert np.array_equal(info["cameras"][k]["K"], want_K)
    assert Ks[0][0, 2] == fc.scene()[1][0]["K"][0, 2]  # the caller's Ks are not written
    pano = host(panos[0])
    assert pano.ndim == 3 and (pano.max(axis=2) > 0).mean() > 0.5


def test_stitch_without_the_key_does_not_enter_the_prologue(ip, distorted_scene, stitched, monkeypatch):
    """Two calls without the key on the distorted views: the first as it is, the second with the undistortion operators
    replaced by ones that raise.  Both return the same bytes, and nothing of the prologue shows in info."""
    distorted, _, Ks = distorted_scene
    pl, (_, with_key) = stitched
    inp = pl.default_input(resizeImage=0)
    panos_a, a = pl.stitch(inp, distorted, Ks=Ks, tile=(512, 512))

    def refuse(*args, **kw):
        raise AssertionError("the prologue was entered")

    monkeypatch.setattr(ip, "undistortImage", refuse)
    monkeypatch.setattr(pl, "undistort_prologue", refuse)
    panos_b, b = pl.stitch(inp, distorted, Ks=Ks, tile=(512, 512))
    assert len(panos_a) == len(panos_b) and all(np.array_equal(host(p), host(q)) for p, q in zip(panos_a, panos_b))
    for info in (a, b):
        assert "undistort" not in info and "undistort" not in info["times"]
        assert all(x is y for x, y in zip(info["images_processed"], distorted))
    assert a["n_features"] == b["n_features"] and np.array_equal(a["putative"], b["putative"])
    assert np.array_equal(a["result"]["numMatches"], b["result"]["numMatches"])
    assert set(a) == set(b) == set(with_key) - {"undistort"}
    # (reported in DESIGN.md; a property of the scene, not of the code: no assertion)
    print("summed RANSAC inliers: with cameraIntrinsics", int(with_key["result"]["numMatches"].sum()), "without",
          int(a["result"]["numMatches"].sum()), "; verified pairs", with_key["n_pairs_verified"], a["n_pairs_verified"])
