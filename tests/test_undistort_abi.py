"""CPU tests of lens distortion: the three C-ABI entries' declarations and argument checks (no device needed: every check
comes before any device work), the wrappers' refusals, the pipeline keys, and the NumPy mirror of the contract (DESIGN.md,
"Lens distortion contract") against the figures the contract was settled with."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

import undistort_mirror as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"aps_undistort_image_u8": 12, "aps_undistort_points": 5, "aps_undistort_valid_view": 7}


@pytest.fixture(scope="module")
def ip(aps):
    return import_module(aps.__name__ + ".imageProcessing")


# ---- the entries -----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported(aps):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aps.h")).read(), flags=re.S)
    so = C.CDLL(aps._capi.LIB_PATH)
    for name, nargs in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in aps._capi.EXPORTED_SYMBOLS and hasattr(so, name)
        assert len(getattr(aps.lib, name).argtypes) == nargs
    m = re.search(r"typedef struct aps_lens \{(.*?)\} aps_lens;", header, flags=re.S)
    assert m and [f.strip() for f in re.sub(r"\bdouble\b|;", "", m.group(1)).split(",")] == list(um.FIELDS)
    lens = aps._capi.aps_lens
    assert [f for f, _ in lens._fields_] == list(um.FIELDS) and all(t is C.c_double for _, t in lens._fields_)
    assert C.sizeof(lens) == 72


def _lens(aps, **over):
    return aps._capi.aps_lens(**dict(um.case("barrel")[2], **over))


def _image_call(aps, img=True, out=True, h=6, w=7, c=3, layout=0, lens=True, oh=6, ow=7, x0=1, y0=1, fill=0, **over):
    src, dst = np.zeros(h * w * 3 if h > 0 and w > 0 else 1, np.uint8), np.full(max(oh * ow * 3, 1), 9, np.uint8)
    L = _lens(aps, **over)
    st = aps.lib.aps_undistort_image_u8(src.ctypes.data if img else None, h, w, c, layout, C.byref(L) if lens else None, oh, ow, x0, y0,
                                        fill, dst.ctypes.data if out else None)
    assert (dst == 9).all()  # a refused call writes nothing
    return st


BAD_LENS = [dict(fx=0.0), dict(fy=-1.0), dict(fx=np.nan), dict(fy=np.inf), dict(cx=np.nan), dict(cy=np.inf), dict(k1=np.nan),
            dict(k2=-np.inf), dict(k3=np.nan), dict(p1=np.inf), dict(p2=np.nan)]


def test_image_entry_refuses_bad_arguments_without_a_device(aps):
    k = aps._capi
    for bad in [dict(img=False), dict(out=False), dict(lens=False), dict(fill=-1), dict(fill=256)] + BAD_LENS:
        assert _image_call(aps, **bad) == k.APS_E_ARG, bad
        assert aps.lib.aps_last_error()
    for bad in (dict(c=0), dict(c=2), dict(c=4), dict(h=0), dict(w=-2), dict(oh=0), dict(ow=-1)):
        assert _image_call(aps, **bad) == k.APS_E_DIM, bad
    for bad in (dict(layout=2), dict(layout=-1)):
        assert _image_call(aps, **bad) == k.APS_E_TYPE, bad


def test_points_entry_refuses_bad_arguments_without_a_device(aps):
    k = aps._capi
    pts, out = np.ones(12), np.full(12, 9.0)
    call = lambda p, n, ld, L, o: aps.lib.aps_undistort_points(p, n, ld, C.byref(L) if L is not None else None, o)  # noqa: E731
    good = _lens(aps)
    assert call(None, 3, 6, good, out.ctypes.data) == k.APS_E_ARG
    assert call(pts.ctypes.data, 3, 6, good, None) == k.APS_E_ARG
    assert call(pts.ctypes.data, 3, 6, None, out.ctypes.data) == k.APS_E_ARG
    assert call(pts.ctypes.data, -1, 6, good, out.ctypes.data) == k.APS_E_DIM
    assert call(pts.ctypes.data, 4, 3, good, out.ctypes.data) == k.APS_E_DIM
    for bad in BAD_LENS:
        assert call(pts.ctypes.data, 3, 6, _lens(aps, **bad), out.ctypes.data) == k.APS_E_ARG, bad
    assert call(None, 0, 0, good, None) == k.APS_OK  # n = 0 is a no-op, with or without a device
    assert (out == 9.0).all()


def test_valid_view_entry_refuses_bad_arguments_without_a_device(aps):
    k = aps._capi
    v = [C.c_int(-7) for _ in range(4)]
    refs = [C.byref(x) for x in v]
    good = _lens(aps)
    assert aps.lib.aps_undistort_valid_view(6, 7, None, *refs) == k.APS_E_ARG
    for q in range(4):
        assert aps.lib.aps_undistort_valid_view(6, 7, C.byref(good), *[None if t == q else r for t, r in enumerate(refs)]) == k.APS_E_ARG
    for (h, w) in ((0, 7), (6, 0), (-1, 7)):
        assert aps.lib.aps_undistort_valid_view(h, w, C.byref(good), *refs) == k.APS_E_DIM
    for bad in BAD_LENS:
        L = _lens(aps, **bad)
        assert aps.lib.aps_undistort_valid_view(6, 7, C.byref(L), *refs) == k.APS_E_ARG, bad
    assert [x.value for x in v] == [-7] * 4


def test_valid_calls_need_a_device(aps, ip):
    """No CPU fallback: without a device a valid call is APS_E_DEVICE; with one it succeeds."""
    L = ip.cameraIntrinsics((70, 70, 43.3, 30.3), (-0.25, 0.08))
    for call in (lambda: ip.undistortImage(np.zeros((61, 83), np.uint8), L), lambda: ip.undistortPoints(np.ones((3, 2)), L),
                 lambda: ip.undistort_valid_view((61, 83), L)):
        if aps.lib.aps_device_count() > 0:
            call()
        else:
            with pytest.raises(aps.ApsError) as e:
                call()
            assert e.value.code == aps._capi.APS_E_DEVICE


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------
def test_camera_intrinsics_record(ip):
    K = np.array([[70.0, 0, 43.3], [0, 71.0, 30.3], [0, 0, 1]])
    a = ip.cameraIntrinsics(K, (-0.25, 0.08), (1e-3, -5e-4))
    b = ip.cameraIntrinsics((70.0, 71.0, 43.3, 30.3), RadialDistortion=(-0.25, 0.08, 0.0), TangentialDistortion=(1e-3, -5e-4))
    for L in (a, b):
        lens = L.lens()
        assert [getattr(lens, f) for f in um.FIELDS] == [70.0, 71.0, 43.3, 30.3, -0.25, 0.08, 0.0, 1e-3, -5e-4]
        assert np.array_equal(L.K, K)
    plain = ip.cameraIntrinsics(K).lens()
    assert [getattr(plain, f) for f in um.FIELDS[4:]] == [0.0] * 5
    skew = K.copy()
    skew[0, 1] = 0.5
    with pytest.raises(ValueError):
        ip.cameraIntrinsics(skew)
    for k in ((), (0.1,), (0.1, 0.2, 0.3, 0.4)):
        with pytest.raises(ValueError):
            ip.cameraIntrinsics(K, RadialDistortion=k)
    for p in ((), (0.1,), (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError):
            ip.cameraIntrinsics(K, TangentialDistortion=p)
    with pytest.raises(ValueError):
        ip.cameraIntrinsics(np.eye(2))


def test_wrappers_refuse_before_any_device_work(ip):
    L = ip.cameraIntrinsics((70, 70, 43.3, 30.3), (-0.25, 0.08))
    img = np.zeros((6, 7, 3), np.uint8)
    for view in ("full", "", "Valid ", None):
        with pytest.raises(ValueError):
            ip.undistortImage(img, L, OutputView=view)
    with pytest.raises(TypeError):
        ip.undistortImage(img.astype(np.float32), L)
    for bad in (np.zeros((6, 7, 2), np.uint8), np.zeros((6, 7, 3, 1), np.uint8), np.zeros(6, np.uint8)):
        with pytest.raises(ValueError):
            ip.undistortImage(bad, L)
    for fill in (-1, 256, 1.5, (1, 2, 3)):
        with pytest.raises(ValueError):
            ip.undistortImage(img, L, FillValues=fill)
    for pts in (np.ones((3, 3)), np.ones(4), np.ones((2, 2, 2))):
        with pytest.raises(ValueError):
            ip.undistortPoints(pts, L)
    assert ip.undistortPoints(np.zeros((0, 2)), L).shape == (0, 2)  # n = 0 needs no device


def test_pipeline_keys(aps, ip):
    pl = import_module(aps.__name__ + ".pipeline")
    par = import_module(aps.__name__ + ".parallel")
    assert "cameraIntrinsics" not in pl.DEFAULT_INPUT and "undistortOutputView" not in pl.DEFAULT_INPUT
    L = ip.cameraIntrinsics((70, 70, 43.3, 30.3), (-0.25, 0.08))
    with pytest.raises(NotImplementedError):
        par.stitch_distributed({"cameraIntrinsics": L}, {}, 0, None)
    with pytest.raises(ValueError):  # one lens, or one per image
        pl.undistort_prologue({"cameraIntrinsics": [L]}, [np.zeros((6, 7, 3), np.uint8)] * 2, None, None)
    K = np.array([[70.0, 0, 43.3], [0, 70.0, 30.3], [0, 0, 1]])
    assert np.array_equal(pl.shift_K(K, (-3, 0)), [[70.0, 0, 47.3], [0, 70.0, 31.3], [0, 0, 1]])
    assert np.array_equal(pl.shift_K(K, (1, 1)), K) and K[0, 2] == 43.3


# ---- the mirror ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bound_seen", [("barrel", 6e-13), ("pincushion", 2e-14)])
def test_mirror_round_trip_closes(name, bound_seen):
    """distort(undistort(p)) over all pixel centres: within 1e-6 px (the contract was settled at 6e-13 / 2e-14 px)."""
    h, w, L = um.case(name)
    u, v = np.meshgrid(np.arange(1, w + 1, dtype=np.float64), np.arange(1, h + 1, dtype=np.float64))
    q = um.undistort_points(L, np.stack([u.ravel(), v.ravel()], 1))
    ud, vd = um.distort(L, q[:, 0], q[:, 1])
    err = float(np.hypot(ud - u.ravel(), vd - v.ravel()).max())
    print(name, "round trip", err, "px; settled at", bound_seen)
    assert err <= 1e-6


@pytest.mark.parametrize("name,want", [("barrel", (-3, 0, 63, 90)), ("pincushion", (4, 3, 57, 77)), ("small", (-1, 0, 49, 52))])
def test_mirror_valid_views(name, want):
    h, w, L = um.case(name)
    assert um.valid_view(L, h, w) == want


@pytest.mark.parametrize("name", list(um.CASES))
def test_mirror_valid_views_have_no_invalid_sample(name):
    h, w, L = um.case(name)
    _, _, valid = um.sample_map(L, h, w, *um.valid_view(L, h, w))
    assert valid.all()


def test_mirror_same_view_of_the_pincushion_lens_exercises_the_fill():
    h, w, L = um.case("pincushion")
    _, _, valid = um.sample_map(L, h, w, 1, 1, h, w)
    assert abs(valid.mean() - 0.901) < 0.002
    img = np.full((h, w, 3), 200, np.uint8)
    J, origin = um.undistort_image(img, L, "same", 7)
    assert origin == (1, 1) and (J[~valid] == 7).all() and (J[valid] == 200).all()


def test_mirror_identity_and_rounding():
    h, w, _ = um.case("small")
    L = um.lens(40.0, 40.0, 26.3, 23.3)
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    J, origin = um.undistort_image(img, L, "same")
    assert origin == (1, 1) and np.array_equal(J, img)
    s = np.array([0.49999999999999994, 0.5, 1.5, 2.5, 254.5, 3.4999999999999996])
    assert um._round_half_away(s).tolist() == [0.0, 1.0, 2.0, 3.0, 255.0, 3.0]
