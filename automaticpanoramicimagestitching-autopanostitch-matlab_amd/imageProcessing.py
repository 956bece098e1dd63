"""Host-side mirror of PP/imageProcessing/imageWarp.m and its imref2d helpers."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib, ptr


def imref2dScratch(imageSize, xWorldLimits=None, yWorldLimits=None):
    """imref2dScratch.m:50-76 — a struct clone of imref2d."""
    h, w = int(imageSize[0]), int(imageSize[1])
    xl = (0.5, w + 0.5) if xWorldLimits is None else tuple(map(float, xWorldLimits))
    yl = (0.5, h + 0.5) if yWorldLimits is None else tuple(map(float, yWorldLimits))
    return {"ImageSize": (h, w), "XWorldLimits": xl, "YWorldLimits": yl,
            "PixelExtentInWorldX": (xl[1] - xl[0]) / w, "PixelExtentInWorldY": (yl[1] - yl[0]) / h}


def transformPointsForwardScratch(tform, xy):
    """transformPointsForwardScratch.m:57-77: [x y 1] -> H*[x;y;1], |w| < 1e-12 -> NaN."""
    H = np.asarray(tform, np.float64)
    xy = np.asarray(xy, np.float64)
    q = np.c_[xy, np.ones(len(xy))] @ H.T
    w = q[:, 2].copy()
    w[np.abs(w) < 1e-12] = np.nan
    return q[:, :2] / w[:, None]


def outputLimitsScratch(tform, xLimitsIn, yLimitsIn):
    """outputLimitsScratch.m:71-111: bounding box of the transformed input rectangle (corners + edge midpoints)."""
    x0, x1 = map(float, xLimitsIn)
    y0, y1 = map(float, yLimitsIn)
    xm, ym = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    pts = np.array([[x0, y0], [xm, y0], [x1, y0], [x0, ym], [xm, ym], [x1, ym], [x0, y1], [xm, y1], [x1, y1]])
    out = transformPointsForwardScratch(tform, pts)
    return (np.nanmin(out[:, 0]), np.nanmax(out[:, 0])), (np.nanmin(out[:, 1]), np.nanmax(out[:, 1]))


def imageWarp(image, tform, outputView, method="bilinear", fillValue=0):
    """warped = imageWarp(image, tform, outputView, options) (imageWarp.m:1-273) on the device: options.method
    'nearest' (:109-123), 'bilinear' (:125-168, the default) or 'bicubic' (:170-264); uint8 images stay uint8, every
    other class is interpolated as single."""
    m = {"nearest": _capi.APS_WARP_NEAREST, "bilinear": _capi.APS_WARP_BILINEAR, "bicubic": _capi.APS_WARP_BICUBIC}.get(str(method).lower())
    if m is None:
        raise ValueError(f"unknown interpolation method '{method}'")  # (the reference's switch silently leaves the fill value)
    img = np.asarray(image)
    squeeze = img.ndim == 2
    if squeeze:
        img = img[..., None]
    H = np.ascontiguousarray(np.asarray(tform, np.float64).T)  # column-major 3x3
    oh, ow = outputView["ImageSize"]
    x0, y0 = outputView["XWorldLimits"][0], outputView["YWorldLimits"][0]
    sx, sy = outputView["PixelExtentInWorldX"], outputView["PixelExtentInWorldY"]
    c = img.shape[2]
    if img.dtype == np.uint8:
        src = np.ascontiguousarray(img)
        out = np.zeros((oh, ow, c), np.uint8)
        check(lib.aps_image_warp_u8(ptr(src), img.shape[0], img.shape[1], c, ptr(H), oh, ow, x0, y0, sx, sy,
                                    int(fillValue), m, ptr(out)))
    else:
        src = np.ascontiguousarray(img, np.float32)
        out = np.zeros((oh, ow, c), np.float32)
        check(lib.aps_image_warp_f32(ptr(src), img.shape[0], img.shape[1], c, ptr(H), oh, ow, x0, y0, sx, sy,
                                     float(fillValue), m, ptr(out)))
        out = out.astype(img.dtype) if img.dtype != np.float32 else out
    return out[..., 0] if squeeze else out


def imresize(I, scale_or_size, method="bicubic"):
    """J = imresize(I, s, method) / imresize(I, [oh ow], method) for uint8 images on the device (toolbox semantics
    as restated in oracle/render_oracle.c).  The scalar form gives ceil(s * size) with scale s in both dimensions.
    A torch CUDA tensor stays resident: the result is a CUDA tensor and nothing visits the host."""
    import math

    dev = _capi.is_torch(I) and I.is_cuda
    if dev:
        import torch

        a = I.contiguous()
        if a.dtype != torch.uint8:
            raise TypeError("uint8 images only")
        sq = a.dim() == 2
        if sq:
            a = a[..., None]
        h, w, c = (int(v) for v in a.shape)
    else:
        a = np.ascontiguousarray(I)
        if a.dtype != np.uint8:
            raise TypeError("uint8 images only")
        sq = a.ndim == 2
        if sq:
            a = a[..., None]
        h, w, c = a.shape
    if np.isscalar(scale_or_size):
        s = float(scale_or_size)
        oh, ow, sr, sc = int(math.ceil(h * s)), int(math.ceil(w * s)), s, s
    else:
        oh, ow = int(scale_or_size[0]), int(scale_or_size[1])
        sr, sc = oh / h, ow / w
    m = {"bicubic": _capi.APS_RESIZE_BICUBIC, "bilinear": _capi.APS_RESIZE_BILINEAR}[str(method).lower()]
    if dev:
        out = torch.empty((oh, ow, c), dtype=torch.uint8, device=a.device)
        torch.cuda.current_stream().synchronize()  # the input came from torch's stream; the library runs on its own
    else:
        out = np.zeros((oh, ow, c), np.uint8)
    check(lib.aps_imresize_u8(ptr(a), h, w, c, _capi.APS_IMG_U8_HWC, oh, ow, sr, sc, m, ptr(out)))
    return out[..., 0] if sq else out


def _center_crop(J, Ht, Wt):
    h, w = J.shape[:2]
    r0, c0 = (h - Ht) // 2, (w - Wt) // 2
    return J[r0:r0 + Ht, c0:c0 + Wt]


def resizeImagesToLimits(imageFiles, heightLimit, widthLimit, mode="fit"):
    """imageFilesResized = resizeImagesToLimits(imageFiles, heightLimit, widthLimit, mode)
    (resizeImagesToLimits.m:1-160): 'fit' (isotropic shrink to the box, then all images to the common largest size),
    'pad' (fit, then replicate-pad to the box) or 'fillcrop' (cover, then centre crop).  Resizing runs on the device.
    When no image exceeds the limits and all have one size, the input comes back untouched in every mode (:29-42)."""
    mode = str(mode).lower()
    if mode not in ("fit", "pad", "fillcrop"):
        raise ValueError(f"unknown mode '{mode}'")
    if not isinstance(imageFiles, (list, tuple)) or len(imageFiles) == 0:
        raise ValueError("imageFiles must be a nonempty cell array of images.")  # :21-23
    if not (np.isscalar(heightLimit) and np.isscalar(widthLimit) and heightLimit > 0 and widthLimit > 0):
        raise ValueError("heightLimit and widthLimit must be positive scalars.")  # :25-27
    initial = [tuple(a.shape[:2]) if a.size else (0, 0) for a in map(np.asarray, imageFiles)]  # size([]) is [0 0]
    if not any(h > heightLimit or w > widthLimit for (h, w) in initial) and len(set(initial)) == 1:
        return list(imageFiles)  # all the same size, nothing to do
    stage1 = []
    for I in imageFiles:
        I = np.asarray(I)
        if I.size == 0:
            stage1.append(I)
            continue
        h, w = I.shape[:2]
        if mode in ("fit", "pad"):
            s = min(heightLimit / h, widthLimit / w)
            if not np.isfinite(s) or s <= 0:
                s = 1
            J = imresize(I, s, "bicubic") if s < 1 else I
            if mode == "pad":
                if J.shape[0] > heightLimit or J.shape[1] > widthLimit:
                    J = _center_crop(J, min(heightLimit, J.shape[0]), min(widthLimit, J.shape[1]))
                ph, pw = heightLimit - J.shape[0], widthLimit - J.shape[1]
                pad = ((ph // 2, ph - ph // 2), (pw // 2, pw - pw // 2)) + (((0, 0),) if J.ndim == 3 else ())
                J = np.pad(J, pad, mode="edge")
        else:
            s = max(heightLimit / h, widthLimit / w)
            if not np.isfinite(s) or s <= 0:
                s = 1
            J = _center_crop(imresize(I, s, "bicubic"), heightLimit, widthLimit)
        stage1.append(J)
    if mode != "fit":
        return stage1
    sizes = {(J.shape[0], J.shape[1]) for J in stage1 if J.size}
    if len(sizes) <= 1:
        return stage1
    Hmax, Wmax = max(s[0] for s in sizes), max(s[1] for s in sizes)
    return [J if J.size == 0 else imresize(J, (Hmax, Wmax), "bicubic") for J in stage1]


def cropRectangle(stitchedImage, canvasColor="black", blackRange=0, whiteRange=250):
    """The crop indices of panoramaCropper.m:73-157 on the device: (offsetx, offsety, cropW, cropH) 1-based as in the
    reference, and whether rows offsety..offsety+cropH / columns offsetx..offsetx+cropW lie inside the image."""
    white = str(canvasColor).lower() == "white"
    if _capi.is_torch(stitchedImage):
        img = stitchedImage.contiguous()
        if str(img.dtype) != "torch.uint8" or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError("stitchedImage must be M-by-N-by-3 uint8")
        h, w = int(img.shape[0]), int(img.shape[1])
    else:
        img = np.ascontiguousarray(stitchedImage)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("stitchedImage must be M-by-N-by-3 uint8")
        h, w = img.shape[:2]
    rect = np.zeros(4, np.int32)
    valid = np.zeros(1, np.int32)
    check(lib.aps_crop_rect(ptr(img), h, w, _capi.APS_IMG_U8_HWC, int(white), float(whiteRange if white else blackRange),
                            ptr(rect), ptr(valid)))
    return tuple(int(v) for v in rect), bool(valid[0])


def panoramaCropper(input, stitchedImage):
    """croppedImage = panoramaCropper(input, stitchedImage) (panoramaCropper.m:1-178): same field checks, same crop
    (offsety:offsety+cropH, offsetx:offsetx+cropW, 1-based inclusive), the input unchanged with a warning when the
    rectangle leaves the image ("Image has background holes")."""
    import warnings

    req = ["canvasColor", "blackRange", "whiteRange", "showCropBoundingBox", "displayPanoramas"]
    missing = [f for f in req if f not in input]
    if missing:
        raise ValueError("panoramaCropper:MissingField: Missing required input fields: " + ", ".join(missing))
    color = str(input["canvasColor"]).lower()
    if color not in ("black", "white"):
        raise ValueError('panoramaCropper:InvalidCanvasColor: input.canvasColor must be "black" or "white".')
    for f in ("blackRange", "whiteRange"):
        v = input[f]
        if not (np.isscalar(v) and np.isfinite(v) and 0 <= v <= 255):
            raise ValueError(f"panoramaCropper:Invalid{f[0].upper() + f[1:]}: input.{f} must be a numeric scalar in [0,255].")
    for f in ("showCropBoundingBox", "displayPanoramas"):
        if not isinstance(input[f], (bool, np.bool_)):
            raise ValueError(f"panoramaCropper:InvalidFlag: input.{f} must be a logical scalar.")
    (ox, oy, cw, ch), ok = cropRectangle(stitchedImage, color, input["blackRange"], input["whiteRange"])
    if not ok:
        warnings.warn("Cannot crop the image. Image has background holes.")
        return stitchedImage
    return stitchedImage[oy - 1:oy + ch, ox - 1:ox + cw]


PANO_PROJECTIONS = ("planar", "cylindrical", "spherical", "equirectangular", "stereographic", "miller", "fisheye", "panini")


def panorama_file_names(input, panoStore, myImg, datasetName):
    """The file names cropNsavePanorama.m:136-208 writes, in its order: for every panorama ii (1-based) and every projection
    field present and non-empty: '<proj>_<transformationType>_<myImg>_<ii>_<dataset>.png'; then, with input.cropPanorama,
    '<proj>_cropped_...'; then, with showPanoramaImgsNums and showCropBoundingBox, '<proj>_annotated_...'.
    Returns [(file name, panorama index (0-based), projection, slot)], slot 0 = base, 1 = annotated, 2 = cropped
    (the cell slots {1}, {2}, {3} of the reference)."""
    tt = str(input["transformationType"])
    name = str(datasetName[myImg - 1])
    out = []
    for ii, rec in enumerate(panoStore):
        have = [p for p in PANO_PROJECTIONS if rec.get(p)]
        for tag, slot, on in (("", 0, True), ("_cropped", 2, int(input.get("cropPanorama", 0)) == 1),
                              ("_annotated", 1, bool(input.get("showPanoramaImgsNums")) and bool(input.get("showCropBoundingBox")))):
            if on:
                out += [(f"{p}{tag}_{tt}_{myImg}_{ii + 1}_{name}.png", ii, p, slot) for p in have]
    return out


def cropNsavePanorama(input, panoStore, myImg, datasetName):
    """panoStore = cropNsavePanorama(input, panoStore, myImg, datasetName) (cropNsavePanorama.m:1-215): panoStore is a list of
    dicts, one per panorama, with a projection name -> [base RGB, annotated RGB or None, cropped RGB] (the reference's 1 x M
    struct array of cells).  With input.cropPanorama every present projection's base panorama goes through panoramaCropper
    (crop rectangle on the device) into slot 3; with input.imageWrite the PNG files are written to input.imageSaveFolder under
    the reference's names (host I/O: PIL).  Same argument checks and messages as :51-66.  myImg is 1-based."""
    import os

    if not (isinstance(myImg, (int, np.integer)) and 1 <= myImg <= len(datasetName)):
        raise ValueError(f"cropNsavePanorama:InvalidDatasetIndex: myImg ({myImg}) must index into datasetName (numel={len(datasetName)}).")
    if not isinstance(datasetName[myImg - 1], str):
        raise ValueError("cropNsavePanorama:InvalidDatasetNameType: datasetName{myImg} must be char or string.")
    write = bool(input.get("imageWrite"))
    if write and "transformationType" not in input:
        raise ValueError("cropNsavePanorama:MissingTransformationType: input.transformationType is required when input.imageWrite is true.")
    if write and not os.path.isdir(input["imageSaveFolder"]):
        os.makedirs(input["imageSaveFolder"])
    if int(input.get("cropPanorama", 0)) == 1:
        for rec in panoStore:
            for p in PANO_PROJECTIONS:
                if rec.get(p):
                    cell = list(rec[p]) + [None] * (3 - len(rec[p]))
                    cell[2] = panoramaCropper(input, cell[0])
                    rec[p] = cell
    if write:
        from PIL import Image

        for fname, ii, p, slot in panorama_file_names(input, panoStore, myImg, datasetName):
            img = panoStore[ii][p][slot]
            if _capi.is_torch(img):
                img = img.cpu().numpy()
            Image.fromarray(np.ascontiguousarray(img)).save(os.path.join(input["imageSaveFolder"], fname))
    return panoStore


# ---- loadImages.m:57-68,103-215: the two per-image steps in front of the resize ----------------------------------------
def applyOrientation(img, orientation):
    """The EXIF orientation switch of imreadAutoRotate (loadImages.m:194-212) on an H x W [x C] array: numpy, or a torch
    tensor (host or resident: pure data movement, the result stays where the input is).  rot90(A, k) turns
    counter-clockwise like MATLAB's; unknown codes leave the image unchanged, like the reference's switch."""
    is_t = _capi.is_torch(img)
    if is_t:
        import torch

        flip = lambda a, ax: torch.flip(a, (ax,))  # noqa: E731
        rot = lambda a, k: torch.rot90(a, k, (0, 1))  # noqa: E731
    else:
        flip = lambda a, ax: np.flip(a, ax)  # noqa: E731
        rot = lambda a, k: np.rot90(a, k, (0, 1))  # noqa: E731
    o = int(orientation) if orientation is not None else 1
    if o == 2:
        out = flip(img, 1)
    elif o == 3:
        out = rot(img, 2)
    elif o == 4:
        out = flip(img, 0)
    elif o == 5:
        out = rot(flip(img, 1), -1)
    elif o == 6:
        out = rot(img, -1)
    elif o == 7:
        out = rot(flip(img, 1), 1)
    elif o == 8:
        out = rot(img, 1)
    else:
        return img
    return out.contiguous() if is_t else np.ascontiguousarray(out)


def convertToRGB(img):
    """loadImages.m:103-125: a single-channel image replicated to H x W x 3, a three-channel one unchanged."""
    if img.ndim == 2:
        img = img[:, :, None]
    if img.shape[2] == 1:
        return img.repeat(1, 1, 3).contiguous() if _capi.is_torch(img) else np.ascontiguousarray(np.repeat(img, 3, axis=2))
    return img


def imreadAutoRotate(filename, device=None):
    """img = imreadAutoRotate(filename) (loadImages.m:127-215): imread + the EXIF orientation (tag 274) undone.  Returns a
    uint8 numpy array, or with device='cuda' a resident torch tensor (the turn is then done on the device)."""
    from PIL import Image

    with Image.open(filename) as im_:
        orientation = None
        try:
            orientation = im_.getexif().get(274)
        except Exception:  # noqa: BLE001 - like the reference's try/catch around imfinfo: unreadable metadata = no turn
            orientation = None
        if im_.mode not in ("L", "RGB", "RGBA"):
            im_ = im_.convert("RGB")
        arr = np.asarray(im_)
    if device is not None:
        import torch

        arr = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
    return applyOrientation(arr, orientation)


# ---- drawing on images: marks (segments and rings) and the montage of a pair ("Mark contract") ---------------
def drawing_buffers(image, what="image"):
    """(src, dst, H, W) for an entry that draws src into dst: image is uint8 H x W x 3 (H x W and H x W x 1 are replicated), a
    numpy array or a torch tensor; dst is of the same kind, resident when image is, and image itself is never written.  When
    src is a copy made here (a replicated channel, a non-contiguous view made contiguous) it is drawn on in place (dst is
    src): one copy of the canvas either way."""
    is_t = _capi.is_torch(image)
    if not is_t:
        image = np.asarray(image)
    if image.ndim == 2:
        image = image[:, :, None]
    if str(image.dtype).split(".")[-1] != "uint8" or image.ndim != 3 or int(image.shape[2]) not in (1, 3):
        raise ValueError(f"{what} must be uint8 H x W, H x W x 1 or H x W x 3, got {image.dtype} {tuple(image.shape)}")
    if is_t and image.is_cuda:
        check(lib.aps_synchronize())  # the image may still be in flight on the library's stream of this thread
    if int(image.shape[2]) == 1:
        src, own = (image.expand(-1, -1, 3).contiguous() if is_t else np.repeat(image, 3, axis=2)), True
    elif is_t:
        src, own = (image, False) if image.is_contiguous() else (image.contiguous(), True)
    else:
        src, own = (image, False) if image.flags.c_contiguous else (np.ascontiguousarray(image), True)
    if own:
        dst = src
    elif is_t:
        import torch

        dst = torch.empty_like(src)
    else:
        dst = np.empty_like(src)
    if is_t and src.is_cuda:
        import torch

        torch.cuda.current_stream().synchronize()  # torch produced them; the library draws on its own stream
    return src, dst, int(src.shape[0]), int(src.shape[1])


def _marks(kind, a, b, rgb, lineWidth):
    a = np.asarray(a, np.float64).reshape(-1, 2)
    m = np.zeros(len(a), _capi.MARK_DTYPE)
    m["x0"], m["y0"] = a[:, 0], a[:, 1]
    m["x1"], m["y1"] = b
    m["kind"] = kind
    m["line_width"] = np.asarray(lineWidth, np.int64)  # a scalar, or one per mark
    m["rgb"] = np.asarray(rgb, np.uint8).reshape(-1, 3)  # one colour, or one per mark
    return m


def mark_segments(p0, p1, rgb, lineWidth=1):
    """The marks (an array of _capi.MARK_DTYPE = aps_mark) of the segments p0[k] -> p1[k]: [n, 2] (x, y), 1-based.  rgb: one
    uint8 triple or [n, 3]; lineWidth: one value or [n], each in 1..64.  Concatenating mark arrays gives the drawing order."""
    p1 = np.asarray(p1, np.float64).reshape(-1, 2)
    if len(p1) != len(np.asarray(p0, np.float64).reshape(-1, 2)):
        raise ValueError("p0 and p1 must have one row per segment")
    return _marks(_capi.APS_MARK_SEGMENT, p0, (p1[:, 0], p1[:, 1]), rgb, lineWidth)


def mark_rings(centres, radii, rgb, lineWidth=1):
    """The marks of rings around centres[k] ([n, 2] (x, y), 1-based) of radius radii[k] pixels (one value or [n]; radius 0 is a
    disc of diameter lineWidth; rings above 4096 px are skipped when drawn).  rgb and lineWidth as for mark_segments."""
    return _marks(_capi.APS_MARK_RING, centres, (np.asarray(radii, np.float64), 0.0), rgb, lineWidth)


def draw_marks(image, marks):
    """(drawn_image, marks_drawn): the marks drawn on a copy of image on the device (aps_draw_marks; the raster rule is
    DESIGN.md's "Mark contract"), in ascending index, the highest index on top.  image as drawing_buffers takes it; the result
    is a new H x W x 3 array of the same kind, resident when image is.  marks: an array of _capi.MARK_DTYPE (mark_segments,
    mark_rings, np.concatenate of them).  marks_drawn counts the valid marks (finite, |coordinate| <= 2^20, radius in 0..4096)."""
    marks = np.ascontiguousarray(marks)
    if marks.dtype != _capi.MARK_DTYPE or marks.ndim != 1:
        raise ValueError("marks must be a one-dimensional array of _capi.MARK_DTYPE (mark_segments / mark_rings)")
    src, dst, H, W = drawing_buffers(image)
    drawn = C.c_int64(0)
    check(lib.aps_draw_marks(ptr(src), H, W, ptr(marks), len(marks), ptr(dst), C.byref(drawn)))
    return dst, int(drawn.value)


def montage_pair(I1, I2):
    """The 'montage' of showMatchedFeatures: I1 and I2 side by side on a max(h1, h2) x (w1 + w2) x 3 canvas, 0 elsewhere
    (aps_montage_pair).  I1, I2: uint8 H x W, H x W x 1 or H x W x 3, numpy arrays or torch tensors; the result is a CUDA tensor
    when either is one, a host tensor when either is a torch tensor, a numpy array otherwise."""
    imgs = []
    for k, im in enumerate((I1, I2)):
        is_t = _capi.is_torch(im)
        if not is_t:
            im = np.asarray(im)
        if str(im.dtype).split(".")[-1] != "uint8" or im.ndim not in (2, 3) or (im.ndim == 3 and int(im.shape[2]) not in (1, 3)):
            raise ValueError(f"I{k + 1} must be uint8 H x W, H x W x 1 or H x W x 3, got {im.dtype} {tuple(im.shape)}")
        im = convertToRGB(im)
        imgs.append(im.contiguous() if is_t else np.ascontiguousarray(im))
    (h1, w1), (h2, w2) = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
    shape = (max(h1, h2), w1 + w2, 3)
    tens = [im for im in imgs if _capi.is_torch(im)]
    if tens:
        import torch

        cuda = [t for t in tens if t.is_cuda]
        if cuda:
            check(lib.aps_synchronize())
            torch.cuda.current_stream().synchronize()  # torch produced them; the library copies on its own stream
        dst = torch.empty(shape, dtype=torch.uint8, device=cuda[0].device if cuda else "cpu")
    else:
        dst = np.empty(shape, np.uint8)
    check(lib.aps_montage_pair(ptr(imgs[0]), h1, w1, ptr(imgs[1]), h2, w2, ptr(dst)))
    return dst


# ---- lens distortion: cameraIntrinsics, undistortImage, undistortPoints ("Lens distortion contract") -------------------
class cameraIntrinsics:
    """intrinsics = cameraIntrinsics(K | (fx, fy, cx, cy), RadialDistortion=(k1, k2[, k3]), TangentialDistortion=(p1, p2)): a lens
    without skew in the project's 1-based pixel frame (the frame of keypoints and of Ks).  K is 3 x 3 with K[0, 1] == 0."""

    def __init__(self, K, RadialDistortion=(0.0, 0.0), TangentialDistortion=(0.0, 0.0)):
        K = np.asarray(K, np.float64)
        if K.shape == (3, 3):
            if K[0, 1] != 0:
                raise ValueError("cameraIntrinsics: skew (K[0, 1] != 0) is not modelled")
            fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        elif K.shape == (4,):
            fx, fy, cx, cy = K
        else:
            raise ValueError("cameraIntrinsics: give a 3 x 3 K or (fx, fy, cx, cy)")
        k = tuple(float(v) for v in np.asarray(RadialDistortion, np.float64).ravel())
        p = tuple(float(v) for v in np.asarray(TangentialDistortion, np.float64).ravel())
        if len(k) not in (2, 3):
            raise ValueError("cameraIntrinsics: RadialDistortion has 2 or 3 coefficients")
        if len(p) != 2:
            raise ValueError("cameraIntrinsics: TangentialDistortion has 2 coefficients")
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.RadialDistortion, self.TangentialDistortion = k, p

    @property
    def K(self):
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])

    def lens(self):
        """The aps_lens of the C ABI (a two-term radial model has k3 = 0)."""
        k = self.RadialDistortion + (0.0,) * (3 - len(self.RadialDistortion))
        return _capi.aps_lens(self.fx, self.fy, self.cx, self.cy, *k, *self.TangentialDistortion)

    def __repr__(self):
        return (f"cameraIntrinsics(fx={self.fx}, fy={self.fy}, cx={self.cx}, cy={self.cy}, RadialDistortion={self.RadialDistortion}, "
                f"TangentialDistortion={self.TangentialDistortion})")


def undistort_valid_view(shape, intrinsics):
    """(x0, y0, out_h, out_w): the 'valid' view of an image of shape (h, w[, c]) - the largest rectangle of whole pixels inside
    the undistorted images of its four border rows and columns (aps_undistort_valid_view; an empty one raises ApsError)."""
    v = [C.c_int(0) for _ in range(4)]
    lens = intrinsics.lens()
    check(lib.aps_undistort_valid_view(int(shape[0]), int(shape[1]), C.byref(lens), *(C.byref(x) for x in v)))
    return tuple(x.value for x in v)


def undistortImage(I, intrinsics, OutputView="same", FillValues=0):
    """(J, newOrigin) = undistortImage(I, intrinsics, OutputView, FillValues) on the device (aps_undistort_image_u8): bilinear,
    uint8 H x W or H x W x {1, 3}.  OutputView 'same' keeps the input's size and origin (1, 1); 'valid' is undistort_valid_view's
    rectangle.  newOrigin = (x0, y0): pixel (row i, column j), 0-based, of J has the ideal coordinates (x0 + j, y0 + i).  Pixels
    that sample outside I get FillValues (a scalar in 0..255).  A torch CUDA tensor stays resident: the result is a CUDA tensor and
    nothing visits the host."""
    view = str(OutputView).lower()
    if view not in ("same", "valid"):
        raise ValueError(f"unknown OutputView '{OutputView}' ('same' or 'valid')")
    if not (np.isscalar(FillValues) and 0 <= FillValues <= 255 and int(FillValues) == FillValues):
        raise ValueError("FillValues must be an integer scalar in 0..255")
    dev = _capi.is_torch(I) and I.is_cuda
    a = I.contiguous() if _capi.is_torch(I) else np.ascontiguousarray(I)
    if str(a.dtype).split(".")[-1] != "uint8":
        raise TypeError("uint8 images only")
    sq = a.ndim == 2
    if sq:
        a = a[..., None]
    if a.ndim != 3 or int(a.shape[2]) not in (1, 3):
        raise ValueError(f"I must be H x W, H x W x 1 or H x W x 3, got {tuple(I.shape)}")
    h, w, c = (int(v) for v in a.shape)
    x0, y0, oh, ow = (1, 1, h, w) if view == "same" else undistort_valid_view((h, w), intrinsics)
    if dev:
        import torch

        out = torch.empty((oh, ow, c), dtype=torch.uint8, device=a.device)
        torch.cuda.current_stream().synchronize()  # the input came from torch's stream; the library runs on its own
    elif _capi.is_torch(a):
        import torch

        out = torch.empty((oh, ow, c), dtype=torch.uint8)
    else:
        out = np.empty((oh, ow, c), np.uint8)
    lens = intrinsics.lens()
    check(lib.aps_undistort_image_u8(ptr(a), h, w, c, _capi.APS_IMG_U8_HWC, C.byref(lens), oh, ow, x0, y0, int(FillValues), ptr(out)))
    return (out[..., 0] if sq else out), (x0, y0)


def undistortPoints(points, intrinsics):
    """undistortedPoints = undistortPoints(points, intrinsics): n x 2 [x y] float64, 1-based, through the inverse of the lens map
    (aps_undistort_points: 20 fixed-point steps).  A numpy array gives a numpy array, a torch CUDA tensor a resident one."""
    is_t = _capi.is_torch(points)
    p = points if is_t else np.asarray(points, np.float64)
    if p.ndim != 2 or int(p.shape[1]) != 2 or str(p.dtype).split(".")[-1] != "float64":
        raise ValueError(f"points must be n x 2 float64, got {p.dtype} {tuple(p.shape)}")
    n = int(p.shape[0])
    lens = intrinsics.lens()
    if is_t:
        import torch

        src = p.t().contiguous()  # x at [k], y at [n + k]
        dst = torch.empty_like(src)
        if p.is_cuda:
            torch.cuda.current_stream().synchronize()  # torch produced the transpose; the library runs on its own stream
        check(lib.aps_undistort_points(ptr(src), n, n, C.byref(lens), ptr(dst)))
        return dst.t().contiguous()
    src = np.ascontiguousarray(p.T)
    dst = np.empty_like(src)
    check(lib.aps_undistort_points(ptr(src), n, n, C.byref(lens), ptr(dst)))
    return np.ascontiguousarray(dst.T)
