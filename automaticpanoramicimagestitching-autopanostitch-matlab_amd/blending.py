"""Host-side mirror of PP/blending/ (multiBandBlending.m, linearBlending.m)."""
from __future__ import annotations

import numpy as np

from ._capi import check, lib, ptr


def _stack(Ci, Wi):
    K = len(Ci)
    if K < 1 or K != len(Wi):
        raise ValueError("Ci and Wi must be non-empty cell arrays of equal length")
    h, w = np.asarray(Ci[0]).shape[:2]
    C = np.zeros((K, h, w, 3), np.float32)
    W = np.zeros((K, h, w), np.float32)
    for k in range(K):
        c = np.asarray(Ci[k], np.float32)
        if c.ndim == 2:
            c = np.repeat(c[..., None], 3, axis=2)  # C0 == 1 -> repmat (multiBandBlending.m:93-95)
        ww = np.asarray(Wi[k], np.float32)
        if ww.ndim == 3:
            ww = ww[..., 0]
        if c.shape[:2] != (h, w) or ww.shape != (h, w):
            raise ValueError(f"Ci{{{k + 1}}} size differs from Ci{{1}}.")
        C[k], W[k] = c, ww
    return C, W, K, h, w


def maxWeightPartition(Wi):
    """The max-weight partition of K weight maps (aps_maxweight_weights; DESIGN.md, "Max-weight multiband contract"): 1.0
    where a layer is the FIRST of maximal weight and that weight is > 0, else 0.0; a pixel without a positive weight has no
    owner, and a NaN never owns.  Wi: K x h x w, a list of h x w maps or one h x w map.  numpy in, numpy float32 K x h x w
    out; a resident float32 tensor in, a resident result."""
    from ._capi import is_torch

    if is_torch(Wi):
        import torch

        if Wi.dtype != torch.float32 or Wi.ndim not in (2, 3) or Wi.numel() == 0:
            raise ValueError("a resident Wi must be a non-empty float32 K x h x w tensor")
        W = Wi.contiguous()
        W = W[None] if W.ndim == 2 else W
        out = torch.empty_like(W)
        torch.cuda.current_stream().synchronize()  # the library reads Wi on its own stream
    else:
        W = np.ascontiguousarray(np.stack([np.asarray(x, np.float32) for x in Wi]) if isinstance(Wi, (list, tuple))
                                 else np.asarray(Wi, np.float32))
        W = W[None] if W.ndim == 2 else W
        if W.ndim != 3 or W.size == 0:
            raise ValueError("Wi must be K x h x w with K, h, w >= 1")
        out = np.empty_like(W)
    K, h, w = (int(v) for v in W.shape)
    check(lib.aps_maxweight_weights(ptr(W), K, h, w, ptr(out)))
    return out


def multiBandBlending(Ci, Wi, levels, onGPU=True, sigma=1.0, Weights="tent"):
    """F = multiBandBlending(Ci, Wi, levels, onGPU, sigma) (multiBandBlending.m:1-178); F is h x w x 3 single
    in [0,1] (h x w when the inputs are single channel).  Weights = 'maxweight' (not in the reference): Wi is replaced by
    its max-weight partition (maxWeightPartition) before the blend - Brown & Lowe's Eq. 15-19."""
    if int(levels) != levels or levels < 1:
        raise ValueError("levels must be a positive integer")
    if sigma <= 0:
        raise ValueError("sigma must be positive")
    if not isinstance(Weights, str) or Weights.lower() not in ("tent", "maxweight"):
        raise ValueError(f"Weights must be 'tent' or 'maxweight', not {Weights!r}")
    gray = np.asarray(Ci[0]).ndim == 2
    C, W, K, h, w = _stack(Ci, Wi)
    if Weights.lower() == "maxweight":
        check(lib.aps_maxweight_weights(ptr(W), K, h, w, ptr(W)))
    F = np.zeros((h, w, 3), np.float32)
    check(lib.aps_multiband_blend(ptr(C), ptr(W), K, h, w, int(levels), float(sigma), ptr(F)))
    return F[..., 0] if gray else F


def linearBlending(warpedImages, warpedWeights):
    """imageBlended = linearBlending(warpedImages, warpedWeights) (linearBlending.m:1-117); integer inputs are
    rounded and saturated back to their class (:104-112)."""
    if len(warpedImages) == 0:
        return None
    cls = np.asarray(warpedImages[0]).dtype
    gray = np.asarray(warpedImages[0]).ndim == 2
    C, W, K, h, w = _stack(warpedImages, warpedWeights)
    F = np.zeros((h, w, 3), np.float32)
    check(lib.aps_linear_blend(ptr(C), ptr(W), K, h, w, ptr(F)))
    if np.issubdtype(cls, np.integer):
        info = np.iinfo(cls)
        Fd = np.clip(F.astype(np.float64), info.min, info.max)
        F = (np.sign(Fd) * np.floor(np.abs(Fd) + 0.5)).astype(cls)
    else:
        F = F.astype(cls)
    return F[..., 0] if gray else F
