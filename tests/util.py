"""Shared helpers for the tests (seeded synthetic data only; nothing reads /root/reference)."""
import numpy as np


def sift_like(rng, n, dim=128, unit=True):
    """Non-negative, clipped-at-0.2, unit-norm vectors like SIFT descriptors."""
    x = rng.gamma(0.6, 1.0, size=(n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True) + 1e-12
    x = np.minimum(x, 0.2)
    x /= np.linalg.norm(x, axis=1, keepdims=True) + 1e-12
    if not unit:
        x = np.round(x * 512).clip(0, 255)
    return x.astype(np.float32)


def planted_pair(rng, n1, n2, n_common, noise=0.02, unit=True):
    """Two descriptor sets sharing n_common noisy correspondences at random positions."""
    a = sift_like(rng, n1)
    b = sift_like(rng, n2)
    n_common = min(n_common, n1, n2)
    ia = rng.permutation(n1)[:n_common]
    ib = rng.permutation(n2)[:n_common]
    pert = a[ia] + noise * rng.standard_normal((n_common, a.shape[1])).astype(np.float32)
    pert = np.maximum(pert, 0)
    pert /= np.linalg.norm(pert, axis=1, keepdims=True) + 1e-12
    b[ib] = pert
    if not unit:
        a = np.round(a * 512).clip(0, 255).astype(np.float32)
        b = np.round(b * 512).clip(0, 255).astype(np.float32)
    return a.astype(np.float32), b.astype(np.float32), ia, ib


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- the C ABI as the MATLAB gateway calls it: planar images, column-major matrices, padded leading dimensions ----------
# Sentinels that no result can equal: a quiet NaN with a payload (compared as integers), 0xA5 bytes, all-ones indices.
SENTINEL = {np.dtype(np.float32): np.array([0x7FC5A5A5], np.uint32).view(np.float32)[0],
            np.dtype(np.float64): np.array([0x7FF85A5A5A5A5A5A], np.uint64).view(np.float64)[0],
            np.dtype(np.uint8): np.uint8(0xA5), np.dtype(np.uint32): np.uint32(0xFFFFFFFF), np.dtype(np.int32): np.int32(-1)}
_AS_INT = {4: np.uint32, 8: np.uint64, 1: np.uint8}


def as_int(x):
    """The bits of an array as unsigned integers (NaN payloads compare equal, -0.0 differs from +0.0)."""
    x = np.ascontiguousarray(x)
    return x.view(_AS_INT[x.dtype.itemsize])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(as_int(a), as_int(b))


def sentinel_buffer(n, dtype):
    return np.full(int(n), SENTINEL[np.dtype(dtype)], dtype)


def to_planar(img):
    """h x w (x c) uint8 -> the bytes of MATLAB's column-major planar array: element (y, x, q) at y + h * (x + w * q)."""
    return np.ascontiguousarray(np.asarray(img).ravel(order="F"))


def from_planar(buf, shape):
    return np.ascontiguousarray(np.asarray(buf).reshape(shape, order="F"))


def padded(M, layout_colmajor, ld, fill=None):
    """The flat buffer of matrix M (rows x cols) with leading dimension ld > the minimum: element (i, k) at i + k * ld
    (column-major) or i * ld + k (row-major); everything else holds the dtype's sentinel (or `fill`)."""
    M = np.asarray(M)
    r, c = M.shape
    assert ld > (r if layout_colmajor else c), "the leading dimension must be strictly larger than its minimum"
    outer = c if layout_colmajor else r
    buf = np.full(outer * ld, SENTINEL[M.dtype] if fill is None else fill, M.dtype)
    view = buf.reshape(outer, ld)
    if layout_colmajor:
        view[:, :r] = M.T
    else:
        view[:, :c] = M
    return buf


def unpad(buf, rows, cols, layout_colmajor, ld):
    """(the logical rows x cols matrix, True when every element outside it still holds the sentinel)."""
    buf = np.asarray(buf)
    outer, inner = (cols, rows) if layout_colmajor else (rows, cols)
    assert buf.size >= outer * ld
    view = buf[:outer * ld].reshape(outer, ld)
    logical = view[:, :inner].T if layout_colmajor else view[:, :inner]
    sent = as_int(np.array([SENTINEL[buf.dtype]], buf.dtype))[0]
    intact = bool(np.all(as_int(np.ascontiguousarray(view[:, inner:])) == sent)) and bool(np.all(as_int(buf[outer * ld:]) == sent))
    return np.ascontiguousarray(logical), intact


def place(arr, where):
    """A host array as the argument of an ABI call: itself ('host') or a resident copy ('device', a torch tensor)."""
    if where == "host":
        return arr
    import torch

    if arr.dtype == np.uint32:  # (torch has no uint32 arithmetic; the bytes are what the library sees)
        t = torch.from_numpy(arr.view(np.int32)).cuda()
    else:
        t = torch.from_numpy(arr).cuda()
    torch.cuda.synchronize()
    return t


def fetch(x, dtype=None):
    """The host bytes of an argument after the call (the library ran on its own stream: the caller synchronised it)."""
    if isinstance(x, np.ndarray):
        return x
    a = x.cpu().numpy()
    return a.view(dtype) if dtype is not None else a
