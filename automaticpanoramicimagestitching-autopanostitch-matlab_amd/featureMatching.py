"""Host-side mirror of PP/featureMatching/ — same operator names, argument meaning and outputs as the
reference's MATLAB functions, with the arithmetic done by libaps_hip.so on the MI355X.

MATLAB cell arrays become Python lists (n x n cells -> list of lists), structs become dicts, and
index outputs stay 1-based ``float64`` exactly like ``double(matches)`` in
featureMatchingPairwise.m:120.  Inputs may be numpy arrays (host; staged through HBM by the library)
or torch CUDA tensors (device resident; no copies).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib, ptr

DIM = 128


def _as_desc(x):
    """Row-major float32 N x 128 view of a descriptor matrix (numpy or torch); returns (obj, n, ld, layout)."""
    if _capi.is_torch(x):
        import torch

        if x.dtype != torch.float32:
            x = x.float()
        if x.dim() != 2:
            raise ValueError("descriptors must be 2-D")
        if x.stride(1) == 1 and (x.shape[0] <= 1 or x.stride(0) >= x.shape[1]):
            return x, x.shape[0], max(x.stride(0), x.shape[1]), _capi.APS_ROWMAJOR
        if x.stride(0) == 1:  # column-major (MATLAB) storage
            return x, x.shape[0], max(x.stride(1), x.shape[0]), _capi.APS_COLMAJOR
        x = x.contiguous()
        return x, x.shape[0], x.shape[1], _capi.APS_ROWMAJOR
    x = np.asarray(x)
    if x.dtype != np.float32:
        x = x.astype(np.float32)  # normalizeInputs casts non-float input to single (matchFeaturesScratch.m:277-278)
    if x.ndim != 2:
        raise ValueError("descriptors must be 2-D")
    if x.flags.f_contiguous and not x.flags.c_contiguous:
        return x, x.shape[0], x.shape[0], _capi.APS_COLMAJOR
    x = np.ascontiguousarray(x)
    return x, x.shape[0], x.shape[1], _capi.APS_ROWMAJOR


def _opts(MaxRatio, MatchThreshold, Unique, normalize=2):
    o = _capi.aps_match_opts()
    o.max_ratio = float(MaxRatio)
    o.match_threshold = float(MatchThreshold)
    o.unique = 1 if Unique else 0
    o.normalize = int(normalize)
    return o


def nearest2SSDExhaustive(A, B):
    """[idx1, idx2, d1, d2] = nearest2SSDExhaustive(A, B) (matchFeaturesScratch.m:322-366)."""
    A, n1, lda, la = _as_desc(A)
    B, n2, ldb, lb = _as_desc(B)
    if la != lb:
        raise ValueError("A and B must share a storage order")
    if n1 and A.shape[1] != DIM or n2 and B.shape[1] != DIM:
        raise ValueError("Descriptor dimensions must match for non-binary.")
    idx2 = np.zeros(n1, np.uint32)
    d1 = np.zeros(n1, np.float32)
    d2 = np.zeros(n1, np.float32)
    check(lib.aps_match_2nn_ssd(ptr(A), n1, lda, ptr(B), n2, ldb, DIM, la, ptr(idx2), ptr(d1), ptr(d2)))
    return np.arange(1, n1 + 1, dtype=np.float64), idx2, d1, d2


def _normalize_like_reference(A, B):
    """matchFeaturesScratch.m:105-110: both sets are L2-row-normalised (x ./ (||x|| + eps('single')), :232-233)
    iff either has an entry above 2 in magnitude."""
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    if (A.size and np.abs(A).max() > 2) or (B.size and np.abs(B).max() > 2):
        eps = np.float32(np.finfo(np.float32).eps)
        A = A / (np.sqrt((A * A).sum(1, dtype=np.float32, keepdims=True)) + eps)
        B = B / (np.sqrt((B * B).sum(1, dtype=np.float32, keepdims=True)) + eps)
    return np.ascontiguousarray(A, np.float32), np.ascontiguousarray(B, np.float32)


def _pad_dim(X):
    """The device 2-NN kernel is built for 128-D rows; shorter rows are zero-padded (distances unchanged)."""
    X = np.ascontiguousarray(X, np.float32)
    if X.shape[1] == DIM:
        return X
    if X.shape[1] > DIM:
        raise ValueError(f"descriptor length {X.shape[1]} > {DIM}")
    out = np.zeros((X.shape[0], DIM), np.float32)
    out[:, : X.shape[1]] = X
    return out


def _pad_rows(X):
    """A descriptor set as the 128-wide matchers take it: narrower rows (SURF: 64) are zero-padded, on the host or on the
    device as the set lives; distances, and with them every match list, are those of the padded rows.  128-wide sets pass
    through untouched."""
    if not hasattr(X, "ndim"):
        X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] >= DIM or X.shape[0] == 0:
        return X
    if _capi.is_torch(X):
        import torch

        out = torch.zeros((X.shape[0], DIM), dtype=torch.float32, device=X.device)
        out[:, : X.shape[1]] = X
        if X.is_cuda:
            torch.cuda.current_stream().synchronize()  # torch made the copy; the library reads it on its own stream
        return out
    return _pad_dim(X)


def nearest2KDTree(A, B, bucketSize=40):
    """[idx1, idx2, d1, d2] = nearest2KDTree(A, B, bucketSize) (matchFeaturesScratch.m:411-440).  knnsearch on a
    kd-tree is EXACT, so this is the exhaustive device search; d are Euclidean distances (the caller squares
    them, :152-153).  bucketSize only shapes the reference's tree and has no effect on the result."""
    idx1, idx2, d1, d2 = nearest2SSDExhaustive(_pad_dim(A), _pad_dim(B))
    return idx1, idx2, np.sqrt(np.maximum(d1, 0)), np.sqrt(np.maximum(d2, 0))


def nearest2SubsetPdist2(A, B, subset=12000, candB=None, seed=0):
    """[idx1, idx2, d1, d2] = nearest2SubsetPdist2(A, B, subset) (matchFeaturesScratch.m:368-409): exact 2-NN
    (Euclidean) against a random `subset`-row sample of B, indices mapped back into B.  The sample is an
    explicit input here (candB, 1-based) or drawn from `seed`; the reference uses the unseeded randperm (:377)."""
    B = np.asarray(B, np.float32)
    n2 = B.shape[0]
    subset = min(int(subset), n2)
    if candB is None:
        candB = np.random.default_rng(seed).permutation(n2)[:subset] + 1
    candB = np.asarray(candB, np.int64).reshape(-1)
    if candB.size != subset or candB.min() < 1 or candB.max() > n2 or np.unique(candB).size != subset:
        raise ValueError("candB must hold `subset` distinct 1-based rows of B")
    idx1, i2, d1, d2 = nearest2SSDExhaustive(_pad_dim(A), _pad_dim(B[candB - 1]))
    e1, e2 = np.sqrt(np.maximum(d1, 0)), np.sqrt(np.maximum(d2, 0))
    if subset == 1:  # :385-388: a second "neighbour" one ulp away
        e2 = e1 + np.spacing(e1)
    return idx1, candB[i2.astype(np.int64) - 1].astype(np.uint32), e1, e2


def nearest2ApproxFloatFast(A, B, opts=None, return_basis=False):
    """[idx1, idx2, dBest, dSecond] = nearest2ApproxFloatFast(A, B, opts) (matchFeaturesScratch.m:442-573): PCA of B
    to ApproxNumComponents (48) dimensions, both sets centred with B's mean and projected, L2-normalised, then the top
    two cosine similarities per row of A, returned as d = 2 - 2*sim.  All of it on the device (aps_match_pca2nn: column
    means and the covariance B'B through the f32 MFMA path, projection, normalisation, the cosine product and its top
    two); only the 128 x 128 symmetric eigen-problem is solved on the host (inside the library).  opts: 'UsePCA',
    'ApproxNumComponents' as in the reference; BlockRows / UseParfor / UseGPU only partition the reference's loop and
    have no effect on a row's result.  return_basis: also (mu, coeff) of the projection (None when it is skipped)."""
    o = {"ApproxNumComponents": 48, "UsePCA": True}
    o.update(opts or {})
    A, n1, lda, la = _as_desc(A)
    B, n2, ldb, lb = _as_desc(B)
    if la != lb:
        raise ValueError("A and B must share a storage order")
    if n1 == 0 or n2 == 0:
        raise ValueError("Expected input to be nonempty.")
    if A.shape[1] != DIM or B.shape[1] != DIM:
        raise ValueError("Descriptor dimensions must match for non-binary.")
    k = int(o["ApproxNumComponents"])
    idx2 = np.zeros(n1, np.uint32)
    d1 = np.zeros(n1, np.float32)
    d2 = np.zeros(n1, np.float32)
    projected = bool(o["UsePCA"]) and DIM > k
    mu = np.zeros(DIM, np.float32) if return_basis and projected else None
    coeff = np.zeros((DIM, k), np.float32) if return_basis and projected else None
    check(lib.aps_match_pca2nn(ptr(A), n1, lda, ptr(B), n2, ldb, DIM, la, k, int(bool(o["UsePCA"])), ptr(idx2), ptr(d1), ptr(d2),
                               ptr(mu) if mu is not None else None, ptr(coeff) if coeff is not None else None))
    out = (np.arange(1, n1 + 1, dtype=np.float64), idx2, d1, d2)
    return out + ((mu, coeff),) if return_basis else out


def filter_matches(idx2, dBest, dSecond, n2, MaxRatio, MatchThreshold, Unique, binary=False):
    """matchFeaturesScratch.m:170-211 on the host (used by the approximate back ends and the binary branch, whose 2-NN
    lists live on the host): ratio on SSD (r^2), threshold, finiteness, greedy one-to-one by ascending distance (stable).
    binary=True: the distances are percent mismatched bits and the ratio is linear (:171), evaluated in single as MATLAB
    evaluates double scalar * single array."""
    dBest = np.asarray(dBest, np.float32)
    dSecond = np.asarray(dSecond, np.float32)
    if binary:
        keep = (dBest <= np.float32(MaxRatio) * dSecond) & (dBest <= np.float32(MatchThreshold)) & np.isfinite(dBest) & np.isfinite(dSecond)
    else:
        # the reference holds dBest/dSecond in double arrays (inf(N1,1), :344) and evaluates MaxRatio^2 in double
        r2 = float(MaxRatio) * float(MaxRatio)
        b64, s64 = dBest.astype(np.float64), dSecond.astype(np.float64)
        keep = (b64 <= r2 * s64) & (b64 <= float(MatchThreshold)) & np.isfinite(b64) & np.isfinite(s64)
    i1 = np.flatnonzero(keep).astype(np.uint32) + 1
    i2 = np.asarray(idx2, np.uint32)[keep]
    d = dBest[keep]
    if Unique and i1.size:
        order = np.argsort(d, kind="stable")
        i1, i2, d = i1[order], i2[order], d[order]
        used2 = np.zeros(n2 + 1, bool)
        sel = np.zeros(i1.size, bool)
        for k in range(i1.size):  # rows are unique already; first come, first served on the columns
            if not used2[i2[k]]:
                used2[i2[k]] = True
                sel[k] = True
        i1, i2, d = i1[sel], i2[sel], d[sel]
    return np.stack([i1, i2], axis=1), d.astype(np.float32)


class binaryFeatures:
    """Stand-in for MATLAB's binaryFeatures object: .Features is uint8 n x nbytes (packed bits; numpy, or a resident torch
    tensor), .NumFeatures = n, .NumBits = 8 * nbytes."""

    def __init__(self, Features):
        if _capi.is_torch(Features):
            import torch

            if Features.dtype != torch.uint8 or Features.dim() != 2:
                raise TypeError("binaryFeatures takes a 2-D uint8 matrix")
            self.Features = Features.contiguous()
        else:
            F = np.asarray(Features)
            if F.dtype != np.uint8 or F.ndim != 2:
                raise TypeError("binaryFeatures takes a 2-D uint8 matrix")
            self.Features = np.ascontiguousarray(F)

    @property
    def NumFeatures(self):
        return int(self.Features.shape[0])

    @property
    def NumBits(self):
        return 8 * int(self.Features.shape[1])

    def __len__(self):
        return self.NumFeatures


def packBits(unpacked01):
    """[packed, nBits] = packBits(unpacked01) (matchFeaturesScratch.m:618-645): n x D bits -> n x ceil(D / 8) uint8,
    bit b of a row (1-based) into byte ceil(b / 8), MSB first."""
    U = np.asarray(unpacked01)
    if U.ndim != 2 or U.dtype not in (np.bool_, np.uint8):
        raise TypeError("packBits takes a 2-D logical or uint8 matrix")
    return np.packbits(U.astype(bool), axis=1, bitorder="big"), int(U.shape[1])


def _binary_inputs(F1, F2):
    """normalizeInputs' binary cases (matchFeaturesScratch.m:259-275): (A bytes, B bytes, nBits), or None for the float
    path.  Deviation from :266-268: a plain uint8 matrix is NOT inspected for holding only 0 / 1 - it keeps the float path it
    always had here; unpacked bits are given as bool arrays."""
    if isinstance(F1, binaryFeatures) and isinstance(F2, binaryFeatures):
        return F1.Features, F2.Features, F1.NumBits
    if isinstance(F1, binaryFeatures) or isinstance(F2, binaryFeatures):
        raise TypeError("both sets must be binaryFeatures")
    if isinstance(F1, np.ndarray) and isinstance(F2, np.ndarray) and F1.dtype == np.bool_ and F2.dtype == np.bool_:
        A, nBits = packBits(F1)
        B, _ = packBits(F2)
        return A, B, nBits
    return None


def _hamming_2nn(A, B):
    """aps_hamming_2nn on packed rows that live on the host (numpy) or on the device (torch): (idx2, d1, d2) on the host."""
    if A.shape[1] != B.shape[1]:
        raise ValueError("Byte width mismatch.")  # hamm2nn:cols
    n1 = int(A.shape[0])
    idx2 = np.zeros(n1, np.uint32)
    d1 = np.zeros(n1, np.float32)
    d2 = np.zeros(n1, np.float32)
    check(lib.aps_hamming_2nn(ptr(A), n1, A.shape[1], ptr(B), int(B.shape[0]), B.shape[1], A.shape[1],
                              _capi.APS_ROWMAJOR, ptr(idx2), ptr(d1), ptr(d2)))
    return idx2, d1, d2


def _match_binary(A, B, nBits, MaxRatio, MatchThreshold, Unique):
    """The binary branch of matchFeaturesScratch.m:84-88,118-121,170-211 on packed bytes."""
    n1, n2 = int(A.shape[0]), int(B.shape[0])
    if n1 == 0 or n2 == 0:  # :84-88
        return np.zeros((0, 2), np.uint32), np.zeros(0, np.float32)
    idx2, d1, d2 = _hamming_2nn(A, B)
    d2[~np.isfinite(d2) | (d2 == 0)] = np.float32(nBits)  # :318
    nb = np.float32(nBits)
    return filter_matches(idx2, (d1 / nb) * np.float32(100), (d2 / nb) * np.float32(100), n2, MaxRatio, MatchThreshold, Unique, binary=True)


def matchFeaturesScratch(F1, F2, Method="Exhaustive", MatchThreshold=3.5, MaxRatio=0.6, Unique=True,
                         ApproxFloatNNMethod="pca2nn", ApproxKDBucketSize=40, candB=None, seed=0, ZeroPad=False,
                         **_ignored_approx_args):
    """[matches, matchMetric] = matchFeaturesScratch(F1, F2, 'Method', ..., 'MatchThreshold', ...,
    'MaxRatio', ..., 'Unique', ...) (matchFeaturesScratch.m:1-215).

    Binary branch (:81-135,170-171): a pair of binaryFeatures, or a pair of bool arrays (unpacked bits, packed by packBits),
    is searched by the device Hamming 2-NN (aps_hamming_2nn; an empty side gives empty results, :84-88); distances are
    percent mismatched bits, the ratio is linear, MatchThreshold is in percent (:32 suggests 10 or more).  'Approximate' runs
    the same exact search: the reference's LSH function itself calls the exhaustive mex (:611).  Deviation from :266-268:
    plain uint8 arrays are not inspected for 0 / 1 content and keep the float path.
    Float descriptors:

    'Exhaustive' (the north-star path): 2-NN + ratio/threshold/uniqueness fused on the device.
    'Approximate' float back ends (:142-160), selected by ApproxFloatNNMethod: 'pca2nn' (PCA-48 + cosine),
    'kdtree' (exact), 'subsetpdist2' (random 12000-row subset of F2; pass candB or seed): their 2-NN search is
    the same device kernel on the transformed data, the filter runs on the host.
    ZeroPad=True ('Exhaustive'): rows shorter than the 128 the kernels are built for (SURF's 64) are zero-padded, which
    leaves every distance and so the match list unchanged; by default such sets are refused, as they always were.
    Returns (matches K x 2 uint32 1-based, matchMetric K float32)."""
    method = str(Method).lower()
    if method not in ("exhaustive", "approximate"):
        raise ValueError(f"Unknown Method: {Method}")
    if not (0 < MaxRatio <= 1) or MatchThreshold < 0:
        raise ValueError("invalid MaxRatio/MatchThreshold")
    packed = _binary_inputs(F1, F2)
    if packed is not None:
        return _match_binary(*packed, MaxRatio, MatchThreshold, Unique)
    if method == "approximate":
        An, Bn = _normalize_like_reference(F1, F2)
        if An.shape[0] == 0 or Bn.shape[0] == 0:
            raise ValueError("Expected input to be nonempty.")
        am = str(ApproxFloatNNMethod).lower()
        if am == "pca2nn":
            _, idx2, d1, d2 = nearest2ApproxFloatFast(An, Bn, {"ApproxNumComponents": 48, "UsePCA": True})
        elif am == "kdtree":
            _, idx2, e1, e2 = nearest2KDTree(An, Bn, ApproxKDBucketSize)
            d1, d2 = e1 * e1, e2 * e2  # :152-153
        elif am == "subsetpdist2":
            _, idx2, e1, e2 = nearest2SubsetPdist2(An, Bn, 12000, candB, seed)
            d1, d2 = e1 * e1, e2 * e2  # :156-157
        else:
            raise ValueError("Select a approximate method")
        return filter_matches(idx2, d1, d2, Bn.shape[0], MaxRatio, MatchThreshold, Unique)
    A, n1, ld1, la = _as_desc(F1)
    B, n2, ld2, lb = _as_desc(F2)
    if n1 == 0 or n2 == 0:
        raise ValueError("Expected input to be nonempty.")  # validateattributes(... 'nonempty') :279-280
    if A.shape[1] != B.shape[1]:
        raise ValueError("Descriptor dimensions must match for non-binary.")
    if ZeroPad and A.shape[1] < DIM:  # SURF's 64-wide rows
        A, n1, ld1, la = _as_desc(_pad_rows(A))
        B, n2, ld2, lb = _as_desc(_pad_rows(B))
    if la != lb:
        B = np.ascontiguousarray(B) if la == _capi.APS_ROWMAJOR else np.asfortranarray(B)
        B, n2, ld2, lb = _as_desc(B)
    cap = n1
    i1 = np.zeros(cap, np.uint32)
    i2 = np.zeros(cap, np.uint32)
    met = np.zeros(cap, np.float32)
    cnt = C.c_int64(0)
    o = _opts(MaxRatio, MatchThreshold, Unique)
    check(lib.aps_match_features(ptr(A), n1, ld1, ptr(B), n2, ld2, A.shape[1], la, C.byref(o), ptr(i1),
                                 ptr(i2), ptr(met), cap, C.byref(cnt)))
    k = cnt.value
    return np.stack([i1[:k], i2[:k]], axis=1), met[:k].copy()


def _desc_table(allDescriptors):
    """The descriptor sets of a float CSR matcher as the library takes them: (ptrs, counts, lds, layout, rows per set, and the
    prepared arrays, which the caller keeps alive for the length of the call).  Sets of mixed storage order are a ValueError."""
    n = len(allDescriptors)
    prepared = [_as_desc(_pad_rows(d)) for d in allDescriptors]
    layouts = {p[3] for p in prepared if p[1] > 0}
    if len(layouts) > 1:
        raise ValueError("all descriptor matrices must share a storage order")
    layout = layouts.pop() if layouts else _capi.APS_ROWMAJOR
    ptrs = (C.c_void_p * n)(*[ptr(p[0]) if p[1] > 0 else None for p in prepared])
    counts = (C.c_int64 * n)(*[p[1] for p in prepared])
    lds = (C.c_int64 * n)(*[max(p[2], DIM if layout == _capi.APS_ROWMAJOR else p[1]) for p in prepared])
    return ptrs, counts, lds, layout, [p[1] for p in prepared], prepared


def _match_lists_regrow(call, cap, device_out):
    """The output lists of a float CSR matcher with automatic capacity: call(idx_a, idx_b, metric, cap, count) runs the library
    entry on freshly allocated lists (resident with device_out, fenced against torch's stream) and returns its status; on
    APS_E_CAP the count is the exact need and the call is repeated with it.  Returns the three lists cut to the count."""
    cnt = C.c_int64(0)
    while True:
        if device_out:
            import torch

            i_a = torch.empty(cap, dtype=torch.int32, device="cuda")
            i_b = torch.empty(cap, dtype=torch.int32, device="cuda")
            met = torch.empty(cap, dtype=torch.float32, device="cuda")
            _fence_fresh_blocks()
        else:
            i_a = np.zeros(cap, np.uint32)
            i_b = np.zeros(cap, np.uint32)
            met = np.zeros(cap, np.float32)
        rc = call(ptr(i_a), ptr(i_b), ptr(met), cap, C.byref(cnt))
        if rc == _capi.APS_E_CAP:
            cap = cnt.value
            continue
        check(rc)
        k = cnt.value
        return i_a[:k], i_b[:k], met[:k]


def match_pairwise_csr(allDescriptors, MaxRatio, MatchThreshold, Unique=True, normalize=2,
                       device_out=False):
    """Batched all-pairs matcher: the CSR form of featureMatchingPairwise used by the resident pipeline.
    Returns (pair_ptr int64[P+1], idx_i, idx_j, metric) with pairs in the reference's triu order."""
    n = len(allDescriptors)
    ptrs, counts, lds, layout, ns, _keep = _desc_table(allDescriptors)
    pair_ptr = np.zeros(n * (n - 1) // 2 + 1, np.int64)
    o = _opts(MaxRatio, MatchThreshold, Unique, normalize)
    # resident outputs: room for every row of every pair (see match_pairs_csr); host outputs: a modest first capacity,
    # APS_E_CAP reports the exact need
    rows = sum(ns[i] * (n - 1 - i) for i in range(n))  # pair (i, j), i < j, has image i's rows
    cap = max(1, rows if device_out else sum(ns) // 4)
    return (pair_ptr,) + _match_lists_regrow(
        lambda *out: lib.aps_match_pairwise(ptrs, counts, lds, n, DIM, layout, C.byref(o), ptr(pair_ptr), *out), cap, device_out)


def match_pairs_csr(allDescriptors, pairs, MaxRatio, MatchThreshold, Unique=True, normalize=2, device_out=False):
    """aps_match_pairs: the matcher on an explicit list of (a, b) image pairs (0-based) — the unit that is
    sharded across GPUs.  Returns (pair_ptr int64[P+1], idx_a, idx_b, metric) as numpy arrays, or with
    device_out=True the three match arrays as resident torch tensors (int32, int32, float32)."""
    n = len(allDescriptors)
    ptrs, counts, lds, layout, ns, _keep = _desc_table(allDescriptors)
    if isinstance(pairs, np.ndarray):  # [P, 2] (pair_order_array and slices of it)
        pa = np.ascontiguousarray(pairs[:, 0], np.int32)
        pb = np.ascontiguousarray(pairs[:, 1], np.int32)
    else:
        pa = np.ascontiguousarray([p[0] for p in pairs], np.int32)
        pb = np.ascontiguousarray([p[1] for p in pairs], np.int32)
    P = len(pairs)
    pair_ptr = np.zeros(P + 1, np.int64)
    o = _opts(MaxRatio, MatchThreshold, Unique, normalize)
    rows = int(np.asarray(ns, np.int64)[pa].sum()) if P else 0
    # resident outputs: room for every row (uninitialised device memory from torch's cache costs nothing, and a second
    # pass over all pairs after APS_E_CAP costs the whole matcher again - well-overlapping small sets keep more than a
    # sixteenth of their rows); host outputs: a sixteenth, grown on demand
    cap = max(1, rows if device_out else rows // 16)
    return (pair_ptr,) + _match_lists_regrow(
        lambda *out: lib.aps_match_pairs(ptrs, counts, lds, n, DIM, layout, ptr(pa), ptr(pb), P, C.byref(o), ptr(pair_ptr), *out),
        cap, device_out)


_PAIR_ORDER = {}


def pair_order(numImg):
    """The reference's pair order: nonzeros(triu(reshape(1:n^2,n,n),1)) (featureMatchingPairwise.m:48).  (Cached per image
    count: a step asks for it several times; callers do not modify the list.)"""
    numImg = int(numImg)
    if numImg not in _PAIR_ORDER:
        _PAIR_ORDER[numImg] = [(i, j) for j in range(1, numImg) for i in range(j)]
    return _PAIR_ORDER[numImg]


_PAIR_ORDER_ARR = {}


def pair_order_array(numImg):
    """pair_order as a read-only int32 array [P, 2] (cached): match_pairs_csr takes it without walking 2016 tuples."""
    numImg = int(numImg)
    if numImg not in _PAIR_ORDER_ARR:
        a = np.asarray(pair_order(numImg), np.int32).reshape(-1, 2)
        a.setflags(write=False)
        _PAIR_ORDER_ARR[numImg] = a
    return _PAIR_ORDER_ARR[numImg]


def _hamming_opts(MaxRatio, MatchThreshold, Unique, nbits=0):
    o = _capi.aps_hamming_match_opts()
    o.max_ratio = float(MaxRatio)
    o.match_threshold = float(MatchThreshold)
    o.unique = 1 if Unique else 0
    o.nbits = int(nbits)
    return o


def _binary_sets(allDescriptors):
    """The sets of a binary list as (byte matrices, bit widths): all binaryFeatures, or all bool arrays (unpacked bits, packed
    by packBits); anything else mixed in raises, as the per-pair branch does."""
    if all(isinstance(d, binaryFeatures) for d in allDescriptors):
        return [d.Features for d in allDescriptors], [d.NumBits for d in allDescriptors]
    if any(isinstance(d, binaryFeatures) for d in allDescriptors):
        raise TypeError("both sets must be binaryFeatures")
    if not all(isinstance(d, np.ndarray) and d.dtype == np.bool_ and d.ndim == 2 for d in allDescriptors):
        raise TypeError("binary sets are binaryFeatures, or bool arrays of unpacked bits")
    return [packBits(d)[0] for d in allDescriptors], [int(d.shape[1]) for d in allDescriptors]


def match_pairs_binary_csr(allDescriptors, pairs, MaxRatio, MatchThreshold, Unique=True, device_out=False, max_columns=None):
    """aps_hamming_match_pairs: matchFeaturesScratch's binary branch on an explicit list of (a, b) image pairs (0-based; rows of
    a searched in b) in one batched device call - the lists of matchFeaturesScratch(allDescriptors[a], allDescriptors[b], ...)
    pair after pair, element for element.  pairs = None: every pair of pair_order (aps_hamming_match_pairwise).
    allDescriptors: binaryFeatures (host or resident), or bool arrays of unpacked bits.  Returns (pair_ptr int64[P+1], idx_a,
    idx_b uint32 1-based, metric float32 percent) as numpy arrays; with device_out=True the three lists are resident torch
    tensors (int32, int32, float32; empty ones when nothing matches or no pair has two non-empty sides), and resident sets never
    leave the device.  pair_ptr is a numpy array either way, as match_pairs_csr's: P + 1 offsets the host indexes the lists with.
    The sets that meet in a pair with two non-empty sides share one byte and bit width (ValueError otherwise; one call has
    one width); sets that meet only empty partners may be of any width.
    max_columns: bound on the per-column workspace of the uniqueness step (columns of the pairs in flight; the pair list is
    walked in chunks under it, same results) - for tests of the chunked walk and hosts short of device memory."""
    if not (0 < MaxRatio <= 1) or MatchThreshold < 0:
        raise ValueError("invalid MaxRatio/MatchThreshold")
    n = len(allDescriptors)
    sets, bits = _binary_sets(allDescriptors)
    cnt = np.asarray([int(s.shape[0]) for s in sets], np.int64)
    if pairs is None:
        pp = pair_order_array(n)
    elif isinstance(pairs, np.ndarray):
        pp = pairs.reshape(-1, 2)
    else:
        pp = np.asarray([(p[0], p[1]) for p in pairs], np.int32).reshape(-1, 2)
    pa, pb = np.ascontiguousarray(pp[:, 0], np.int32), np.ascontiguousarray(pp[:, 1], np.int32)
    P = len(pa)
    if P and (min(pa.min(), pb.min()) < 0 or max(pa.max(), pb.max()) >= n):
        raise ValueError("image index out of range in the pair list")
    width = np.asarray([int(s.shape[1]) for s in sets], np.int64)
    bits = np.asarray(bits, np.int64)
    live = (cnt[pa] > 0) & (cnt[pb] > 0) if P else np.zeros(0, bool)
    # one width for the sets that meet: bytes (hamm2nn:cols), and bits too (a pair of unpacked sets of 250 and 252 bits shares
    # the byte width, not the divisor)
    if np.any(width[pa[live]] != width[pb[live]]) or np.unique(width[pa[live]]).size > 1 or np.unique(bits[pa[live]]).size > 1 \
            or np.any(bits[pa[live]] != bits[pb[live]]):
        raise ValueError("Byte width mismatch.")  # hamm2nn:cols
    # a set that meets only empty partners takes no part (its width does not matter, as pair by pair): handed over as empty
    used = np.zeros(n, bool)
    used[pa[live]] = used[pb[live]] = True
    cnt = np.where(used, cnt, 0)
    nbytes, nbits = (int(width[pa[live]][0]), int(bits[pa[live]][0])) if live.any() else (1, 0)
    if nbits == 8 * nbytes:
        nbits = 0
    ptrs = (C.c_void_p * n)(*[ptr(s) if c else None for s, c in zip(sets, cnt)])
    counts = (C.c_int64 * n)(*cnt.tolist())
    lds = (C.c_int64 * n)(*[max(int(w), 1) for w in width])  # row-major, contiguous (binaryFeatures, packBits)
    pair_ptr = np.zeros(P + 1, np.int64)
    o = _hamming_opts(MaxRatio, MatchThreshold, Unique, nbits)
    total = C.c_int64(0)
    cap = int(cnt[pa][live].sum()) if P else 0  # every row of every pair: always enough, and only the matches are written
    if device_out:
        import torch

        i_a = torch.empty(cap, dtype=torch.int32, device="cuda")
        i_b = torch.empty(cap, dtype=torch.int32, device="cuda")
        met = torch.empty(cap, dtype=torch.float32, device="cuda")
        _fence_fresh_blocks()
    else:
        i_a, i_b, met = np.empty(cap, np.uint32), np.empty(cap, np.uint32), np.empty(cap, np.float32)
    out = (ptr(pair_ptr), ptr(i_a) if cap else None, ptr(i_b) if cap else None, ptr(met) if cap else None, cap, C.byref(total))
    lay = _capi.APS_ROWMAJOR
    if max_columns is not None:  # the library's internal entry with the bound as an argument (not part of aps.h)
        bounded = lib.aps_hamming_match_pairs_bounded
        bounded.restype = C.c_int
        bounded.argtypes = list(lib.aps_hamming_match_pairs.argtypes) + [C.c_int64]
        lists = (None, None) if pairs is None else (ptr(pa), ptr(pb))
        check(bounded(ptrs, counts, lds, n, nbytes, lay, *lists, P, C.byref(o), *out, int(max_columns)))
    elif pairs is None:
        check(lib.aps_hamming_match_pairwise(ptrs, counts, lds, n, nbytes, lay, C.byref(o), *out))
    else:
        check(lib.aps_hamming_match_pairs(ptrs, counts, lds, n, nbytes, lay, ptr(pa), ptr(pb), P, C.byref(o), *out))
    k = total.value
    return pair_ptr, i_a[:k], i_b[:k], met[:k]


def match_pairwise_binary_csr(allDescriptors, MaxRatio, MatchThreshold, Unique=True):
    """match_pairwise_csr for lists of binaryFeatures: every pair of pair_order through matchFeaturesScratch's binary branch, all
    of them in one batched device call (match_pairs_binary_csr).
    Returns (pair_ptr int64[P+1], idx_i, idx_j uint32 1-based, metric float32 percent) on the host."""
    return match_pairs_binary_csr(allDescriptors, None, MaxRatio, MatchThreshold, Unique)


def featureMatchingPairwise(input, allDescriptors, numImg):
    """matches = featureMatchingPairwise(input, allDescriptors, numImg) (featureMatchingPairwise.m:1-63).

    Returns an n x n list of lists; cell (i, j), i < j, holds an M x 2 float64 array of 1-based
    [idx_i idx_j]; every other cell is None (MATLAB: empty)."""
    numImg = int(numImg)
    if numImg <= 0 or len(allDescriptors) != numImg:
        raise ValueError("numImg must be positive and match numel(allDescriptors)")
    thr = input.get("Matchingthreshold", 1.5)
    ratio = input.get("Ratiothreshold", 0.6)
    if int(input.get("useMATLABFeatureMatch", 0)) == 1:
        # getMatches :103-107 hands the pair to the toolbox's matchFeatures (closed code): no device counterpart
        raise NotImplementedError("input.useMATLABFeatureMatch = 1 selects the Computer Vision Toolbox's matchFeatures; "
                                  "set it to 0 for the device matcher (the MATLAB overlay forwards this switch to the reference)")
    matches = [[None] * numImg for _ in range(numImg)]
    if any(isinstance(d, binaryFeatures) for d in allDescriptors):
        # binary sets: the reference's pair loop (:48-63) around matchFeaturesScratch's binary branch, as one batched device call
        pair_ptr, ii, jj, _ = match_pairwise_binary_csr(allDescriptors, ratio, thr, True)
        for p, (i, j) in enumerate(pair_order(numImg)):
            s, e = pair_ptr[p], pair_ptr[p + 1]
            matches[i][j] = np.stack([ii[s:e], jj[s:e]], axis=1).astype(np.float64)
        return matches
    if str(input.get("Matchingmethod", "Exhaustive")).lower() == "approximate":
        # getMatches :108-117 with Method = 'Approximate': pair by pair through matchFeaturesScratch, as the reference's parfor
        # (:48-63) does; 'pca2nn' = nearest2ApproxFloatFast on the device, 'kdtree' / 'subsetpdist2' the exact device search
        for (i, j) in pair_order(numImg):
            m, _ = matchFeaturesScratch(allDescriptors[i], allDescriptors[j], Method="Approximate", MatchThreshold=thr, MaxRatio=ratio,
                                        Unique=True, ApproxFloatNNMethod=input.get("ApproxFloatNNMethod", "pca2nn"))
            matches[i][j] = np.asarray(m, np.float64).reshape(-1, 2)
        return matches
    pair_ptr, ii, jj, _ = match_pairwise_csr(allDescriptors, ratio, thr, True)
    for p, (i, j) in enumerate(pair_order(numImg)):
        s, e = pair_ptr[p], pair_ptr[p + 1]
        matches[i][j] = np.stack([ii[s:e], jj[s:e]], axis=1).astype(np.float64)
    return matches


# ---- getFeaturePoints (getFeaturePoints.m:1-76) ----------------------------------------------------
def _sift_params(input):
    p = _capi.aps_sift_params()
    p.sigma = float(input.get("Sigma", 1.6))
    p.n_layers = int(input.get("NumLayersInOctave", 4))
    p.contrast_threshold = float(input.get("ContrastThreshold", 0.00133))
    p.edge_threshold = float(input.get("EdgeThreshold", 6))
    p.max_features = int(input.get("maxFeatures", 0))
    return p


def _sift_strongest_params(input, n=None):
    p = _capi.aps_sift_strongest_params()
    p.sift = _sift_params(input)
    p.n_strongest = int(input["NumStrongest"] if n is None else n)
    return p


def _uniform_keys(input):
    """(N, rows, cols) of input.NumUniform and input.UniformGrid (default 8 x 8), or None without NumUniform (UniformGrid alone is
    ignored).  NumUniform next to NumStrongest is a ValueError, raised before any library call; the values themselves are the
    library's to refuse (APS_E_ARG)."""
    if "NumUniform" not in input:
        return None
    if "NumStrongest" in input:
        raise ValueError("input.NumUniform and input.NumStrongest exclude each other: one selection rule per call")
    rows, cols = input.get("UniformGrid", (8, 8))
    return int(input["NumUniform"]), int(rows), int(cols)


def _uniform_params(struct, strongest, uniform):
    """aps_*_uniform_params around the detector's strongest params, whose n_strongest is N."""
    p = struct()
    p.strongest = strongest
    p.grid_rows, p.grid_cols = uniform[1:]
    return p


def _fence_fresh_blocks():
    """torch's caching allocator recycles a freed block for the next torch.empty at once, which is safe for consumers on
    torch's own stream only: kernels that were queued there before the block was freed (by ANY thread) may still be
    running.  The library writes on its private per-thread streams, so a freshly allocated output buffer is fenced
    against torch's stream before it is handed over (the stream is nearly idle in this pipeline: the wait is short)."""
    import torch

    torch.cuda.current_stream().synchronize()


def _image_hwc(image):
    """The image preamble of the extraction wrappers: (contiguous uint8 image, h, w, c) of an H x W [x C] numpy array or torch
    tensor; channel counts other than 1 and 3 are a ValueError."""
    if _capi.is_torch(image):
        img = image.contiguous()
        h, w = int(img.shape[0]), int(img.shape[1])
        c = 1 if img.dim() == 2 else int(img.shape[2])
    else:
        img = np.ascontiguousarray(image, np.uint8)
        h, w = img.shape[:2]
        c = 1 if img.ndim == 2 else img.shape[2]
    if c not in (1, 3):
        raise ValueError("image must be gray or RGB")
    return img, h, w, c


def _pick_entry(input, uniform, cap, plain, strongest, uniform_struct, uniform_entry):
    """(parameter struct, library entry, first capacity) of an extraction call, from the detector's own pieces.
    plain: (params, entry) without a selection key; strongest: (builder of the strongest params taking N or None for
    input.NumStrongest, entry); uniform: what _uniform_keys(input) returned (the caller asks first: its ValueError comes before
    any library call), with the detector's uniform struct and entry; cap: the capacity without a selection key.
    With a selection of N rows the capacity is min(cap, max(N, 1)): a resident result then holds N rows (a value below 1 is the
    library's to refuse)."""
    (prm, entry), n_keep = plain, None
    if "NumStrongest" in input:
        prm, entry = strongest[0](None), strongest[1]
        n_keep = prm.n_strongest
    if uniform:
        prm, entry = _uniform_params(uniform_struct, strongest[0](uniform[0]), uniform), uniform_entry
        n_keep = uniform[0]
    return prm, entry, (cap if n_keep is None else min(cap, max(n_keep, 1)))


def _extract_regrow(g, cap, call, retry, width, dtype, device_out, points_device, compact, want_aux):
    """The driver of every extraction wrapper: allocate the outputs of g views -> fence -> call -> regrow on APS_E_CAP -> finish.
    call(bufs, cap) runs the library entry on bufs = [(desc, loc, aux)] * g, each of capacity `cap` (desc: cap x width rows of
    `dtype`, resident with device_out; loc: column-major cap x 2 float64, resident with device_out and points_device; aux: cap x 4
    float32 on the host, or None) and returns (status, [count per view]).  On APS_E_CAP with retry(counts, cap) true, everything
    is allocated again with the largest count as every view's capacity.
    Returns [(rows, points, aux or None)] * g: rows is the first count rows of the capacity buffer (resident: a view, or a
    right-sized clone with compact), points count x 2.
    Streams: fresh resident buffers are fenced against torch's stream once per attempt (_fence_fresh_blocks); the library's stream
    is drained before torch reads resident outputs (an entry whose outputs are all resident returns before its last kernel);
    torch's stream is drained after the transposes and clones, whose consumers run on the library's again."""
    dev_pts = device_out and points_device
    if device_out:
        import torch
    while True:
        bufs = []
        for _ in range(g):
            desc = (torch.empty((cap, width), dtype=getattr(torch, np.dtype(dtype).name), device="cuda") if device_out
                    else np.zeros((cap, width), dtype))
            loc = torch.empty((2, cap), dtype=torch.float64, device="cuda") if dev_pts else np.zeros((2, cap), np.float64)
            bufs.append((desc, loc, np.zeros((cap, 4), np.float32) if want_aux else None))
        if device_out:
            _fence_fresh_blocks()
        rc, counts = call(bufs, cap)
        if rc == _capi.APS_E_CAP and retry(counts, cap):
            cap = max(counts)
            continue
        check(rc)
        break
    if device_out:
        check(lib.aps_synchronize())  # (with every output resident the call returns without waiting for its last kernel)
    out = []
    for (desc, loc, aux), n in zip(bufs, counts):
        pts = loc[:, :n].t().contiguous() if dev_pts else np.ascontiguousarray(loc[:, :n].T)
        # Resident output: the first n rows of the capacity buffer, as a view.  (Until round 4 a right-sized clone was handed
        # back so that the worst-case buffer - H*W/64 rows = 66 MB for a 4K view - could be freed: a 10 MB device copy per view
        # on torch's stream plus a stream synchronisation, 23 us of a chip-filling copy kernel and the host wait, to save
        # 64 x 56 MB = 3.6 GB of a 288 GB device for the length of one step.)
        if device_out:
            d = desc[:n].clone() if compact else desc[:n]
        else:
            d = np.ascontiguousarray(desc[:n])
        out.append((d, pts, aux[:n].copy() if want_aux else None))
    if device_out and (dev_pts or compact):
        torch.cuda.current_stream().synchronize()  # the transposes / clones ran on torch's stream; consumers run on the library's
    return out


def _one_view_call(entry, prm, img, h, w, c, ld):
    """call(bufs, cap) of _extract_regrow for the single-image entries (aps_sift_extract and its kin)."""
    cnt = C.c_int64(0)

    def call(bufs, cap):
        desc, loc, aux = bufs[0]
        rc = entry(ptr(img), h, w, c, _capi.APS_IMG_U8_HWC, C.byref(prm), ptr(desc), _capi.APS_ROWMAJOR, ld, ptr(loc), cap,
                   ptr(aux), cap, C.byref(cnt))
        return rc, [int(cnt.value)]

    return call


def _over_capacity(counts, cap):
    """SIFT's retry predicate: some view found more than its buffers hold (maxFeatures is a candidate capacity there, not a row
    limit)."""
    return any(n > cap for n in counts)


def _over_capacity_unless_limited(max_features):
    """SURF's and FAST's retry predicate: some view's count exceeds the capacity and none is the count before a maxFeatures row
    limit."""
    return lambda counts, cap: any(n > cap for n in counts) and not any(0 < max_features < n for n in counts)


def _group_images(images):
    """The image preamble of the group wrappers: ([contiguous uint8 images], h, w, c) of images of one shape (ValueError
    otherwise); an empty list gives a 1 x 1 x 3 shape, which no call uses."""
    prepared = [_image_hwc(im) for im in images]
    imgs = [p[0] for p in prepared]
    if any(tuple(im.shape) != tuple(imgs[0].shape) for im in imgs):
        raise ValueError("the images of a batch must have one shape")
    return (imgs,) + (tuple(prepared[0][1:]) if imgs else (1, 1, 3))


def _group_call(view_struct, entry, prm, imgs, h, w, c, ld):
    """call(bufs, cap) of _extract_regrow for the group entries (aps_sift_extract_batch and its kin): one view record per image,
    all of one capacity, which is also the leading dimension of their column-major locations."""
    g = len(imgs)
    views = (view_struct * max(g, 1))()

    def call(bufs, cap):
        for k, (desc, loc, aux) in enumerate(bufs):
            views[k].img, views[k].desc, views[k].loc, views[k].aux = ptr(imgs[k]), ptr(desc), ptr(loc), ptr(aux)
            views[k].cap, views[k].count = cap, 0
        rc = entry(views, g, h, w, c, _capi.APS_IMG_U8_HWC, C.byref(prm), _capi.APS_ROWMAJOR, ld, cap if g else 0)
        return rc, [int(views[k].count) for k in range(g)]

    return call


def sift_extract(input, image, device_out=False, want_aux=False, points_device=False, compact=False):
    """aps_sift_extract with automatic capacity: returns (features, validPts[, aux]).

    Retained memory of a resident result: with device_out the descriptors come back as a VIEW of the capacity
    buffer (H*W/64 rows: 66 MB for a 4K view, ~6x what ~20 k features need), which stays allocated as long as the caller keeps
    the descriptors.  compact=True returns a right-sized clone instead (one device copy per view); pipeline.sift_many asks for
    it when a call extracts more than 96 views, so that a 256- or 500-view set holds what it uses.

    image: H x W x 3 or H x W uint8, numpy (host) or torch (host/device), row-major.
    device_out=True keeps the descriptors on the GPU (torch float32 [n,128]) for the resident pipeline;
    points_device=True (with device_out) leaves the keypoints there as well (torch float64 [n,2]) instead of bringing
    them to the host - the resident pipeline only ever hands them back to the device (aps_gather_match_points).

    input.NumStrongest (absent by default; cv::SIFT's nfeatures, selectStrongest) keeps at most that many rows through
    aps_sift_extract_strongest: those that come first by (aux[:, 2], the keypoint's contrast, descending; row index ascending), with
    no quota per octave.  The kept rows are rows of the result without the key, bit for bit and in the same order, and the capacity
    buffer of a resident result holds NumStrongest rows, not H*W/64.  A value below 1 is an ApsError (APS_E_ARG).

    input.NumUniform (absent by default; selectUniform) keeps min(N, rows) rows through aps_sift_extract_uniform, spread over the
    cells of the input.UniformGrid = (rows, cols) grid (default (8, 8), each 1..32) on the image by water-filling, the largest
    contrast first within a cell (DESIGN.md "Uniform-N selection").  The kept rows are rows of the result without the key, bit for
    bit and in the same order; a resident result holds NumUniform rows.  Together with NumStrongest it is a ValueError."""
    img, h, w, c = _image_hwc(image)
    prm, entry, cap = _pick_entry(input, _uniform_keys(input), max(4096, (h * w) // 64), (_sift_params(input), lib.aps_sift_extract),
                                  (lambda n: _sift_strongest_params(input, n), lib.aps_sift_extract_strongest),
                                  _capi.aps_sift_uniform_params, lib.aps_sift_extract_uniform)
    d, pts, aux = _extract_regrow(1, cap, _one_view_call(entry, prm, img, h, w, c, DIM), _over_capacity, DIM, np.float32,
                                  device_out, points_device, compact, want_aux)[0]
    return (d, pts, aux) if want_aux else (d, pts)


def sift_extract_batch(input, images, device_out=False, want_aux=False, points_device=False, compact=False):
    """aps_sift_extract_batch with automatic capacity: sift_extract for 1.._capi.APS_SIFT_MAX_VIEWS images of one shape in one call,
    every stage once for the group.  Returns a list of sift_extract's results, one (features, validPts[, aux]) per image, bit for
    bit those of sift_extract(input, image, ...) on each.  The arguments are sift_extract's.

    input.NumStrongest and input.NumUniform (with input.UniformGrid) select per view, as in sift_extract: every view keeps its own
    min(N, rows) rows through aps_sift_extract_batch_strongest / aps_sift_extract_batch_uniform, whose selection is one more stage of
    the group's chain (one sort and one compaction for all the views, no further read-back).  The capacity per view is then
    min(default, max(N, 1)), so a resident result holds N rows per view.  Both keys together are a ValueError, raised before any
    library call; the values themselves are the library's to refuse (APS_E_ARG)."""
    uniform = _uniform_keys(input)
    imgs, h, w, c = _group_images(images)
    prm, entry, cap = _pick_entry(input, uniform, max(4096, (h * w) // 64), (_sift_params(input), lib.aps_sift_extract_batch),
                                  (lambda n: _sift_strongest_params(input, n), lib.aps_sift_extract_batch_strongest),
                                  _capi.aps_sift_uniform_params, lib.aps_sift_extract_batch_uniform)
    out = _extract_regrow(len(imgs), cap, _group_call(_capi.aps_sift_view, entry, prm, imgs, h, w, c, DIM), _over_capacity, DIM,
                          np.float32, device_out, points_device, compact, want_aux)
    return [r if want_aux else r[:2] for r in out]


SURF_DIM = 64


def _surf_params(input):
    p = _capi.aps_surf_params()
    p.metric_threshold = float(input.get("MetricThreshold", 1000.0))
    p.n_octaves = int(input.get("NumOctaves", 8))  # getFeaturePoints.m:55
    p.n_scale_levels = int(input.get("NumScaleLevels", 4))
    p.upright = int(bool(input.get("Upright", False)))  # extractFeatures' Upright; the strongest and uniform structs nest it
    p.max_features = int(input.get("maxFeatures", 0))
    return p


def _surf_strongest_params(input, n=None):
    p = _capi.aps_surf_strongest_params()
    p.surf = _surf_params(input)
    p.n_strongest = int(input["NumStrongest"] if n is None else n)
    return p


def surf_extract(input, image, device_out=False, want_aux=False, points_device=False, compact=False, padded=False):
    """aps_surf_extract with automatic capacity: returns (features, validPts[, aux]); the arguments are sift_extract's.

    Host results are n x 64.  Resident results (device_out=True) are the [:, :64] view of an n x 128 buffer whose columns
    64..127 the library zeroed: the 128-wide matchers take the padded rows behind the view without a copy (_as_desc).
    padded=True (with device_out) returns that n x 128 buffer itself: the form the resident pipeline hands to the matchers and
    the all-gather.  aux: n x 4 [scale, angle_deg, metric, sign_of_laplacian].

    input.NumStrongest (absent by default; selectStrongest) keeps at most that many rows through aps_surf_extract_strongest: those
    that come first by (metric descending, row index ascending), with no quota per octave.  The kept rows are rows of the result
    without the key, in the same order; the capacity buffer of a resident result holds NumStrongest rows.  A value below 1 is an
    ApsError (APS_E_ARG).

    input.NumUniform with input.UniformGrid (sift_extract's keys; selectUniform) keeps min(N, rows) rows through
    aps_surf_extract_uniform, spread over the grid's cells by water-filling, the largest metric first within a cell; a row's cell is
    that of its detection sample, before refinement (DESIGN.md "Uniform-N selection").

    input.Upright (absent or false by default; extractFeatures' Upright) skips the orientation stage on every entry above: the rows
    are described along the image axes, angle_deg is 0, and count, validPts, scale and metric are those of the oriented call."""
    img, h, w, c = _image_hwc(image)
    prm, entry, cap = _pick_entry(input, _uniform_keys(input), max(4096, (h * w) // 64), (_surf_params(input), lib.aps_surf_extract),
                                  (lambda n: _surf_strongest_params(input, n), lib.aps_surf_extract_strongest),
                                  _capi.aps_surf_uniform_params, lib.aps_surf_extract_uniform)
    width = DIM if device_out else SURF_DIM  # (resident rows are 128 wide, host rows 64; the leading dimension follows)
    d, pts, aux = _extract_regrow(1, cap, _one_view_call(entry, prm, img, h, w, c, width),
                                  _over_capacity_unless_limited(int(input.get("maxFeatures", 0))), width, np.float32,
                                  device_out, points_device, compact, want_aux)[0]
    if device_out and not padded:
        d = d[:, :SURF_DIM]
    return (d, pts, aux) if want_aux else (d, pts)


def surf_extract_batch(input, images, device_out=False, want_aux=False, points_device=False, compact=False, padded=False):
    """aps_surf_extract_batch with automatic capacity: surf_extract for 1.._capi.APS_SURF_MAX_VIEWS images of one shape in one call,
    every stage once for the group.  Returns a list of surf_extract's results, one (features, validPts[, aux]) per image, bit for
    bit those of surf_extract(input, image, ...) on each.  The arguments are surf_extract's.

    input.NumStrongest and input.NumUniform (with input.UniformGrid) select per view, as in surf_extract: every view keeps its own
    min(N, rows) rows through aps_surf_extract_batch_strongest / aps_surf_extract_batch_uniform, whose selection is one more stage of
    the group's chain.  The capacity per view is then min(default, max(N, 1)).  Both keys together are a ValueError, raised before
    any library call; the values themselves are the library's to refuse (APS_E_ARG)."""
    uniform = _uniform_keys(input)
    imgs, h, w, c = _group_images(images)
    prm, entry, cap = _pick_entry(input, uniform, max(4096, (h * w) // 64), (_surf_params(input), lib.aps_surf_extract_batch),
                                  (lambda n: _surf_strongest_params(input, n), lib.aps_surf_extract_batch_strongest),
                                  _capi.aps_surf_uniform_params, lib.aps_surf_extract_batch_uniform)
    width = DIM if device_out else SURF_DIM  # (resident rows are 128 wide, host rows 64; the leading dimension follows)
    out = _extract_regrow(len(imgs), cap, _group_call(_capi.aps_surf_view, entry, prm, imgs, h, w, c, width),
                          _over_capacity_unless_limited(int(input.get("maxFeatures", 0))), width, np.float32, device_out,
                          points_device, compact, want_aux)
    if device_out and not padded:
        out = [(d[:, :SURF_DIM], pts, aux) for d, pts, aux in out]
    return [r if want_aux else r[:2] for r in out]


KAZE_DIM = 64
_KAZE_DIFFUSION = {"region": _capi.APS_KAZE_DIFFUSION_REGION, "sharpedge": _capi.APS_KAZE_DIFFUSION_SHARPEDGE,
                   "edge": _capi.APS_KAZE_DIFFUSION_EDGE}


def _kaze_params(input):
    """detectKAZEFeatures' defaults; a Diffusion the library does not build is a ValueError here, before any library call."""
    diffusion = str(input.get("Diffusion", "region"))
    if diffusion not in _KAZE_DIFFUSION:
        raise ValueError(f"Diffusion must be 'region', 'sharpedge' or 'edge', not {diffusion!r}")
    if diffusion != "region":
        raise ValueError(f"Diffusion = {diffusion!r} is not built (it needs exp on the device); only 'region' is")
    p = _capi.aps_kaze_params()
    p.threshold = float(input.get("Threshold", 0.0001))
    p.num_octaves = int(input.get("NumOctaves", 3))
    p.num_scale_levels = int(input.get("NumScaleLevels", 4))
    p.diffusion = _KAZE_DIFFUSION[diffusion]
    p.max_features = int(input.get("maxFeatures", 0))
    return p


def _kaze_select_params(input, kaze, uniform):
    """aps_kaze_select_params around kaze_extract's params: the selection that NumStrongest or NumUniform (uniform: what
    _uniform_keys(input) returned) asks for, and Upright."""
    p = _capi.aps_kaze_select_params()
    p.kaze = kaze
    if uniform:
        p.select, p.n_select, p.grid_rows, p.grid_cols = 2, *uniform
    elif "NumStrongest" in input:
        p.select, p.n_select = 1, int(input["NumStrongest"])
    p.upright = int(bool(input.get("Upright", False)))
    return p


def kaze_extract(input, image, device_out=False, want_aux=False, points_device=False, compact=False, padded=False):
    """aps_kaze_extract with automatic capacity: returns (features, validPts[, aux]); the arguments are surf_extract's.

    Keys of `input`, all optional: Threshold (0.0001), NumOctaves (3, 1..4), NumScaleLevels (4, 3..10), Diffusion ('region'; the
    other two are a ValueError), maxFeatures.  Host results are n x 64 unit-norm oriented M-SURF rows.  Resident results
    (device_out=True) are the [:, :64] view of an n x 128 buffer whose columns 64..127 the library zeroed, or with padded=True that
    buffer itself, as surf_extract's.  validPts: n x 2 float64 [x y] 1-based.  aux: n x 4 [scale, angle_deg, metric, level].
    There is no group form (DESIGN.md "KAZE contract").

    Four more keys, all absent by default, go through aps_kaze_extract_select (DESIGN.md "KAZE selection and Upright"); without
    any of them the call is aps_kaze_extract.
    input.NumStrongest (selectStrongest) keeps at most that many rows: those that come first by (metric descending, row index
    ascending), in one group with no quota per level.  input.NumUniform with input.UniformGrid = (rows, cols) (default (8, 8), each
    1..32; selectUniform) keeps min(N, rows) rows spread over the grid's cells by water-filling, the largest metric first within a
    cell; a row's cell is that of its detection pixel, before refinement.  Either way the kept rows are rows of the result without
    the key, bit for bit and in the same order, and the capacity buffer of a resident result holds N rows.  Both keys together are
    a ValueError, raised before any library call; a value below 1 or a grid value outside 1..32 is an ApsError (APS_E_ARG).
    input.Upright (extractFeatures' Upright) skips the orientation: the rows are described along the image axes, angle_deg is 0,
    and count, validPts, scale, metric and level are those of the oriented call.  It combines with either selection."""
    uniform = _uniform_keys(input)
    img, h, w, c = _image_hwc(image)
    prm, entry, cap = _kaze_params(input), lib.aps_kaze_extract, max(4096, (h * w) // 64)
    if any(k in input for k in ("NumStrongest", "NumUniform", "UniformGrid", "Upright")):
        prm, entry = _kaze_select_params(input, prm, uniform), lib.aps_kaze_extract_select
        if prm.select:  # (as _pick_entry: a resident result holds N rows)
            cap = min(cap, max(prm.n_select, 1))
    width = DIM if device_out else KAZE_DIM  # (resident rows are 128 wide, host rows 64; the leading dimension follows)
    d, pts, aux = _extract_regrow(1, cap, _one_view_call(entry, prm, img, h, w, c, width),
                                  _over_capacity_unless_limited(int(input.get("maxFeatures", 0))), width, np.float32,
                                  device_out, points_device, compact, want_aux)[0]
    if device_out and not padded:
        d = d[:, :KAZE_DIM]
    return (d, pts, aux) if want_aux else (d, pts)


FREAK_BYTES = 64
ORB_BYTES = 32


def _descriptor_method(input):
    """input.DescriptorMethod (extractFeatures' Method) of detector = 'FAST': 'FREAK' (the default when the key is absent) or 'ORB';
    anything else is a ValueError, raised before any library call."""
    method = input.get("DescriptorMethod", "FREAK")
    if method not in ("FREAK", "ORB"):
        raise ValueError(f"input.DescriptorMethod must be 'FREAK' or 'ORB', not {method!r}")
    return method


def _corner_method(input):
    """input.CornerMethod of detector = 'FAST': 'FAST' (the default when the key is absent; detectFASTFeatures) or 'Harris'
    (detectHarrisFeatures: the dense integer Harris detector, DESIGN.md "Harris corner contract"); anything else is a ValueError,
    raised before any library call."""
    method = input.get("CornerMethod", "FAST")
    if method not in ("FAST", "Harris"):
        raise ValueError(f"input.CornerMethod must be 'FAST' or 'Harris', not {method!r}")
    return method


def _corner_params(input, n_levels, uniform, method):
    """aps_corner_params of CornerMethod = 'Harris': fast_extract's keys, with detectHarrisFeatures' MinQuality default of 0.01.
    MinContrast is not read by the detector; the threshold field carries 0."""
    p = _capi.aps_corner_params()
    p.chain = _fast_orb_params({**input, "MinContrast": 0.0, "MinQuality": input.get("MinQuality", 0.01)}, n_levels, uniform)
    p.corner = _capi.APS_CORNER_HARRIS
    p.descriptor = _capi.APS_DESC_ORB if method == "ORB" else _capi.APS_DESC_FREAK
    return p


def _fast_params(input):
    p = _capi.aps_fast_params()
    p.threshold = int(np.floor(float(input.get("MinContrast", 0.2)) * 255))  # detectFASTFeatures: MinContrast 0.2
    p.quality_num, p.quality_den = int(round(float(input.get("MinQuality", 0.1)) * 1000000)), 1000000
    p.max_features = int(input.get("maxFeatures", 0))
    return p


def _fast_pyramid_params(input, n_levels):
    p = _capi.aps_fast_pyramid_params()
    p.fast = _fast_params(input)
    p.n_levels = n_levels
    p.scale_num, p.scale_den = int(round(float(input.get("ScaleFactor", 1.2)) * 1000000)), 1000000
    return p


def _fast_strongest_params(input, n_levels, n=None):
    p = _capi.aps_fast_strongest_params()
    p.pyramid = _fast_pyramid_params(input, n_levels)
    p.n_strongest = int(input["NumStrongest"] if n is None else n)
    return p


def _fast_plan_pixels(h, w, pyramid):
    """The pixels of all levels of aps_fast_pyramid_plan's plan for an h x w image: what the first capacity is sized by."""
    hs, ws, used = (C.c_int * 16)(), (C.c_int * 16)(), C.c_int(0)
    check(lib.aps_fast_pyramid_plan(h, w, pyramid.n_levels, pyramid.scale_num, pyramid.scale_den, hs, ws, C.byref(used)))
    return sum(hs[l] * ws[l] for l in range(used.value))


def _fast_orb_params(input, n_levels, uniform):
    """aps_fast_orb_params of fast_extract's keys: the pyramid, and the selection that NumStrongest or NumUniform asks for."""
    p = _capi.aps_fast_orb_params()
    p.pyramid = _fast_pyramid_params(input, n_levels)
    if uniform:
        p.select, p.n_select, p.grid_rows, p.grid_cols = 2, *uniform
    elif "NumStrongest" in input:
        p.select, p.n_select = 1, int(input["NumStrongest"])
    return p


def fast_extract(input, image, device_out=False, want_aux=False, points_device=False, compact=False):
    """aps_fast_extract with automatic capacity: returns (binaryFeatures, validPts[, aux]); the arguments are sift_extract's.
    Features are n x 64 uint8 (FREAK, 512 bits), on the host or, with device_out, resident; validPts n x 2 [x y] 1-based,
    integer-valued; aux n x 4 [FAST score, orientation bin, 0, 0].  input.MinContrast (0.2) and input.MinQuality (0.1) are
    detectFASTFeatures' parameters.

    input.NumLevels (1) and input.ScaleFactor (1.2), detectORBFeatures' names, ask for a scale pyramid: NumLevels > 1 goes
    through aps_fast_extract_pyramid, which runs FAST/FREAK on every level of the plan.  validPts are then the level pixels'
    centres in image coordinates (not integers beyond level 0), aux is [score, bin, level, 0], and the rows are in ascending
    (level, row, col) order; a corner may be reported at several levels.

    input.NumStrongest (absent by default; detectORBFeatures' nfeatures, selectStrongest) keeps at most that many rows, for any
    NumLevels, through aps_fast_extract_strongest: a quota per level in proportion to h_l + w_l, and within a level the rows
    with the largest integer Harris response.  The kept rows are rows of the result without the key, in the same order;
    aux is [score, bin, level, f32(R)].  A value below 1 is an ApsError (APS_E_ARG).

    input.NumUniform with input.UniformGrid (sift_extract's keys; selectUniform) keeps the same number of rows per level as
    NumStrongest = N does, through aps_fast_extract_uniform, but spreads each level's rows over the cells of the grid on the level's
    plane by water-filling, the largest Harris response first within a cell (DESIGN.md "Uniform-N selection"); aux as above.

    input.DescriptorMethod = 'ORB' (extractFeatures' Method; absent or 'FREAK': the above) describes the same rows - count, validPts,
    score, level and f32(R) are bit for bit those of the FREAK call with the same keys - with ORB's intensity-centroid orientation
    and steered BRIEF descriptor through aps_fast_orb_extract (DESIGN.md "FAST/ORB contract"): Features are n x 32 uint8 (256 bits)
    and aux[:, 1] is the ORB bin.  Any other value is a ValueError.

    input.CornerMethod = 'Harris' (absent or 'FAST': the above, through the same entries) replaces the detector alone, through
    aps_corner_extract (DESIGN.md "Harris corner contract"): on every level the integer Harris response at every pixel, strict 3 x 3
    suppression, and the gate R >= MinQuality * Rmax of the level, MinQuality defaulting to detectHarrisFeatures' 0.01; MinContrast
    is ignored.  Every other key keeps its meaning; aux is [f32(R), bin, level, f32(R) with a selection else 0].  Any other value
    is a ValueError."""
    method = _descriptor_method(input)
    harris = _corner_method(input) == "Harris"
    img, h, w, c = _image_hwc(image)
    n_levels = int(input.get("NumLevels", 1))
    uniform = _uniform_keys(input)
    if method == "ORB" or harris:
        nbytes = ORB_BYTES if method == "ORB" else FREAK_BYTES
        prm = _corner_params(input, n_levels, uniform, method) if harris else _fast_orb_params(input, n_levels, uniform)
        chain = prm.chain if harris else prm
        cap = max(4096, _fast_plan_pixels(h, w, chain.pyramid) // 64)
        if chain.select:  # (as _pick_entry: a resident result holds N rows)
            cap = min(cap, max(chain.n_select, 1))
        entry = lib.aps_corner_extract if harris else lib.aps_fast_orb_extract
        d, pts, aux = _extract_regrow(1, cap, _one_view_call(entry, prm, img, h, w, c, nbytes),
                                      _over_capacity_unless_limited(int(input.get("maxFeatures", 0))), nbytes, np.uint8,
                                      device_out, points_device, compact, want_aux)[0]
        f = binaryFeatures(d)
        return (f, pts, aux) if want_aux else (f, pts)
    if n_levels == 1 and "NumStrongest" not in input and not uniform:
        plain, pixels = (_fast_params(input), lib.aps_fast_extract), h * w
    else:
        plain = (_fast_pyramid_params(input, n_levels), lib.aps_fast_extract_pyramid)
        pixels = _fast_plan_pixels(h, w, plain[0])
    prm, entry, cap = _pick_entry(input, uniform, max(4096, pixels // 64), plain,
                                  (lambda n: _fast_strongest_params(input, n_levels, n), lib.aps_fast_extract_strongest),
                                  _capi.aps_fast_uniform_params, lib.aps_fast_extract_uniform)
    d, pts, aux = _extract_regrow(1, cap, _one_view_call(entry, prm, img, h, w, c, FREAK_BYTES),
                                  _over_capacity_unless_limited(int(input.get("maxFeatures", 0))), FREAK_BYTES, np.uint8,
                                  device_out, points_device, compact, want_aux)[0]
    f = binaryFeatures(d)
    return (f, pts, aux) if want_aux else (f, pts)


def fast_extract_batch(input, images, device_out=False, want_aux=False, points_device=False, compact=False):
    """aps_fast_extract_batch with automatic capacity: fast_extract for 1.._capi.APS_FAST_MAX_VIEWS images of one shape in one call,
    every stage once for the group, for any input.NumLevels.  Returns a list of fast_extract's results, one (binaryFeatures,
    validPts[, aux]) per image, byte for byte those of fast_extract(input, image, ...) on each (aux is [score, bin, level, 0], also
    with NumLevels = 1, where the level is 0).  The arguments are fast_extract's.

    input.NumStrongest and input.NumUniform have no group form - a FAST selection group is a level, and a group of views would need
    views x levels of them: with either key this is a ValueError; call fast_extract per view.

    input.DescriptorMethod = 'ORB' goes through aps_fast_orb_extract_batch: rows of 32 bytes, as fast_extract's.
    input.CornerMethod = 'Harris' goes through aps_corner_extract_batch, with either descriptor."""
    if "NumStrongest" in input or "NumUniform" in input:
        raise ValueError("fast_extract_batch takes no input.NumStrongest / input.NumUniform: call fast_extract per view")
    method = _descriptor_method(input)
    harris = _corner_method(input) == "Harris"
    entry, nbytes = ((lib.aps_fast_orb_extract_batch, ORB_BYTES) if method == "ORB" else (lib.aps_fast_extract_batch, FREAK_BYTES))
    imgs, h, w, c = _group_images(images)
    prm = _fast_pyramid_params(input, int(input.get("NumLevels", 1)))
    cap = max(4096, _fast_plan_pixels(h, w, prm) // 64)  # (no selection key: nothing for _pick_entry to pick)
    if harris:
        entry, prm = lib.aps_corner_extract_batch, _corner_params(input, prm.n_levels, None, method)
    out = _extract_regrow(len(imgs), cap, _group_call(_capi.aps_fast_view, entry, prm, imgs, h, w, c, nbytes),
                          _over_capacity_unless_limited(int(input.get("maxFeatures", 0))), nbytes, np.uint8, device_out,
                          points_device, compact, want_aux)
    return [(binaryFeatures(d), pts, aux) if want_aux else (binaryFeatures(d), pts) for d, pts, aux in out]


def extract_features(input, image, **kw):
    """sift_extract, surf_extract, kaze_extract or fast_extract, as input.detector says (the dispatch of the pipeline's extraction
    stages).  'KAZE' enters here and not through getFeaturePoints, which keeps refusing it."""
    det = input.get("detector", "SIFT")
    if det == "FAST":
        return fast_extract(input, image, **kw)
    if det == "SURF":
        return surf_extract(input, image, padded=bool(kw.get("device_out")), **kw)
    if det == "KAZE":
        return kaze_extract(input, image, padded=bool(kw.get("device_out")), **kw)
    if det == "SIFT":
        return sift_extract(input, image, **kw)
    return getFeaturePoints(input, image)  # raises for the rest of the switch


def getFeaturePoints(input, ImageOriginal):
    """[features, validPts] = getFeaturePoints(input, ImageOriginal) (getFeaturePoints.m:1-76) for
    input.detector == 'SIFT' (features Kf x 128 single, unit norm), 'SURF' (Kf x 64 single, unit norm; :54-55) and 'FAST'
    (binaryFeatures, Kf x 64 uint8 FREAK, or Kf x 32 uint8 ORB with input.DescriptorMethod = 'ORB'; :51-52); validPts Kf x 2 double
    [x y] 1-based.
    The other detectors of the switch (:33-68) are toolbox calls with no device counterpart here."""
    det = input.get("detector", "SIFT")
    if det == "SURF":
        return surf_extract(input, ImageOriginal)
    if det == "FAST":
        return fast_extract(input, ImageOriginal)
    if det != "SIFT":
        if det in ("vl_SIFT", "HARRIS", "BRISK", "ORB", "KAZE"):
            raise NotImplementedError(f"detector '{det}' is a MATLAB toolbox/VLFeat call; only 'SIFT', 'SURF' and 'FAST' run on the device")
        raise ValueError("Need a valid input!")  # getFeaturePoints.m:67
    return sift_extract(input, ImageOriginal)


# ---- global matcher (featureMatchingGlobal.m) and the mex contracts it calls ------------------------
def flann_knn_win(train, query, k, method="flann", trees=4, checks=32):
    """[idx, dist] = flann_knn_win(train, query, k, 'flann' | 'bf', trees, checks) (PP/mex/flann_knn.cpp:118-253) for
    float (single) and binary (uint8) descriptors, computed EXACTLY on the device (the reference's kd-forest is approximate and
    seed-dependent; `trees`/`checks` are accepted and ignored).  idx: Fq x k uint32 1-based, dist: Fq x k
    single squared-L2, ascending."""
    if k != int(k) or k <= 0:
        raise ValueError("k must be > 0")  # flann_knn:k
    tr = train if _capi.is_torch(train) else np.asarray(train)
    if str(tr.dtype).endswith("uint8"):
        # binary descriptors (flann_knn.cpp:199-223 'bf' = BFMatcher knnMatch; :235-240 'flann' = LSH index): ONE exact
        # brute-force Hamming k-NN serves both; dist = Hamming distance as single, ascending, ties -> lower index
        T = np.ascontiguousarray(train, np.uint8)
        Q = np.ascontiguousarray(query, np.uint8)
        if T.ndim != 2 or Q.ndim != 2:
            raise ValueError("train must be 2-D")  # flann_knn:dim (checkReal2D)
        if T.shape[1] != Q.shape[1]:
            raise ValueError("query must have same descriptor dimension as train")  # flann_knn:dim
        k = int(k)
        idx = np.zeros((Q.shape[0], k), np.uint32)
        dist = np.zeros((Q.shape[0], k), np.float32)
        check(lib.aps_knn_hamming(ptr(T), T.shape[0], T.shape[1], ptr(Q), Q.shape[0], Q.shape[1], T.shape[1],
                                  _capi.APS_ROWMAJOR, k, ptr(idx), ptr(dist), k))
        return idx, dist
    if str(method) == "bf":
        raise ValueError("BFMatcher only supports uint8 (binary) descriptors")  # flann_knn:bf
    T, ft, ldt, lt = _as_desc(train)
    Q, fq, ldq, lq = _as_desc(query)
    if (ft and T.shape[1] != DIM) or (fq and Q.shape[1] != DIM) or lt != lq:
        raise ValueError("query must have same descriptor dimension as train")  # flann_knn:dim
    k = int(k)
    idx = np.zeros((fq, k), np.uint32)
    dist = np.zeros((fq, k), np.float32)
    check(lib.aps_knn_global(ptr(T), ft, ldt, ptr(Q), fq, ldq, DIM, lt, k, ptr(idx), ptr(dist), k))
    return idx, dist


def nearest2HammingExhaustiveMEX(Abytes, Bbytes):
    """[idx2, d1, d2] = nearest2HammingExhaustiveMEX(Abytes, Bbytes) (PP/mex/nearest2HammingExhaustiveMEX.cpp)."""
    A = np.ascontiguousarray(Abytes)
    B = np.ascontiguousarray(Bbytes)
    if A.dtype != np.uint8 or B.dtype != np.uint8:
        raise TypeError("Inputs must be uint8.")  # hamm2nn:type
    if A.ndim != 2 or B.ndim != 2:
        raise ValueError("2D only.")  # hamm2nn:dim
    if A.shape[1] != B.shape[1]:
        raise ValueError("Byte width mismatch.")  # hamm2nn:cols
    n1 = A.shape[0]
    idx2 = np.zeros(n1, np.uint32)
    d1 = np.zeros(n1, np.float32)
    d2 = np.zeros(n1, np.float32)
    check(lib.aps_hamming_2nn(ptr(A), n1, A.shape[1], ptr(B), B.shape[0], B.shape[1], A.shape[1],
                              _capi.APS_ROWMAJOR, ptr(idx2), ptr(d1), ptr(d2)))
    return idx2, d1, d2


nearest2HammingExhaustiveOMPMEX = nearest2HammingExhaustiveMEX  # same arithmetic (OMP twin)


def match_global_csr(allDescriptors, ratio=0.6, k=4, device_out=False):
    """featureMatchingGlobal.m:69-161 in CSR form, resident when the descriptors are: pool (torch.cat / concatenate),
    row normalisation with eps inside the root (:83-85, aps_global_normalize), exact k-NN of the pool against itself
    (aps_knn_global: blocked f16-screened search with exact distances), per-query filter (aps_global_filter).
    Returns (pair_ptr int64[P+1] in featureMatchingPairwise's pair order, idx_i, idx_j): 1-based local indices in the
    lower- / higher-numbered image of each pair, query order; device_out=True keeps idx_i/idx_j as int32 CUDA tensors."""
    numImg = len(allDescriptors)
    allDescriptors = [_pad_rows(d) for d in allDescriptors]
    counts = [int(d.shape[0]) for d in allDescriptors]
    F = sum(counts)
    npairs = numImg * (numImg - 1) // 2
    pair_ptr = np.zeros(npairs + 1, np.int64)
    resident = F > 0 and all(_capi.is_torch(d) and d.is_cuda for d in allDescriptors)
    if F == 0:
        z = np.zeros(0, np.uint32)
        return pair_ptr, z, z.copy()
    img_idx = np.repeat(np.arange(1, numImg + 1, dtype=np.uint32), counts)
    local_idx = np.concatenate([np.arange(1, c + 1, dtype=np.uint32) for c in counts])
    if resident:
        import torch

        raw = torch.cat([d.reshape(-1, DIM) for d in allDescriptors]).contiguous()
        torch.cuda.current_stream().synchronize()  # torch produced the pool; the library reads it on its own stream
        pool = torch.empty_like(raw)
        nn_idx = torch.empty((F, k), dtype=torch.int32, device=raw.device)
        nn_dist = torch.empty((F, k), dtype=torch.float32, device=raw.device)
        oi = torch.empty(F, dtype=torch.int32, device=raw.device)
        oj = torch.empty(F, dtype=torch.int32, device=raw.device)
    else:
        raw = np.ascontiguousarray(np.concatenate([np.asarray(d.cpu() if _capi.is_torch(d) else d, np.float32).reshape(-1, DIM)
                                                   for d in allDescriptors]))
        pool = np.empty_like(raw)
        nn_idx = np.zeros((F, k), np.uint32)
        nn_dist = np.zeros((F, k), np.float32)
        oi = np.zeros(F, np.uint32)
        oj = np.zeros(F, np.uint32)
    check(lib.aps_global_normalize(ptr(raw), F, DIM, DIM, _capi.APS_ROWMAJOR, ptr(pool)))
    if k <= 4:
        # the search with the filter in view: queries that featureMatchingGlobal.m:129-147 provably drops at this ratio are
        # not searched (they come back as copies of themselves, which the filter removes as self matches); every other
        # query gets its exact k nearest - the CSR lists equal those of the plain search
        img_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        check(lib.aps_knn_global_screened(ptr(pool), F, DIM, DIM, _capi.APS_ROWMAJOR, ptr(img_off), numImg, float(ratio), k,
                                          ptr(nn_idx), ptr(nn_dist), k))
    else:
        check(lib.aps_knn_global(ptr(pool), F, DIM, ptr(pool), F, DIM, DIM, _capi.APS_ROWMAJOR, k, ptr(nn_idx), ptr(nn_dist), k))
    cnt = C.c_int64(0)
    check(lib.aps_global_filter(ptr(nn_idx), ptr(nn_dist), F, k, k, _capi.APS_ROWMAJOR, ptr(img_idx), ptr(local_idx),
                                numImg, float(ratio), ptr(pair_ptr), ptr(oi), ptr(oj), F, C.byref(cnt)))
    n = cnt.value
    if resident and not device_out:
        return pair_ptr, oi[:n].cpu().numpy().astype(np.uint32), oj[:n].cpu().numpy().astype(np.uint32)
    return pair_ptr, oi[:n], oj[:n]


def match_global_binary_csr(allDescriptors, ratio=0.6, k=4, method="flann"):
    """The isBinary branch of featureMatchingGlobal.m:54-161 in CSR form: the sets' bytes pooled (:70-74, 85), exact Hamming
    k-NN of the pool against itself through flann_knn_win ('bf' or 'flann' as input.BFMatch says: one exact device search
    serves both, :110-118), then the per-query filter of :123-161 (aps_global_filter) on the Hamming distances.
    Returns (pair_ptr, idx_i, idx_j) as match_global_csr does, on the host.  Every set has to be binaryFeatures: a list that
    mixes them with float matrices raises TypeError, as the pairwise branch does."""
    numImg = len(allDescriptors)
    if not all(isinstance(d, binaryFeatures) for d in allDescriptors):
        raise TypeError("all sets must be binaryFeatures")
    sets = [np.asarray(d.Features.cpu() if _capi.is_torch(d.Features) else d.Features, np.uint8) for d in allDescriptors]
    counts = [int(f.shape[0]) for f in sets]
    F = sum(counts)
    pair_ptr = np.zeros(numImg * (numImg - 1) // 2 + 1, np.int64)
    if F == 0:
        z = np.zeros(0, np.uint32)
        return pair_ptr, z, z.copy()
    pool = np.ascontiguousarray(np.concatenate([f for f in sets if f.shape[0]]))
    nn_idx, nn_dist = flann_knn_win(pool, pool, k, method)
    img_idx = np.repeat(np.arange(1, numImg + 1, dtype=np.uint32), counts)
    local_idx = np.concatenate([np.arange(1, c + 1, dtype=np.uint32) for c in counts])
    oi = np.zeros(F, np.uint32)
    oj = np.zeros(F, np.uint32)
    cnt = C.c_int64(0)
    check(lib.aps_global_filter(ptr(nn_idx), ptr(nn_dist), F, k, k, _capi.APS_ROWMAJOR, ptr(img_idx), ptr(local_idx),
                                numImg, float(ratio), ptr(pair_ptr), ptr(oi), ptr(oj), F, C.byref(cnt)))
    n = cnt.value
    return pair_ptr, oi[:n], oj[:n]


def featureMatchingGlobal(input, allDescriptors, numImg):
    """matches = featureMatchingGlobal(input, allDescriptors, numImg) (featureMatchingGlobal.m:1-161): pool all
    descriptors, L2-normalise (:80-86), exact kNN (k = input.k) of the pool against itself, per-query filter
    (drop self / same image, need >= 2, ratio on squared L2), append to the upper-triangular cell in query order."""
    numImg = int(numImg)
    counts = [len(d) for d in allDescriptors]
    matches = [[None] * numImg for _ in range(numImg)]
    F = sum(counts)
    if F == 0:
        return matches
    if any(isinstance(d, binaryFeatures) for d in allDescriptors):  # :54-56
        pair_ptr, oi, oj = match_global_binary_csr(allDescriptors, float(input.get("Ratiothreshold", 0.6)), int(input.get("k", 4)),
                                                   "bf" if input.get("BFMatch") else "flann")
    else:
        pair_ptr, oi, oj = match_global_csr(allDescriptors, float(input.get("Ratiothreshold", 0.6)), int(input.get("k", 4)))
    for p, (i, j) in enumerate(pair_order(numImg)):
        s, e = pair_ptr[p], pair_ptr[p + 1]
        if e > s:
            matches[i][j] = np.stack([oi[s:e], oj[s:e]], axis=1).astype(np.float64)
    return matches


def keypoint_marks(points, scales=None, angles_deg=None, color=(0, 255, 0), markerRadius=3, lineWidth=1):
    """The marks of a keypoint plot ("Mark contract"): one ring per keypoint, of radius scales[k] when given and
    markerRadius otherwise; with angles_deg, after all rings, one segment per keypoint from its centre to
    centre + radius * (cos a, -sin a), a = deg2rad(angles_deg[k]) (counter-clockwise on the screen, y pointing down), computed
    here in f64.  points: n x 2 (x, y), 1-based; the columns of a detector's aux array differ, so the caller picks them."""
    from . import imageProcessing as ip

    pts = np.asarray(points.detach().cpu() if _capi.is_torch(points) else points, np.float64).reshape(-1, 2)
    host = lambda v: np.asarray(v.detach().cpu() if _capi.is_torch(v) else v, np.float64).reshape(-1)  # noqa: E731
    radii = np.full(len(pts), float(markerRadius)) if scales is None else host(scales)
    if len(radii) != len(pts):
        raise ValueError("scales must have one entry per keypoint")
    marks = [ip.mark_rings(pts, radii, color, lineWidth)]
    if angles_deg is not None:
        a = np.deg2rad(host(angles_deg))
        if len(a) != len(pts):
            raise ValueError("angles_deg must have one entry per keypoint")
        tips = pts + radii[:, None] * np.stack([np.cos(a), -np.sin(a)], axis=1)
        marks.append(ip.mark_segments(pts, tips, color, lineWidth))
    return np.concatenate(marks)


def showKeypoints(image, points, scales=None, angles_deg=None, color=(0, 255, 0), markerRadius=3, lineWidth=1):
    """The keypoints drawn on a copy of image (ip.draw_marks of keypoint_marks): a ring per keypoint and, with angles_deg, its
    orientation as a radius.  Rings above 4096 px, and keypoints with a non-finite coordinate, scale or angle, are skipped by
    the mark contract.  Returns the drawn image, of the kind of `image` (resident when it is)."""
    from . import imageProcessing as ip

    return ip.draw_marks(image, keypoint_marks(points, scales, angles_deg, color, markerRadius, lineWidth))[0]
