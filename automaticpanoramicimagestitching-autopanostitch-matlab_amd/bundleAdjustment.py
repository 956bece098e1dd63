"""Host-side mirror of the normal-equation accumulation of PP/bundleAdjustment/bundleAdjustmentRKf.m
(SURVEY.md section 8(f) rank 3).

The per-pair blocks - the reference's `parfor p = 1:numel(pairList)` body (:717-741) - run on the device through
`aps_ba_pair_blocks`; what stays here is the bookkeeping around it, restated from the reference: buildDeltaVector
(:1360-1405), applyIncrements (:1407-1501), the pair list of accumulateNormalEqnsBlock (:680-708) and its serial
reduction into H and g (:743-789).

Below them, the camera estimation the reference runs when the intrinsics are unknown, restated from
initializeCameraMatrices.m (focal estimation, maximum spanning tree, rotation chaining, rotation consistency, chained
homographies) and bundleAdjustmentRKf.m (incremental Brown-Lowe driver, Levenberg-Marquardt loop, prior, step caps,
match subsampling).  The LM loop takes its normal-equation evaluator as an argument: DeviceEvaluator (a resident
BaProblem: blocks and assembly on the device, bit-identical to the host reduction) in production, HostEvaluator
(accumulateNormalEqnsBlock with any block function) for the CPU tests.  The prior and the solve stay on the host (they
are O(P^2..P^3) in the camera count, not in the match count).

Planar sets are refined by bundleAdjustmentH.m (joint LM over the absolute homographies, opt-in through
input['planarBundleAdjustment']): its data term runs on the same resident problem (aps_ba_h_normal_eqns, DeviceEvaluatorH),
hNormalEqnsMirror restates it bit for bit in numpy (HostEvaluatorH), and adaptiveLM, the RegProj rows and the solve stay
here."""
from __future__ import annotations

import numpy as np

from ._capi import check, lib, ptr


def skewSymmetric(v):
    v = np.asarray(v, np.float64).reshape(3)
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def buildDeltaVector(cameras, camList, seed):
    """[Phi, pmap] = buildDeltaVector(cameras, camList, seed): one parameter (df) for the seed camera, four
    ([dthx dthy dthz df]) for every other camera; indices 0-based here."""
    pmap, idx = [], 0
    for i in camList:
        is_seed = i == seed
        pmap.append({"camIdx": i, "startIdx": idx, "isSeed": is_seed})
        idx += 1 if is_seed else 4
    return np.zeros(idx, np.float64), pmap


def _cxcy(cam):
    if cam.get("cx") is not None:
        return float(cam["cx"]), float(cam["cy"])
    if cam.get("K") is not None:
        return float(cam["K"][0, 2]), float(cam["K"][1, 2])
    return 0.0, 0.0


def applyIncrements(cameras, Phi, pmap):
    """camsOut = applyIncrements(cameras, Phi, pmap, ...) (:1407-1501): R <- exp([dth]x) R (Rodrigues, first order
    below 1e-12), f <- clamp(f + df, 100, 5000) when it moves by more than 1e-9."""
    out = [None if c is None else dict(c) for c in cameras]
    for e in pmap:
        i, s = e["camIdx"], e["startIdx"]
        cam = out[i]
        cam["cx"], cam["cy"] = _cxcy(cam)
        if e["isSeed"]:
            df = Phi[s]
        else:
            dth = np.asarray(Phi[s:s + 3], np.float64)
            df = Phi[s + 3]
            a = float(np.sqrt(np.sum(dth * dth)))
            if a < 1e-12:
                Rupd = np.eye(3) + skewSymmetric(dth)
            else:
                K = skewSymmetric(dth / a)
                Rupd = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
            cam["R"] = Rupd @ np.asarray(cam["R"], np.float64)
        oldf = float(cam["f"])
        f = max(100.0, min(5000.0, oldf + float(df)))
        if abs(f - oldf) > 1e-9:
            cam["f"] = f
            Ki = np.eye(3) if cam.get("K") is None else np.array(cam["K"], np.float64)
            Ki[0, 0] = Ki[1, 1] = f
            cam["K"] = Ki
    return out


def _pack_cam(cam):
    cx, cy = _cxcy(cam)
    return np.concatenate([[float(cam["f"]), cx, cy], np.asarray(cam["R"], np.float64).reshape(3, 3).ravel(order="F")])


def ba_pair_blocks(Ui, Uj, pair_ptr, cams, sigmaHuber, both=True):
    """The device call: (n_pairs, 59) = Hii, Hjj, Hij (4 x 4 column-major), gi, gj, E, r2sum, rcnt per pair."""
    Ui = np.asfortranarray(np.asarray(Ui, np.float64).reshape(-1, 2))
    Uj = np.asfortranarray(np.asarray(Uj, np.float64).reshape(-1, 2))
    pp = np.ascontiguousarray(pair_ptr, np.int64)
    cc = np.ascontiguousarray(cams, np.float64)
    n = len(pp) - 1
    if cc.shape != (n, 4, 12):
        raise ValueError("cams must be (n_pairs, 4, 12)")
    out = np.zeros((n, 59), np.float64)
    check(lib.aps_ba_pair_blocks(ptr(Ui), ptr(Uj), Ui.shape[0], ptr(pp), n, ptr(cc), float(sigmaHuber), int(bool(both)),
                                 ptr(out)))
    return out


def accumulateNormalEqnsBlock(Phi, pmap, baseCams, camList, seed, matches, keypoints, imageSizes, sigmaHuber, opts=None,
                              blocks=ba_pair_blocks):
    """[H, g, E, rmse] = accumulateNormalEqnsBlock(...) (:609-791).  `matches[i][j]` (i < j) is an M x 2 array of
    1-based keypoint indices as in the reference (None/empty when there is no edge); cameras are dicts with f, R and K
    or cx/cy; indices are 0-based.  opts.MaxMatches subsampling (:1047-1358) is the caller's: pass the subsampled
    matches.  H is returned dense (P x P, P <= 4 N)."""
    opts = opts or {}
    if opts.get("MaxMatches") is not None and np.isfinite(opts["MaxMatches"]):
        raise NotImplementedError("subsample the matches before the call (subsampleMatches is host-side bookkeeping)")
    camLin = applyIncrements(baseCams, Phi, pmap)
    last = pmap[-1]
    P = last["startIdx"] + (1 if last["isSeed"] else 4)
    cols = {e["camIdx"]: (np.arange(e["startIdx"], e["startIdx"] + (1 if e["isSeed"] else 4))) for e in pmap}
    pairs, Ui, Uj, ptrs, cams = [], [], [], [0], []
    for a, i in enumerate(camList):
        for j in camList[a + 1:]:
            mp = matches[i][j] if matches[i] is not None else None
            if mp is None or len(mp) == 0:
                continue
            mp = np.asarray(mp, np.int64)
            Ui.append(np.asarray(keypoints[i], np.float64)[mp[:, 0] - 1])
            Uj.append(np.asarray(keypoints[j], np.float64)[mp[:, 1] - 1])
            ptrs.append(ptrs[-1] + len(mp))
            cams.append(np.stack([_pack_cam(baseCams[i]), _pack_cam(baseCams[j]), _pack_cam(camLin[i]), _pack_cam(camLin[j])]))
            pairs.append((i, j))
    H = np.zeros((P, P), np.float64)
    g = np.zeros(P, np.float64)
    if not pairs:
        return H, g, 0.0, 0.0
    out = blocks(np.concatenate(Ui), np.concatenate(Uj), ptrs, np.stack(cams), sigmaHuber, not opts.get("OneDirection", False))
    E = R2 = cnt = 0.0
    for (i, j), o in zip(pairs, out):  # the serial reduction of :743-785, pair by pair
        bi, bj = cols[i], cols[j]
        Hii = o[0:16].reshape(4, 4, order="F")[:len(bi), :len(bi)]
        Hjj = o[16:32].reshape(4, 4, order="F")[:len(bj), :len(bj)]
        Hij = o[32:48].reshape(4, 4, order="F")[:len(bi), :len(bj)]
        H[np.ix_(bi, bi)] += Hii
        H[np.ix_(bj, bj)] += Hjj
        H[np.ix_(bi, bj)] += Hij
        H[np.ix_(bj, bi)] += Hij.T
        g[bi] += o[48:48 + len(bi)]
        g[bj] += o[52:52 + len(bj)]
        E += o[56]
        R2 += o[57]
        cnt += o[58]
    return H, g, E, float(np.sqrt(max(R2, 0.0) / max(cnt, 1.0)))


# ---- the resident device problem (aps_ba_problem_create / aps_ba_normal_eqns) ----------------------------------------------

def pack_cameras(cameras):
    """n x 12 f64: f, cx, cy, R (column-major) per camera, the layout of the C ABI (zeros for a missing camera)."""
    out = np.zeros((len(cameras), 12), np.float64)
    for k, c in enumerate(cameras):
        if c is not None:
            out[k] = _pack_cam(c)
    return out


class BaProblem:
    """The matched points of every pair of a panorama, uploaded once; normal_eqns evaluates H, g, E and rmse on the
    device (ba.hip: the per-pair blocks, then the assembly in the host mirror's order).  pairs: [(i, j)] 0-based with
    i < j, sorted; Ui / Uj: the pairs' points back to back (pair_ptr delimits them)."""

    def __init__(self, Ui, Uj, pair_ptr, pairs, n_cams):
        import ctypes

        self._Ui = np.asfortranarray(np.asarray(Ui, np.float64).reshape(-1, 2))
        self._Uj = np.asfortranarray(np.asarray(Uj, np.float64).reshape(-1, 2))
        self._ptr = np.ascontiguousarray(pair_ptr, np.int64)
        self._ij = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        self.n_cams = int(n_cams)
        self.n_pairs = len(self._ptr) - 1
        if len(self._ij) != self.n_pairs:
            raise ValueError("one (i, j) per pair")
        h = ctypes.c_void_p()
        check(lib.aps_ba_problem_create(ptr(self._Ui), ptr(self._Uj), max(self._Ui.shape[0], 1), ptr(self._ptr),
                                        ptr(self._ij), self.n_pairs, self.n_cams, ctypes.byref(h)))
        self._h = h

    def normal_eqns(self, base, lin, col_start, n_params, P, sigmaHuber, both=True, want_H=True):
        """(H P x P, g, E, rmse); with want_H=False (H, g) are None (energy-only evaluation)."""
        base = np.ascontiguousarray(base, np.float64)
        lin = np.ascontiguousarray(lin, np.float64)
        cs = np.ascontiguousarray(col_start, np.int32)
        npar = np.ascontiguousarray(n_params, np.int32)
        if base.shape != (self.n_cams, 12) or lin.shape != base.shape or cs.shape != (self.n_cams,) or npar.shape != cs.shape:
            raise ValueError("cameras must be (n_cams, 12), col_start / n_params (n_cams,)")
        H = np.empty((P, P), np.float64, order="F") if want_H else None
        g = np.empty(P, np.float64) if want_H else None
        st = np.zeros(2, np.float64)
        check(lib.aps_ba_normal_eqns(self._h, ptr(base), ptr(lin), ptr(cs), ptr(npar), int(P), float(sigmaHuber),
                                     int(bool(both)), int(bool(want_H)), ptr(H), ptr(g), ptr(st)))
        return H, g, float(st[0]), float(st[1])

    def h_normal_eqns(self, G, seed, huber, want_H=True):
        """The data term of bundleAdjustmentH (aps_ba_h_normal_eqns) at the absolute homographies G (n_cams x 3 x 3 or
        x 9, H(3,3) = 1): (J'J P x P, J'r, stats = [sum (w res)^2, sum |res|^2, match count]), P = 8 (n_cams - 1); with
        want_H=False (H, g) are None."""
        G = np.ascontiguousarray(np.asarray(G, np.float64).reshape(self.n_cams, 9))
        P = 8 * (self.n_cams - 1)
        H = np.empty((P, P), np.float64, order="F") if want_H else None
        g = np.empty(P, np.float64) if want_H else None
        st = np.zeros(3, np.float64)
        check(lib.aps_ba_h_normal_eqns(self._h, ptr(G), self.n_cams, int(seed), float(huber), int(bool(want_H)), ptr(H),
                                       ptr(g), ptr(st)))
        return H, g, st

    def close(self):
        if getattr(self, "_h", None):
            check(lib.aps_ba_problem_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def column_map(pmap, n_cams):
    """(col_start, n_params, P) of a pmap: -1 for the cameras outside camList."""
    cs = np.full(n_cams, -1, np.int32)
    npar = np.zeros(n_cams, np.int32)
    for e in pmap:
        cs[e["camIdx"]] = e["startIdx"]
        npar[e["camIdx"]] = 1 if e["isSeed"] else 4
    return cs, npar, int(npar.sum())


class DeviceEvaluator:
    """The production normal-equation evaluator of runLevenbergMarquardt: a resident BaProblem over the (subsampled)
    matches.  Call signature shared with HostEvaluator: (Phi, pmap, baseCams, camList, seed, sigmaHuber, want_H)."""

    def __init__(self, matches, keypoints, both=True):
        n = len(keypoints)
        pairs, Ui, Uj, ptrs = [], [], [], [0]
        for i in range(n):
            for j in range(i + 1, n):
                mp = matches[i][j] if matches[i] is not None else None
                if mp is None or len(mp) == 0:
                    continue
                mp = np.asarray(mp, np.int64)
                Ui.append(np.asarray(keypoints[i], np.float64)[mp[:, 0] - 1])
                Uj.append(np.asarray(keypoints[j], np.float64)[mp[:, 1] - 1])
                ptrs.append(ptrs[-1] + len(mp))
                pairs.append((i, j))
        z = np.zeros((0, 2))
        self.problem = BaProblem(np.concatenate(Ui) if Ui else z, np.concatenate(Uj) if Uj else z, ptrs, pairs, n)
        self.both = both
        self.calls = 0

    def __call__(self, Phi, pmap, baseCams, camList, seed, sigmaHuber, want_H=True):
        self.calls += 1
        camLin = applyIncrements(baseCams, Phi, pmap)
        cs, npar, P = column_map(pmap, self.problem.n_cams)
        return self.problem.normal_eqns(pack_cameras(baseCams), pack_cameras(camLin), cs, npar, P, sigmaHuber, self.both,
                                        want_H)


class HostEvaluator:
    """accumulateNormalEqnsBlock over the same matches with an injectable per-pair block function (the CPU tests pass the
    oracle's); always returns H and g."""

    def __init__(self, matches, keypoints, both=True, blocks=ba_pair_blocks):
        self.matches, self.keypoints, self.both, self.blocks = matches, keypoints, both, blocks
        self.calls = 0

    def __call__(self, Phi, pmap, baseCams, camList, seed, sigmaHuber, want_H=True):
        self.calls += 1
        return accumulateNormalEqnsBlock(Phi, pmap, baseCams, camList, seed, self.matches, self.keypoints, None, sigmaHuber,
                                         {"OneDirection": not self.both}, blocks=self.blocks)


# ---- bundleAdjustmentH.m: joint refinement of the absolute homographies of a planar set ----------------------------------

def normalizeH(H):
    """H = normalizeH(H) (bundleAdjustmentH.m:965-980): H / H(3,3); when H(3,3) == 0 first H / (sign(det) cbrt(max(eps,
    |det|)))."""
    H = np.array(H, np.float64, copy=True).reshape(3, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        if H[2, 2] == 0:
            d = np.linalg.det(H)
            H = H / (np.sign(d) * np.cbrt(max(np.finfo(float).eps, abs(d))))
        if H[2, 2] != 0:
            H = H / H[2, 2]
    return H


def hom2param(H):
    """p = hom2param(H) (:924-941): [a b c d e f g h] of normalizeH(H), row-major."""
    return normalizeH(H).ravel()[:8].copy()


def param2hom(p):
    """H = param2hom(p) (:943-963): [a b c; d e f; g h 1]."""
    return np.append(np.asarray(p, np.float64).reshape(8), 1.0).reshape(3, 3)


def randPermutationPairSeed(imgI, imgJ):
    """The RandStream seed of randPermutationPair (:1118-1138) for the 1-based image indices, in MATLAB's saturating
    uint32 arithmetic: mod(sat(sat(1664525 imgI) + sat(1013904223 imgJ)), 2^31 - 1), 0 becoming 1."""
    a = _u32(1664525.0 * _u32(imgI))
    b = _u32(1013904223.0 * _u32(imgJ))
    seed = int(_u32(a + b)) % (2 ** 31 - 1)
    return seed if seed != 0 else 1


def randPermutationPair(M, kCap, imgI, imgJ):
    """kCap distinct 0-based indices of 0 .. M-1 (randperm(rs, M, kCap)), drawn from numpy's Philox stream under
    randPermutationPairSeed; MATLAB's threefry randperm order is not reproduced."""
    rng = np.random.Generator(np.random.Philox(randPermutationPairSeed(imgI, imgJ)))
    return rng.choice(int(M), int(min(kCap, M)), replace=False)


def subsampleMatchesH(Ui, Uj, i, j, cap, mode="random"):
    """[Ui, Uj] = subsampleMatches(...) of bundleAdjustmentH (:1020-1069) for the 0-based images i, j: a pair of at most
    `cap` matches is returned as it is, a larger one keeps `cap` of them ('random': randPermutationPair of the 1-based
    indices).  'grid' and 'polar' are not built."""
    Ui, Uj = np.asarray(Ui, np.float64), np.asarray(Uj, np.float64)
    if cap is None or not np.isfinite(cap) or len(Ui) <= cap:
        return Ui, Uj
    if mode != "random":
        raise NotImplementedError("SubsampleMode %r is not built (only 'random')" % (mode,))
    idx = randPermutationPair(len(Ui), int(cap), i + 1, j + 1)
    return Ui[idx], Uj[idx]


def _h_jacobian_rows(Hm, u, v, Y1, Y2, Y3, w):
    """computeJacobianBatch (:685-737) as written: the (M, 2, 8) rows du/dp, dv/dp times w, elementwise."""
    M = len(u)
    one, zero = np.ones(M), np.zeros(M)
    dY1 = np.stack([u, v, one, zero, zero, zero, zero, zero], 1)
    dY2 = np.stack([zero, zero, zero, u, v, one, zero, zero], 1)
    dY3 = np.stack([zero, zero, zero, zero, zero, zero, u, v], 1)
    y3sq = (Y3 * Y3)[:, None]
    du = (dY1 * Y3[:, None] - Y1[:, None] * dY3) / y3sq * w[:, None]
    dv = (dY2 * Y3[:, None] - Y2[:, None] * dY3) / y3sq * w[:, None]
    return np.stack([du, dv], 1)


def hNormalEqnsMirror(Ui, Uj, pair_ptr, pairs, G, seed, huber, want_H=True):
    """The numpy mirror of aps_ba_h_normal_eqns: the same f64 operations in the same order (include/aps.h), elementwise
    numpy and explicit loops only - the oracle of that entry's bit contract.  Ui, Uj: the pairs' points back to back
    (pair_ptr delimits them); pairs: [(i, j)] 0-based, i < j, sorted; G: n x 3 x 3 (or n x 9), H(3,3) = 1.
    Returns (H P x P, g, stats = [sum (w res)^2, sum |res|^2, match count]); H, g are None when want_H is False."""
    pairs = [tuple(int(x) for x in q) for q in pairs]
    n = len(G)
    Gm = np.asarray(G, np.float64).reshape(n, 9)
    Ui = np.asarray(Ui, np.float64).reshape(-1, 2)
    Uj = np.asarray(Uj, np.float64).reshape(-1, 2)
    ptr_ = np.asarray(pair_ptr, np.int64)
    n_pairs = len(pairs)
    cnt = ptr_[1:] - ptr_[:-1]
    delta = max(0.0, float(huber))
    P = 8 * (n - 1)
    Mt = int(ptr_[-1]) if n_pairs else 0
    # per match: the pair's homographies, the residual, the Huber weight
    owner = np.repeat(np.arange(n_pairs), cnt)
    ii = np.array([q[0] for q in pairs], np.int64)[owner] if n_pairs else np.zeros(0, np.int64)
    jj = np.array([q[1] for q in pairs], np.int64)[owner] if n_pairs else np.zeros(0, np.int64)

    def project(Hr, u, v):
        return (Hr[:, 0] * u + Hr[:, 1] * v + Hr[:, 2], Hr[:, 3] * u + Hr[:, 4] * v + Hr[:, 5], Hr[:, 6] * u + Hr[:, 7] * v + 1.0)

    ui, vi, uj, vj = Ui[:Mt, 0], Ui[:Mt, 1], Uj[:Mt, 0], Uj[:Mt, 1]
    Yi1, Yi2, Yi3 = project(Gm[ii], ui, vi)
    Yj1, Yj2, Yj3 = project(Gm[jj], uj, vj)
    ru = Yi1 / Yi3 - Yj1 / Yj3
    rv = Yi2 / Yi3 - Yj2 / Yj3
    nn = ru * ru + rv * rv
    w = np.ones(Mt)
    if delta > 0:
        nrm = np.sqrt(nn)
        out = nrm >= delta
        w[out] = delta / nrm[out]
    wr = np.stack([ru * w, rv * w], 1)
    if want_H:
        Ji = _h_jacobian_rows(Gm[ii], ui, vi, Yi1, Yi2, Yi3, w)
        Jj = -_h_jacobian_rows(Gm[jj], uj, vj, Yj1, Yj2, Yj3, w)
    # per pair: 64 lane-strided partials (match k on lane k mod 64, ascending k; row u, then row v), then the butterfly
    steps = int(-(-cnt.max() // 64)) if n_pairs and cnt.max() > 0 else 0
    lane = np.arange(64)
    sums = np.zeros((n_pairs, 64, 3))
    if want_H:
        Hii = np.zeros((n_pairs, 64, 8, 8))
        Hjj = np.zeros((n_pairs, 64, 8, 8))
        Hij = np.zeros((n_pairs, 64, 8, 8))
        gi = np.zeros((n_pairs, 64, 8))
        gj = np.zeros((n_pairs, 64, 8))
    for s in range(steps):
        k = s * 64 + lane[None, :]
        valid = k < cnt[:, None]
        idx = np.where(valid, ptr_[:-1, None] + k, 0)
        for q in range(2):
            e = wr[idx, q] * wr[idx, q]
            sums[:, :, 0] = np.where(valid, sums[:, :, 0] + e, sums[:, :, 0])
        sums[:, :, 1] = np.where(valid, sums[:, :, 1] + nn[idx], sums[:, :, 1])
        sums[:, :, 2] = np.where(valid, sums[:, :, 2] + 1.0, sums[:, :, 2])
        if want_H:
            v2, v3 = valid[:, :, None], valid[:, :, None, None]
            for q in range(2):
                a, b, r = Ji[idx, q], Jj[idx, q], wr[idx, q][:, :, None]
                Hii = np.where(v3, Hii + a[:, :, :, None] * a[:, :, None, :], Hii)
                Hjj = np.where(v3, Hjj + b[:, :, :, None] * b[:, :, None, :], Hjj)
                Hij = np.where(v3, Hij + a[:, :, :, None] * b[:, :, None, :], Hij)
                gi = np.where(v2, gi + a * r, gi)
                gj = np.where(v2, gj + b * r, gj)
    for s in (32, 16, 8, 4, 2, 1):
        sums = sums + sums[:, lane ^ s]
        if want_H:
            Hii, Hjj, Hij = Hii + Hii[:, lane ^ s], Hjj + Hjj[:, lane ^ s], Hij + Hij[:, lane ^ s]
            gi, gj = gi + gi[:, lane ^ s], gj + gj[:, lane ^ s]
    # assembly in pair order; the statistics summed in pair order
    stats = [0.0, 0.0, 0.0]
    for p in range(n_pairs):
        if cnt[p] > 0:
            for e in range(3):
                stats[e] = stats[e] + float(sums[p, 0, e])
    if not want_H:
        return None, None, np.array(stats)
    col = {}
    for k in range(n):
        if k != seed:
            col[k] = np.arange(8 * len(col), 8 * len(col) + 8)
    H = np.zeros((P, P))
    g = np.zeros(P)
    for p, (i, j) in enumerate(pairs):
        if cnt[p] == 0:
            continue
        if i != seed:
            H[np.ix_(col[i], col[i])] += Hii[p, 0]
            g[col[i]] += gi[p, 0]
        if j != seed:
            H[np.ix_(col[j], col[j])] += Hjj[p, 0]
            g[col[j]] += gj[p, 0]
        if i != seed and j != seed:
            H[np.ix_(col[i], col[j])] += Hij[p, 0]
            H[np.ix_(col[j], col[i])] += Hij[p, 0].T
    return H, g, np.array(stats)


def _h_problem(pairs, n):
    """(Ui, Uj, pair_ptr, [(i, j)]) of bundleAdjustmentH's pairs (dicts with i < j, Ui, Uj), in (i, j) order."""
    pairs = sorted(pairs, key=lambda q: (q["i"], q["j"]))
    for q in pairs:
        if not 0 <= q["i"] < q["j"] < n:
            raise ValueError("pairs need 0 <= i < j < N, got (%d, %d)" % (q["i"], q["j"]))
    z = np.zeros((0, 2))
    Ui = np.concatenate([np.asarray(q["Ui"], np.float64).reshape(-1, 2) for q in pairs]) if pairs else z
    Uj = np.concatenate([np.asarray(q["Uj"], np.float64).reshape(-1, 2) for q in pairs]) if pairs else z
    ptrs = np.concatenate([[0], np.cumsum([len(q["Ui"]) for q in pairs])]).astype(np.int64)
    return Ui, Uj, ptrs, [(q["i"], q["j"]) for q in pairs]


class DeviceEvaluatorH:
    """The production data-term evaluator of bundleAdjustmentH: a resident BaProblem over the (subsampled) pairs, evaluated
    by aps_ba_h_normal_eqns.  Call signature shared with HostEvaluatorH: (G n x 3 x 3, seed, huber, want_H) ->
    (J'J, J'r, [sum (w res)^2, sum |res|^2, count])."""

    def __init__(self, pairs, n):
        Ui, Uj, ptrs, ij = _h_problem(pairs, n)
        self.problem = BaProblem(Ui, Uj, ptrs, ij, n)
        self.calls = 0

    def __call__(self, G, seed, huber, want_H=True):
        self.calls += 1
        return self.problem.h_normal_eqns(G, seed, huber, want_H)


class HostEvaluatorH:
    """hNormalEqnsMirror over the same pairs (the CPU tests' evaluator)."""

    def __init__(self, pairs, n):
        self.Ui, self.Uj, self.ptrs, self.ij = _h_problem(pairs, n)
        self.calls = 0

    def __call__(self, G, seed, huber, want_H=True):
        self.calls += 1
        return hNormalEqnsMirror(self.Ui, self.Uj, self.ptrs, self.ij, G, seed, huber, want_H)


def adaptiveLM(p0, evaluate, MaxIters=50, Lambda=1e-3):
    """p = adaptiveLM(...) (bundleAdjustmentH.m:147-279) as written, on an evaluator evaluate(p, want_H) -> (J'J, J'r,
    E = 0.5 r'r, aux) (J'J and J'r None when want_H is False).  Per iteration: (J'J + lambda I) dp = -g (solveSpd: dense
    Cholesky, lstsq as the fallback, for the reference's sparse mldivide); stop when |dp| <= 1e-8 (1 + |p|); one energy-only
    evaluation at p + dp; rho = dE / (|-g'dp - 0.5 lambda dp'dp| + eps); rho > 0 accepts (one full evaluation at the new p,
    lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2), otherwise lambda *= nu, nu *= 2 and the cached J'J, g stay; then the
    gradient stop |g| <= 1e-10 (1 + E) on this iteration's g and the stop at lambda > 1e12.
    Returns (p, info) with info = dict(reason ('step', 'gradient', 'lambda' or 'max_iters'), iterations, accepted, E, aux
    of the returned p, E_init, aux_init)."""
    p = np.array(p0, np.float64, copy=True)
    lam, nu = float(Lambda), 2.0
    JtJ, g, E, aux = evaluate(p, True)
    info = {"reason": "max_iters", "iterations": 0, "accepted": 0, "E_init": E, "aux_init": aux}
    eps = np.finfo(float).eps
    for it in range(1, int(MaxIters) + 1):
        info["iterations"] = it
        dp = solveSpd(JtJ + lam * np.eye(len(p)), -g)
        if np.linalg.norm(dp) <= 1e-8 * (1 + np.linalg.norm(p)):
            info["reason"] = "step"
            break
        pNew = p + dp
        _, _, ENew, auxNew = evaluate(pNew, False)
        dEPred = -float(g @ dp) - 0.5 * float(dp @ (lam * dp))
        rho = (E - ENew) / (abs(dEPred) + eps)
        gIt = g
        if rho > 0:
            p, E, aux = pNew, ENew, auxNew
            JtJ, g, _, _ = evaluate(p, True)
            lam = lam * max(1 / 3, 1 - (2 * rho - 1) ** 3)
            nu = 2.0
            info["accepted"] += 1
        else:
            lam = lam * nu
            nu = 2 * nu
        if np.linalg.norm(gIt) <= 1e-10 * (1 + E):
            info["reason"] = "gradient"
            break
        if lam > 1e12:
            info["reason"] = "lambda"
            break
    info["E"], info["aux"] = E, aux
    return p, info


def _h_absolute(p, G, mask, seed):
    """Habs of residualsJacobian (:311-323): normalizeH(param2hom(p block)) for every non-seed image, eye(3) for the seed."""
    out, b = [], 0
    for k in range(len(G)):
        if k == seed:
            out.append(np.eye(3))
        else:
            out.append(normalizeH(param2hom(p[8 * b:8 * b + 8])))
            b += 1
    return np.stack(out)


def bundleAdjustmentH(input, pairs, N, seed, G0, MaxIters=50, Huber=1.0, Lambda=1e-3, RegProj=1e-4, RegDet=0.0,
                      UseLSQ=False, OneDirection=True, MaxMatches=np.inf, SubsampleMode="random", ImageSizes=None,
                      evaluator=None):
    """[G, stats] = bundleAdjustmentH(input, pairs, N, seed, 'Name', Value, ...) (bundleAdjustmentH.m:1-145) with the
    adaptiveLM optimiser, indices 0-based.  pairs: dicts with i < j and the matched points Ui, Uj (M x 2 pixels) of each;
    G0: N initial absolute homographies (normalised, the seed's replaced by eye(3)).  Minimises 0.5 r'r over the
    one-direction Huber-weighted transfer residuals Hi ui - Hj uj (on the device: aps_ba_h_normal_eqns) plus the RegProj
    rows sqrt(RegProj) H(3,1), sqrt(RegProj) H(3,2) of every non-seed image (on the host).  A pair with more than
    MaxMatches matches keeps MaxMatches of them (subsampleMatchesH).  evaluator(pairs, N) builds the data-term evaluator
    (default: DeviceEvaluatorH).  Not built: UseLSQ (lsqnonlin; bundleAdjustmentRKf passes false), bidirectional residuals
    (OneDirection = false), RegDet > 0, the 'grid' / 'polar' subsampling.
    Returns (G: N refined homographies with H(3,3) = 1, the seed's exactly eye(3); stats = dict(evaluations, rmse_init,
    rmse_final [unweighted transfer RMSE in px over the subsampled matches], reason, iterations, accepted, E_init,
    E_final))."""
    if UseLSQ:
        raise NotImplementedError("UseLSQ (lsqnonlin) is not built; the adaptive LM is")
    if not OneDirection:
        raise NotImplementedError("bidirectional residuals (OneDirection = false) are not built")
    if RegDet and RegDet > 0:
        raise NotImplementedError("RegDet > 0 is not built")
    G = [normalizeH(G0[k]) for k in range(N)]
    G[seed] = np.eye(3)
    sub = []
    for q in pairs:
        Ui, Uj = subsampleMatchesH(q["Ui"], q["Uj"], q["i"], q["j"], MaxMatches, SubsampleMode)
        sub.append({"i": int(q["i"]), "j": int(q["j"]), "Ui": Ui, "Uj": Uj})
    evaluate_data = (evaluator or DeviceEvaluatorH)(sub, N)
    mask = [k != seed for k in range(N)]
    p0 = np.concatenate([hom2param(G[k]) for k in range(N) if mask[k]]) if N > 1 else np.zeros(0)
    sreg = np.sqrt(RegProj) if RegProj > 0 else 0.0

    def evaluate(p, want_H):
        Habs = _h_absolute(p, G, mask, seed)
        JtJ, g, st = evaluate_data(Habs, seed, Huber, want_H)
        rr = float(st[0])
        if want_H:
            JtJ, g = np.array(JtJ, np.float64, order="C"), np.array(g, np.float64)
        b = 0
        for k in range(N):  # the RegProj rows (:438-467)
            if not mask[k] or sreg == 0.0:
                continue
            for e, (rr_k, c) in enumerate(((sreg * Habs[k][2, 0], 8 * b + 6), (sreg * Habs[k][2, 1], 8 * b + 7))):
                rr = rr + rr_k * rr_k
                if want_H:
                    JtJ[c, c] = JtJ[c, c] + sreg * sreg
                    g[c] = g[c] + sreg * rr_k
            b += 1
        return JtJ, g, 0.5 * rr, st

    p, info = adaptiveLM(p0, evaluate, MaxIters, Lambda)
    Gout = [np.eye(3) if k == seed else None for k in range(N)]
    b = 0
    for k in range(N):
        if mask[k]:
            Gout[k] = normalizeH(param2hom(p[8 * b:8 * b + 8]))
            b += 1
    rmse = lambda st: float(np.sqrt(max(float(st[1]), 0.0) / max(float(st[2]), 1.0)))  # noqa: E731
    stats = {"evaluations": evaluate_data.calls, "rmse_init": rmse(info["aux_init"]), "rmse_final": rmse(info["aux"]),
             "reason": info["reason"], "iterations": info["iterations"], "accepted": info["accepted"],
             "E_init": info["E_init"], "E_final": info["E"]}
    return Gout, stats


# ---- camera initialisation: initializeCameraMatrices.m --------------------------------------------------------------------

def projectToSO3(M):
    """rotation = projectToSO3(M) (initializeCameraMatrices.m:743-763): U diag(1, 1, sign(det(U V'))) V'."""
    U, _, Vt = np.linalg.svd(np.asarray(M, np.float64))
    return U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt


def ppCenter(W, H):
    return W / 2.0, H / 2.0


def centerNormalizeH(H, Wi, Hi, Wj, Hj):
    """Hn = centerNormalizeH(H, Wi, Hi, Wj, Hj) (:698-741): Ci^-1 H Cj scaled to unit |det|; None when degenerate."""
    cxi, cyi = ppCenter(Wi, Hi)
    cxj, cyj = ppCenter(Wj, Hj)
    Ci = np.array([[1, 0, cxi], [0, 1, cyi], [0, 0, 1.0]])
    Cj = np.array([[1, 0, cxj], [0, 1, cyj], [0, 0, 1.0]])
    Hc = np.linalg.solve(Ci, np.asarray(H, np.float64)) @ Cj
    d = np.linalg.det(Hc)
    if not np.isfinite(d) or d == 0:
        return None
    return Hc / (np.sign(d) * np.cbrt(abs(d)))


def focalsHomographyShumsz(H):
    """f = focalsHomographyShumsz(H) (:630-696): the Shum-Szeliski focal of one centred homography, NaN when the
    constraints give none; the geometric mean of the two sides' estimates."""
    H = np.asarray(H, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d1 = H[2, 0] * H[2, 1]
        d2 = (H[2, 1] - H[2, 0]) * (H[2, 1] + H[2, 0])
        v1 = -(H[0, 0] * H[0, 1] + H[1, 0] * H[1, 1]) / d1
        v2 = (H[0, 0] ** 2 + H[1, 0] ** 2 - H[0, 1] ** 2 - H[1, 1] ** 2) / d2
        if v1 < v2:
            v1, v2 = v2, v1
        if v1 > 0 and v2 > 0:
            f1 = np.sqrt(v1 * (abs(d1) > abs(d2)) + v2 * (abs(d1) <= abs(d2)))
        elif v1 > 0:
            f1 = np.sqrt(v1)
        else:
            return np.nan
        d1 = H[0, 0] * H[1, 0] + H[0, 1] * H[1, 1]
        d2 = H[0, 0] ** 2 + H[0, 1] ** 2 - H[1, 0] ** 2 - H[1, 1] ** 2
        v1 = -H[0, 2] * H[1, 2] / d1
        v2 = (H[1, 2] ** 2 - H[0, 2] ** 2) / d2
        if v1 < v2:
            v1, v2 = v2, v1
        if v1 > 0 and v2 > 0:
            f0 = np.sqrt(v1 * (abs(d1) > abs(d2)) + v2 * (abs(d1) <= abs(d2)))
        elif v1 > 0:
            f0 = np.sqrt(v1)
        else:
            return np.nan
    return float(np.sqrt(f1 * f0))


def _fallback_focal(imageSizes):
    return float(np.median(0.8 * np.max(np.asarray(imageSizes, np.float64), axis=1)))


def focalShumSzeliski(pairs, imageSizes):
    """The 'shumSzeliskiOneHPaper' branch of initializeKRf (:274-305): the median of the per-homography focals of every
    centred H and its inverse, or None when none is plausible."""
    Hc = []
    for p in pairs:
        i, j = p["i"], p["j"]
        h = centerNormalizeH(p["Hij"], imageSizes[i][1], imageSizes[i][0], imageSizes[j][1], imageSizes[j][0])
        if h is not None:
            Hc.append(h)
    fvec = np.array([focalsHomographyShumsz(M) for M in Hc + [np.linalg.inv(M) for M in Hc]], np.float64)
    fvec = fvec[np.isfinite(fvec) & (fvec > 0) & (fvec < 5e4)]
    return float(np.median(fvec)) if fvec.size else None


def focalWConstraint(pairs, imageSizes):
    """The 'wConstraint' branch of initializeKRf (:193-272): candidates w = 1/f^2 from the two constraints of each
    centred, det-normalised H, MAD-filtered, converted to f and kept inside [0.3, 6] x the median longer side; the
    median, or None."""
    ws = []
    eps = np.finfo(float).eps
    for p in pairs:
        i, j = p["i"], p["j"]
        cxi, cyi = ppCenter(imageSizes[i][1], imageSizes[i][0])
        cxj, cyj = ppCenter(imageSizes[j][1], imageSizes[j][0])
        Ci = np.array([[1, 0, cxi], [0, 1, cyi], [0, 0, 1.0]])
        Cj = np.array([[1, 0, cxj], [0, 1, cyj], [0, 0, 1.0]])
        Hc = np.linalg.solve(Ci, np.asarray(p["Hij"], np.float64)) @ Cj
        d = np.linalg.det(Hc)
        if not np.isfinite(d) or d == 0:
            continue
        Hn = Hc / (np.sign(d) * np.cbrt(abs(d)))
        h1, h2 = Hn[:, 0], Hn[:, 1]
        denA = h1[0] * h2[0] + h1[1] * h2[1]
        if abs(denA) > eps:
            wA = -(h1[2] * h2[2]) / denA
            if np.isfinite(wA) and wA > 0:
                ws.append(wA)
        denB = (h1[0] ** 2 + h1[1] ** 2) - (h2[0] ** 2 + h2[1] ** 2)
        if abs(denB) > eps:
            wB = (h2[2] ** 2 - h1[2] ** 2) / denB
            if np.isfinite(wB) and wB > 0:
                ws.append(wB)
    ws = np.array(ws, np.float64)
    ws = ws[np.isfinite(ws) & (ws > 0)]
    if not ws.size:
        return None
    medw = np.median(ws)
    madw = np.median(np.abs(ws - medw))  # mad(ws, 1)
    keep = np.abs(ws - medw) <= (1e-6 * max(1.0, medw) if madw == 0 else 3 * madw)
    ws = ws[keep]
    if not ws.size:
        return None
    base = np.median(np.max(np.asarray(imageSizes, np.float64), axis=1))
    f = 1.0 / np.sqrt(ws)
    f = f[np.isfinite(f) & (f >= 0.3 * base) & (f <= 6.0 * base)]
    return float(np.median(f)) if f.size else None


def maximumSpanningTree(G):
    """tree = maximumSpanningTree(G) (:398-455): Kruskal over the weights in descending order (ties in column-major
    order, MATLAB's stable sort); a symmetric N x N matrix of the chosen weights."""
    G = np.asarray(G, np.float64)
    n = G.shape[0]
    ccs = list(range(n))
    comps = [[k] for k in range(n)]
    tree = np.zeros((n, n))
    vals = G.ravel(order="F")
    order = np.argsort(-vals, kind="stable")
    edges = 0
    for lin in order:
        v = vals[lin]
        if v > 0:
            i, j = int(lin % n), int(lin // n)
            if ccs[i] != ccs[j]:
                tree[i, j] = tree[j, i] = v
                a, b = ccs[i], ccs[j]
                comps[a] = comps[a] + comps[b]
                for m in comps[b]:
                    ccs[m] = a
                edges += 1
        if edges == n - 1:
            break
    return tree


def chainedHomographies(G, seed, Tforms, n):
    """tforms = chainedHomographies(G, seed, Tforms, n) (:457-522): depth-first over G from the seed (neighbours in index
    order, the visited set is the current path as in the reference's by-value recursion), tforms{j} = tforms{i} *
    Tforms{i, j} normalised to [3, 3] = 1: every view's homography to the seed."""
    tforms = [np.eye(3) for _ in range(n)]

    def walk(i, visited):
        visited = visited | {i}
        for j in range(n):
            if G[i, j] > 0 and j not in visited:
                t = tforms[i] @ np.asarray(Tforms[i][j], np.float64)
                tforms[j] = t / t[2, 2]
                walk(j, visited)

    walk(seed, frozenset())
    return tforms


def relativeRotHij(Hij, Wi, Hi, Wj, Hj, f):
    """(:588-628) ~ R_i R_j' from the homography j -> i: centred, det-normalised, K0^-1 Hn K0, projected to SO(3)."""
    cxi, cyi = ppCenter(Wi, Hi)
    cxj, cyj = ppCenter(Wj, Hj)
    Ci = np.array([[1, 0, cxi], [0, 1, cyi], [0, 0, 1.0]])
    Cj = np.array([[1, 0, cxj], [0, 1, cyj], [0, 0, 1.0]])
    Hc = np.linalg.solve(Ci, np.asarray(Hij, np.float64)) @ Cj
    d = np.linalg.det(Hc)
    Hn = Hc / (np.sign(d) * np.cbrt(abs(d) + np.finfo(float).eps))
    K0 = np.diag([f, f, 1.0])
    return projectToSO3(np.linalg.solve(K0, Hn) @ K0)


def rotationConsistency(pairs, imageSizes, R, f):
    """[noRotation, meanAE, medAE, maxAE] = rotationConsistency(...) (:524-573): the angle between R_i R_j' and each
    pair's homography rotation; a set is non-rotational when the median exceeds 0.6 deg and the maximum 100 deg."""
    err = []
    for p in pairs:
        i, j = p["i"], p["j"]
        Rrel = relativeRotHij(p["Hij"], imageSizes[i][1], imageSizes[i][0], imageSizes[j][1], imageSizes[j][0], f)
        D = R[i] @ R[j].T
        err.append(np.arccos(np.clip((np.trace(D.T @ Rrel) - 1) / 2, -1, 1)))
    err = np.degrees(np.array(err)) if err else np.zeros(1)
    meanAE, medAE, maxAE = float(err.mean()), float(np.median(err)), float(err.max())
    return bool(medAE > 0.6 and maxAE > 100), meanAE, medAE, maxAE


def initializeKRf(input, pairs, imageSizes, N, seed, Tforms, numMatches):
    """[K, R, fUsed, H2seed, noRotation] = initializeKRf(...) (initializeCameraMatrices.m:137-388): one focal for the
    set (input['focalEstimateMethod']), K with the image centre as principal point, rotations propagated from the
    seed over the maximum spanning tree of the match counts (breadth first), the rotation-consistency verdict, and the
    chained homographies when the set is planar (or forcePlanarScan)."""
    method = input.get("focalEstimateMethod", "shumSzeliskiOneHPaper")
    if method == "wConstraint":
        fUsed = focalWConstraint(pairs, imageSizes)
    elif method == "shumSzeliskiOneHPaper":
        fUsed = focalShumSzeliski(pairs, imageSizes)
    else:
        raise ValueError("Require one focal estimate method.")
    if fUsed is None:
        fUsed = _fallback_focal(imageSizes)
    K = []
    for i in range(N):
        cx, cy = ppCenter(imageSizes[i][1], imageSizes[i][0])
        K.append(np.array([[fUsed, 0, cx], [0, fUsed, cy], [0, 0, 1.0]]))
    tree = maximumSpanningTree(numMatches)
    jv, iv = np.nonzero(np.triu(tree, 1).T)  # find(triu(tree, 1)): column-major order
    treeEdges = list(zip(iv.tolist(), jv.tolist()))
    R = [np.eye(3) for _ in range(N)]
    visited = [False] * N
    visited[seed] = True
    queue = [seed]
    while queue:
        u = queue.pop(0)
        for (i, j) in treeEdges:
            if i == u and not visited[j]:
                Rrel = relativeRotHij(Tforms[i][j], imageSizes[i][1], imageSizes[i][0], imageSizes[j][1], imageSizes[j][0], fUsed)
                R[j] = projectToSO3(Rrel.T @ R[i])
                visited[j] = True
                queue.append(j)
            elif j == u and not visited[i]:
                Rrel = relativeRotHij(Tforms[j][i], imageSizes[i][1], imageSizes[i][0], imageSizes[j][1], imageSizes[j][0], fUsed)
                R[i] = projectToSO3(Rrel.T @ R[j])
                visited[i] = True
                queue.append(i)
    noRotation, meanAE, medAE, maxAE = rotationConsistency(pairs, imageSizes, R, fUsed)
    if noRotation or input.get("forcePlanarScan", False):
        H2seed = chainedHomographies(tree, seed, Tforms, N)
    else:
        H2seed = [np.eye(3) for _ in range(N)]
    return K, R, float(fUsed), H2seed, noRotation


def initializeCameraMatrices(input, pairs, imageSizes, Tforms, seed, N, numMatches):
    """cameras = initializeCameraMatrices(...) (:1-135): one dict per image with f, K, R, H2seed, noRotation."""
    K, R, f, H2seed, noRot = initializeKRf(input, pairs, imageSizes, N, seed, Tforms, numMatches)
    return [{"f": f, "K": K[i], "R": R[i], "H2seed": H2seed[i], "noRotation": int(noRot), "initialized": False,
             "cx": K[i][0, 2], "cy": K[i][1, 2]} for i in range(N)]


# ---- bundleAdjustmentRKf.m ----------------------------------------------------------------------------------------------------

def buildPairs(numMatches, matches, keypoints, Tforms):
    """pairs = buildPairs(...) (:376-435): every upper-triangle entry with matches, in column-major order, with its
    points and its homography j -> i."""
    nm = np.asarray(numMatches)
    N = len(keypoints)
    out = []
    for j in range(N):
        for i in range(j):
            if nm[i, j] == 0:
                continue
            M = np.asarray(matches[i][j], np.int64)
            out.append({"i": i, "j": j, "Ui": np.asarray(keypoints[i], np.float64)[M[:, 0] - 1],
                        "Uj": np.asarray(keypoints[j], np.float64)[M[:, 1] - 1], "Hij": np.asarray(Tforms[i][j], np.float64)})
    return out


def _matlab_round(x):
    return float(np.sign(x) * np.floor(abs(x) + 0.5))


def _u32(x):
    """MATLAB's uint32(x): rounds and SATURATES to [0, 2^32 - 1] (no wrap-around)."""
    return min(max(_matlab_round(x), 0.0), 4294967295.0)


def randpermSeed(camI, camJ):
    """The RandStream seed of randpermPerPair (:1104-1139), restated in MATLAB's saturating uint32 arithmetic: it depends
    on the two principal points only (for image-centre principal points of a few hundred pixels every product
    saturates and the seed is 1)."""
    ci = _matlab_round(1e3 * camI["K"][0, 2] + 2e3 * camI["K"][1, 2])
    cj = _matlab_round(1e3 * camJ["K"][0, 2] + 2e3 * camJ["K"][1, 2])
    a = _u32(1664525.0 * _u32(ci))
    b = _u32(1013904223.0 * _u32(cj))
    seed = int(_u32(a + b)) % (2 ** 31 - 1)
    return seed if seed != 0 else 1


def subsampleMatches(M, camI, camJ, cap):
    """The 'random' mode of subsampleMatches (:1047-1102) on a pair's match list (M x 2): at most `cap` rows.  The draw is
    numpy's Philox stream (a counter-based generator, as the reference's threefry) under randpermSeed; MATLAB's
    randperm order is not reproduced.  'grid' and 'polar' are not built."""
    M = np.asarray(M)
    if cap is None or not np.isfinite(cap) or len(M) <= cap:
        return M
    rng = np.random.Generator(np.random.Philox(randpermSeed(camI, camJ)))
    return M[rng.choice(len(M), int(cap), replace=False)]


def buildBrownLowePrior(camList, seed, cameras, opts, pmap):
    """CpInv = buildBrownLowePrior(...) (:1503-1639), dense: 1/sigma_theta^2 (sigma_theta = pi/16) on the rotation
    columns, 1/sigma_f^2 (sigma_f = max(1, mean f / 20)) on the focal columns, plus the focal smoothness couplings of
    cameras at most two apart in camList and in index, and the focal-mean term."""
    fbar = float(np.mean([cameras[i]["f"] for i in camList]))
    sigth = np.pi / 16
    sigf = max(1.0, fbar / 20)
    last = pmap[-1]
    P = last["startIdx"] + (1 if last["isSeed"] else 4)
    C = np.zeros((P, P))
    fc = []
    for e in pmap:
        s = e["startIdx"]
        if e["isSeed"]:
            C[s, s] = 1 / sigf ** 2
            fc.append(s)
        else:
            C[s:s + 3, s:s + 3] += np.eye(3) / sigth ** 2
            C[s + 3, s + 3] = 1 / sigf ** 2
            fc.append(s + 3)
    cams = [e["camIdx"] for e in pmap]
    n = len(pmap)
    lf = opts.get("FocalSmoothnessWeight", 0)
    if isinstance(lf, (int, float)) and lf > 0:
        for ki in range(n - 1):
            for kj in range(ki + 1, min(ki + 3, n)):
                if abs(cams[ki] - cams[kj]) <= 2:
                    a, b = fc[ki], fc[kj]
                    C[a, a] += lf
                    C[b, b] += lf
                    C[a, b] -= lf
                    C[b, a] -= lf
    lm = opts.get("FocalMeanWeight", 0)
    if isinstance(lm, (int, float)) and lm > 0:
        fcs = np.array(fc)
        C[np.ix_(fcs, fcs)] -= lm / n
        C[fcs, fcs] += lm / n + lm * (n - 1) / n
    return C


def capPerCameraStep(delta, pmap, cameras, thetaCap, fracDf):
    """deltaC = capPerCameraStep(...) (:984-1045): a rotation step longer than thetaCap is scaled back to it, a focal
    step is clipped to +-fracDf * f."""
    d = np.array(delta, np.float64, copy=True)
    for e in pmap:
        s, f = e["startIdx"], float(cameras[e["camIdx"]]["f"])
        if not e["isSeed"]:
            a = float(np.linalg.norm(d[s:s + 3]))
            if a > thetaCap:
                d[s:s + 3] = d[s:s + 3] * (thetaCap / a)
            s = s + 3
        d[s] = max(-fracDf * f, min(fracDf * f, d[s]))
    return d


def solveSpd(A, b):
    """Stands in for solveSpd (:901-982: symamd + chol, ichol + pcg as the fallback): the systems here are at most
    4N x 4N and dense, so a dense Cholesky, and least squares when A is not numerically positive definite."""
    try:
        L = np.linalg.cholesky(A)
        return np.linalg.solve(L.T, np.linalg.solve(L, b))
    except np.linalg.LinAlgError:
        return np.linalg.lstsq(A, b, rcond=None)[0]


def runLevenbergMarquardt(cameras, camList, seed, evaluate, opts):
    """[cameras, finalRMSE] = runLevenbergMarquardt(...) (:438-607): three outer relinearisations (focal caps 0.5 %,
    1 %, 2 %), each up to MaxLMIters damped steps with the Brown-Lowe prior and the per-camera caps; a step is taken
    when the energy drops with rho > 0 (rotations re-projected to SO(3)).  `evaluate` is the normal-equation evaluator
    (DeviceEvaluator or HostEvaluator); the trial step asks it for the energy only.
    Deviation: a pass stops when an accepted step lowers the energy by less than 1e-9 (or the predicted decrease is
    below 1e-12).  The reference (:590) compares ETrial with the energy re-evaluated at the accepted cameras - the same
    number up to the SO(3) re-projection - so as written every pass ends after its first accepted step, and the
    cameras stay far from the optimum (on 6-8 synthetic views: RMSE 1.7 px where the noise gives 0.4)."""
    sigma = opts["SigmaHuber"] if opts.get("FinalPass") else 2.0
    lam = float(opts["Lambda0"])
    maxIters = int(opts["MaxLMIters"])
    opts = dict(opts)
    if opts.get("FocalSmoothnessWeight", "auto") == "auto":
        f0 = float(np.median([cameras[i]["f"] for i in camList]))
        opts["FocalSmoothnessWeight"] = (f0 / 20) ** 2 * 0.5 if len(camList) <= 5 else (f0 / 50) ** 2 * 2.0
    thetaCap = np.deg2rad(5)
    history = opts.get("history")
    rmse0 = 0.0
    for outer in range(3):
        fracDf = (0.005, 0.01, 0.02)[outer]
        Phi, pmap = buildDeltaVector(cameras, camList, seed)
        CpInv = buildBrownLowePrior(camList, seed, cameras, opts, pmap)
        H, g, E0, rmse0 = evaluate(Phi, pmap, cameras, camList, seed, sigma, True)
        for _ in range(maxIters):
            A = H + CpInv + lam * np.eye(H.shape[0])
            delta = capPerCameraStep(solveSpd(A, -g), pmap, cameras, thetaCap, fracDf)
            PhiTrial = Phi + delta
            camTrial = applyIncrements(cameras, PhiTrial, pmap)
            _, _, ETrial, _ = evaluate(PhiTrial, pmap, cameras, camList, seed, sigma, False)
            pred = 0.5 * float(delta @ (lam * delta - g + CpInv @ delta))
            rho = -np.inf if pred <= 0 else (E0 - ETrial) / pred
            if ETrial < E0 and rho > 0:
                if history is not None:
                    history.append((E0, ETrial))
                Eprev = E0
                cameras = camTrial
                for i in camList:
                    cameras[i]["R"] = projectToSO3(cameras[i]["R"])
                if rho > 0.75:
                    lam = lam / 2
                elif rho < 0.25:
                    lam = lam * 2
                lam = max(min(lam, 1e6), 1e-10)
                Phi, pmap = buildDeltaVector(cameras, camList, seed)
                CpInv = buildBrownLowePrior(camList, seed, cameras, opts, pmap)
                H, g, E0, rmse0 = evaluate(Phi, pmap, cameras, camList, seed, sigma, True)
                if abs(pred) < 1e-12 or abs(Eprev - ETrial) < 1e-9:  # (deviation: see the docstring)
                    break
            else:
                lam = min(lam * 4, 1e6)
                if lam > 1e5:
                    break
    return cameras, rmse0


def _intrinsics(f, size):
    return np.array([[f, 0, size[1] / 2.0], [0, f, size[0] / 2.0], [0, 0, 1.0]])


def bundleAdjustmentRKf(input, numMatches, matches, keypoints, imageSizes, Tforms, evaluator=None, history=None,
                        evaluatorH=None):
    """[cameras, seed] = bundleAdjustmentRKf(...) (:1-374) for one connected component, indices 0-based.
    numMatches: N x N (upper triangle used); matches[i][j] (i < j): M x 2 1-based keypoint indices; keypoints[i]: K x 2
    pixels; imageSizes: N x 3 (rows, cols, channels); Tforms[i][j]: 3 x 3 homography j -> i for every matched (i, j), both
    orders.  evaluator(matches, keypoints, both) builds the normal-equation evaluator over the subsampled matches
    (default: DeviceEvaluator).
    Seed = the image with the most matched points; cameras from initializeCameraMatrices.  A planar set (noRotation or
    input['forcePlanarScan']) returns them with H2refined: with input['planarBundleAdjustment'] the homographies refined
    by bundleAdjustmentH from H2seed (as the reference always does; evaluatorH(pairs, N) builds its data-term evaluator,
    default DeviceEvaluatorH), without it H2seed itself.  Otherwise the incremental Brown-Lowe loop: add the uninitialised image with the most
    matches to an initialised one (rotation from their homography, focal of its partner), run the global LM over every
    initialised camera, then min(2, ceil(N / 10)) final passes at sigmaHuber.
    Returns (cameras, seed, stats) with stats = dict(f_init, rmse_init [all images at the initial cameras], rmse_final,
    evaluations [normal-equation evaluations of the LM], noRotation, ...); a refined planar set reports bundleAdjustmentH's
    evaluations, transfer RMSE and energy before and after, lm_stop and lm_iterations."""
    N = len(keypoints)
    opts = {"SigmaHuber": float(input.get("sigmaHuber", 2.0)), "MaxLMIters": int(input.get("maxIterLM", 40)),
            "Lambda0": float(input.get("lambda", 1e-3)), "FocalSmoothnessWeight": "auto", "FocalMeanWeight": 50,
            "history": history}
    both = not bool(input.get("residualOneDirection", False))
    cap = input.get("MaxMatches", 300)
    nm = np.asarray(numMatches, np.float64)
    pairs = buildPairs(nm, matches, keypoints, Tforms)
    deg = np.zeros(N)
    for p in pairs:
        deg[p["i"]] += len(p["Ui"])
        deg[p["j"]] += len(p["Ui"])
    seed = int(np.argmax(deg))
    cameras = initializeCameraMatrices(input, pairs, imageSizes, Tforms, seed, N, nm)
    stats = {"f_init": cameras[0]["f"], "noRotation": int(cameras[0]["noRotation"]), "evaluations": 0,
             "rmse_init": None, "rmse_final": None}
    if cameras[0]["noRotation"] == 1 or input.get("forcePlanarScan", False):
        for c in cameras:
            c["noRotation"] = 1
        stats["noRotation"] = 1
        if not input.get("planarBundleAdjustment", False):
            # opt-in: without the key the chained homographies are kept (the reference always refines them)
            for c in cameras:
                c["H2refined"] = c["H2seed"]
            return cameras, seed, stats
        # :117-128: bundleAdjustmentH from G0 = H2seed, one-direction residuals, 'random' subsampling, no lsqnonlin
        G, hst = bundleAdjustmentH(input, pairs, N, seed, G0=[c["H2seed"] for c in cameras], MaxIters=opts["MaxLMIters"],
                                   Huber=opts["SigmaHuber"], UseLSQ=False, ImageSizes=imageSizes, OneDirection=True,
                                   MaxMatches=cap, SubsampleMode="random", evaluator=evaluatorH)
        for c, Gk in zip(cameras, G):
            c["H2refined"] = Gk
        stats.update(evaluations=hst["evaluations"], rmse_init=hst["rmse_init"], rmse_final=hst["rmse_final"],
                     lm_stop=hst["reason"], lm_iterations=hst["iterations"], E_init=hst["E_init"], E_final=hst["E_final"])
        return cameras, seed, stats
    # MaxMatches: one 'random' subset per pair, drawn once (its seed depends on the principal points only)
    sub = [[None] * N for _ in range(N)]
    for i in range(N):
        for j in range(i + 1, N):
            if matches[i][j] is not None and len(matches[i][j]):
                sub[i][j] = subsampleMatches(matches[i][j], cameras[i], cameras[j], cap)
    evaluate = (evaluator or DeviceEvaluator)(sub, keypoints, both)
    all_cams = list(range(N))
    Phi0, pm = buildDeltaVector(cameras, all_cams, seed)  # the RMSE at the initial cameras, every image, final-pass sigma
    stats["rmse_init"] = evaluate(Phi0, pm, cameras, all_cams, seed, opts["SigmaHuber"], False)[3]
    initialized = np.zeros(N, bool)
    initialized[seed] = True
    cameras[seed]["initialized"] = True
    score = nm + nm.T
    rmseHistory = []
    for step in range(1, N):
        cand = np.where(~initialized[:, None] & initialized[None, :], score, 0)
        if not (cand > 0).any():
            break  # 'No more images with matches to add'
        best, to = np.unravel_index(int(np.argmax(cand)), cand.shape)  # first maximum over (candidate, initialised)
        best, to = int(best), int(to)
        a, b = min(best, to), max(best, to)
        if matches[a][b] is None or len(matches[a][b]) < 4:
            continue  # 'Skipping (no robust matches)'
        Hij = Tforms[best][to]
        if Hij is not None:
            Hji = np.linalg.solve(_intrinsics(cameras[best]["f"], imageSizes[best]), Hij) @ _intrinsics(cameras[to]["f"], imageSizes[to])
            cameras[best]["R"] = projectToSO3(Hji) @ cameras[to]["R"] if np.isfinite(Hji).all() else cameras[to]["R"]
        else:
            cameras[best]["R"] = cameras[to]["R"]
        cameras[best]["f"] = cameras[to]["f"]
        cameras[best]["K"] = _intrinsics(cameras[best]["f"], imageSizes[best])
        cameras[best]["initialized"] = True
        initialized[best] = True
        camList = [int(k) for k in np.nonzero(initialized)[0]]
        o = dict(opts, FinalPass=len(camList) <= 3)
        cameras, rmse = runLevenbergMarquardt(cameras, camList, seed, evaluate, o)
        rmseHistory.append(rmse)
    camList = [k for k in range(N) if cameras[k]["initialized"]]
    rmse = rmseHistory[-1] if rmseHistory else 0.0
    if len(camList) > 1:
        for _ in range(min(2, int(np.ceil(len(camList) / 10)))):
            cameras, rmse = runLevenbergMarquardt(cameras, camList, seed, evaluate, dict(opts, FinalPass=True))
    stats["rmse_final"] = rmse
    stats["evaluations"] = evaluate.calls - 1  # the LM's own (not the initial RMSE's)
    stats["camList"] = camList
    stats["focals"] = [float(cameras[k]["f"]) for k in camList]
    return cameras, seed, stats
