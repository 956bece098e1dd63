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
are O(P^2..P^3) in the camera count, not in the match count)."""
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


def bundleAdjustmentRKf(input, numMatches, matches, keypoints, imageSizes, Tforms, evaluator=None, history=None):
    """[cameras, seed] = bundleAdjustmentRKf(...) (:1-374) for one connected component, indices 0-based.
    numMatches: N x N (upper triangle used); matches[i][j] (i < j): M x 2 1-based keypoint indices; keypoints[i]: K x 2
    pixels; imageSizes: N x 3 (rows, cols, channels); Tforms[i][j]: 3 x 3 homography j -> i for every matched (i, j), both
    orders.  evaluator(matches, keypoints, both) builds the normal-equation evaluator over the subsampled matches
    (default: DeviceEvaluator).
    Seed = the image with the most matched points; cameras from initializeCameraMatrices; a planar set (noRotation or
    input['forcePlanarScan']) returns them with H2refined = H2seed (the reference refines those with bundleAdjustmentH,
    which is not built here).  Otherwise the incremental Brown-Lowe loop: add the uninitialised image with the most
    matches to an initialised one (rotation from their homography, focal of its partner), run the global LM over every
    initialised camera, then min(2, ceil(N / 10)) final passes at sigmaHuber.
    Returns (cameras, seed, stats) with stats = dict(f_init, rmse_init [all images at the initial cameras], rmse_final,
    evaluations [normal-equation evaluations of the LM], noRotation, ...)."""
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
        # the reference refines H2seed with bundleAdjustmentH here (not built): the chained homographies are kept
        for c in cameras:
            c["noRotation"] = 1
            c["H2refined"] = c["H2seed"]
        stats["noRotation"] = 1
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
