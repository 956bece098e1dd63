"""The reference driver's stage order (PP/main.m:83-138) over the device hot path.

    loadImages/getFeaturePoints -> featureMatchingPairwise -> imageMatching (+ connected components)
    -> [host: camera initialisation from known intrinsics, or focal estimation + bundle adjustment (normal equations
       on the device) when they are unknown; straightening] -> renderPanorama (warp + multiband blend)

Everything heavy stays resident in HBM between stages: descriptors never leave the device, images are
uploaded once, only keypoint coordinates, match index lists and 3x3 models visit the host (they feed the
host-side graph logic exactly as in the reference).
"""
from __future__ import annotations

import threading
import time

import numpy as np

from . import _capi
from . import featureMatching as fm
from . import imageMatching as im
from . import renderPanorama as rp

DEFAULT_INPUT = {
    # inputs.m:31-40
    "detector": "SIFT", "Sigma": 1.6, "NumLayersInOctave": 4, "ContrastThreshold": 0.00133, "EdgeThreshold": 6,
    # inputs.m:44-59 (the north-star configuration: pairwise, exhaustive, scratch matcher)
    "matchFeaturesPairwise": 1, "useMATLABFeatureMatch": 0, "Matchingmethod": "Exhaustive",
    "Matchingthreshold": 1.5, "Ratiothreshold": 0.6,
    # inputs.m:62-74
    "useMATLABImageMatching": 0, "imageMatchingMethod": "ransac", "mBrownLowe": 6, "maxIter": 500,
    "maxDistance": 5.5, "inliersConfidence": 99.9, "transformationType": "projective",
    # inputs.m:76-85 (bundle adjustment, used when the intrinsics are not given)
    "maxIterLM": 40, "lambda": 1e-3, "sigmaHuber": 2.0, "focalEstimateMethod": "shumSzeliskiOneHPaper",
    "residualOneDirection": False, "MaxMatches": 300,
    # inputs.m:94-113
    "gainCompensation": 0, "blending": "multiband", "bands": 3, "MBBsigma": 1, "resizeImage": 0,
    "resizeImagePanoramaCluster": 0, "heightLimit": 800, "widthLimit": 800,
    "panorama2DisplaynSave": "spherical", "canvasColor": "black", "forcePlanarScan": False,
}


def default_input(**overrides):
    d = dict(DEFAULT_INPUT)
    d.update(overrides)
    return d


class StageTimes(dict):
    def add(self, name, t0):
        self[name] = self.get(name, 0.0) + (time.perf_counter() - t0)


def _sync():
    _capi.check(_capi.lib.aps_synchronize())


_SIFT_POOL = None


# Host threads / HIP streams of the per-image feature extraction (host images, and resident SURF and FAST views, which the
# measurements below keep view by view; resident SIFT views go in groups, below, with or without NumStrongest / NumUniform).
# Measured on the 64 x 4K scene on several boxes:
# 4, 5, 10, 11, 12, 14 threads give 88-93 ms, 10 the best or tied everywhere; 7-9 threads read 100 ms on some boxes and
# 92 on others (reproducibly per box; the HIP runtime maps streams onto 8 hardware queues), 12 costs the end-to-end
# step's uploads 14 ms.
SIFT_WORKERS_DEFAULT = 10

# Resident SIFT images go to the library in groups of consecutive same-shape views (fm.sift_extract_batch: one launch per pyramid
# plane and per stage for the whole group), a few groups in flight on worker streams of their own, so that the per-keypoint
# kernels of one group run beside the pyramid of another.  A group of G 4K views holds G x 1.24 GB of pyramid (plus 0.13 GB per
# view of candidate lists) in its worker's workspace: 8 views x 3 workers = 33 GB.
# Measured on the 64 x 4K step (median ms per step, three runs each, the per-view parent 162.6-163.6 in the same series):
# 8 views x 3 workers 156.8-158.0, 8 x 2 156.2-159.5, 8 x 4 158.9-159.6, 4 x 4 162.6-163.3, 4 x 6 156.8-157.6, 16 x 2 156.4-159.9,
# 16 x 3 157.0-160.2, 2 x 8 166.0-166.7.
SIFT_GROUP_VIEWS = 8
SIFT_GROUP_WORKERS = 3

# Resident SURF views, with or without NumStrongest / NumUniform, can go in groups too (fm.surf_extract_batch); a group size of 0
# keeps them view by view on the SIFT_WORKERS_DEFAULT streams, and that is the default, because no group setting was faster.
# Measured with scripts/probe/feature_groups_time.py on 64 resident 4K views of the dense synthetic texture (2047 rows per view),
# ms per extraction pass, median (range) of three alternating series of five passes; per-view = the commit before the group entries,
# in the same process: per-view 38.97 (38.29-39.14); 4 views x 2 workers 40.78 (40.52-40.88), 4 x 3 39.73 (39.68-39.76), 4 x 4 39.95
# (39.84-40.31), 8 x 2 41.78 (41.52-43.35), 8 x 3 40.59 (40.31-41.10), 8 x 4 40.95 (40.84-42.70), 16 x 2 42.37 (41.75-43.86), 16 x 3
# 42.25 (41.96-42.73), 16 x 4 43.03 (42.34-43.18).  With NumStrongest = 5000 (above every view's count): per-view 37.79 (37.70-38.35);
# 4 x 2 39.32, 4 x 3 38.22 (38.19-38.40), 4 x 4 39.10, 8 x 2 41.49, 8 x 3 39.89, 8 x 4 39.91, 16 x 2 40.80, 16 x 3 40.64, 16 x 4 40.75.
# Ten streams already keep the device busy: a pass takes 0.6 ms per view, less than the 0.77 ms of kernels a view runs (DESIGN.md
# section 7), so there is no launch gap left to close.  The workers are those of the best setting.
SURF_GROUP_VIEWS = 0
SURF_GROUP_WORKERS = 3

# Resident FAST views without NumStrongest / NumUniform likewise (fm.fast_extract_batch; with either key a FAST selection group is a
# level, there is no group form, and the views go one by one whatever this says).  Default 0, view by view: same probe, NumLevels = 3,
# MinContrast = 0.08 (58 103 rows per view): per-view 39.02 (30.93-44.29); 4 x 2 42.06 (42.01-42.70), 4 x 3 41.61 (41.17-42.19), 4 x 4
# 42.06 (40.05-42.71), 8 x 2 55.38 (52.89-55.71), 8 x 3 55.15 (41.94-55.92), 8 x 4 39.88 (39.10-40.77), 16 x 2 61.27 (55.18-64.99),
# 16 x 3 45.19 (44.79-45.20), 16 x 4 51.66 (42.19-52.85): the best setting is inside the per-view spread.
FAST_GROUP_VIEWS = 0
FAST_GROUP_WORKERS = 4
_GROUP_POOLS = {}  # detector -> the pool of its group workers


def _group_route(input):
    """(detector, batch extractor, views per group, workers) for resident views of this input, or None where they go view by
    view: a detector without a group form, FAST with a selection key, or a group size of 0."""
    det = input.get("detector", "SIFT")
    if det == "SIFT":
        route = (det, fm.sift_extract_batch, SIFT_GROUP_VIEWS, SIFT_GROUP_WORKERS)
    elif det == "SURF":  # (padded: the 128-wide rows the matchers take, as extract_features asks of surf_extract)
        route = (det, lambda *a, **kw: fm.surf_extract_batch(*a, padded=True, **kw), SURF_GROUP_VIEWS, SURF_GROUP_WORKERS)
    elif det == "FAST" and "NumStrongest" not in input and "NumUniform" not in input:
        route = (det, fm.fast_extract_batch, FAST_GROUP_VIEWS, FAST_GROUP_WORKERS)
    else:
        return None
    return route if route[2] > 0 else None


def sift_many(input, images, workers=SIFT_WORKERS_DEFAULT, ready=None):
    """getFeaturePoints for many images — the reference runs this loop as a parfor (loadImages.m:82-99).
    input.detector selects SIFT, SURF, KAZE or FAST (fm.extract_features); the name is kept, it is public.  With FAST, the optional
    input.DescriptorMethod ('FREAK' | 'ORB') and input.CornerMethod ('FAST' | 'Harris') travel with `input` to fm.fast_extract and
    fm.fast_extract_batch on every route below.
    Here a few host threads each drive their own HIP stream (the C ABI is thread-safe with per-thread streams
    and workspaces), so the small-octave launches and the count read-backs of one image overlap with the
    large-octave kernels of another.  Results are returned in input order and are independent of the
    interleaving (every kernel is deterministic).
    ready: optional list of torch CUDA events, one per image: the worker of image k waits for ready[k] (e.g. the end
    of that image's host-to-device copy on a side stream) instead of a device-wide synchronisation, so the uploads of
    later images overlap with the SIFT kernels of earlier ones."""
    global _SIFT_POOL
    import os
    import torch
    from concurrent.futures import ThreadPoolExecutor

    workers = int(os.environ.get("APS_SIFT_WORKERS", workers))

    dev = _capi.is_torch(images[0]) and images[0].is_cuda
    if len(images) <= 1 or workers <= 1:
        if ready is not None:
            for ev in ready:
                ev.synchronize()
        elif dev:
            torch.cuda.synchronize()
        out = [fm.extract_features(input, img, device_out=dev) for img in images]
        _sync()
        return out
    return [f.result() for f in sift_submit(input, images, workers, ready)]


_INIT_LOCK = threading.Lock()


def _init_worker(device):
    """Pool initializer: each worker creates its library context (device binding, stream, events) on its own, one
    worker after the other - ten threads racing through their first HIP calls at once is what rocprofv3 was seen to
    crash under."""
    import os
    with _INIT_LOCK:
        _capi.check(_capi.lib.aps_set_thread_device(int(device)))
        if os.environ.get("APS_SIFT_STREAM_PRIORITY"):  # (-1: the workers' streams on the device's lowest priority level; see bench.py)
            _capi.check(_capi.lib.aps_set_thread_stream_priority(int(os.environ["APS_SIFT_STREAM_PRIORITY"])))
        _capi.check(_capi.lib.aps_synchronize())


def release_device_memory():
    """Hands cached device memory back to the driver: the library's per-thread workspace pools (aps_release_workspace on the
    calling thread and on every thread of the extraction pool - a thread only frees its own blocks) and torch's caching
    allocator.  For a host that is about to start another process on the same GPU, or that has finished a large job: after
    a 256 x 4K stitch the pools hold tens of gigabytes that nothing else can use.  Blocks in use are kept."""
    import threading
    import torch

    _capi.check(_capi.lib.aps_release_workspace())
    for pool in (_SIFT_POOL, *_GROUP_POOLS.values()):
        n = len(getattr(pool, "_threads", ())) if pool is not None else 0
        if not n:
            continue
        gate = threading.Barrier(n)

        def free(_, gate=gate):
            gate.wait(timeout=30)  # one task per pool thread: nobody takes two
            return _capi.lib.aps_release_workspace()

        try:
            for rc in pool.map(free, range(n)):
                _capi.check(rc)
        except threading.BrokenBarrierError:
            pass  # a pool thread was busy: its blocks stay (they are in use or will be reused)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def sift_submit(input, images, workers=SIFT_WORKERS_DEFAULT, ready=None, points_device=False):
    """The asynchronous form of sift_many: one future per image, submitted in input order to the worker pool, so that
    a caller can start matching the first images while the later ones are still being extracted (parallel._match_pass).
    Resident SIFT images are submitted as groups of up to SIFT_GROUP_VIEWS consecutive images of one shape and device
    (fm.sift_extract_batch, which selects per view under input.NumStrongest / input.NumUniform) to SIFT_GROUP_WORKERS threads; the
    futures of a group resolve together.  Resident SURF views, and FAST views without a selection key, take the same route through
    fm.surf_extract_batch / fm.fast_extract_batch when SURF_GROUP_VIEWS / FAST_GROUP_VIEWS is above 0 (_group_route); by default,
    and for host images and FAST with a selection key, every image is a task of its own.
    Each future resolves to (descriptors, keypoints) once that worker's stream has finished the image.
    points_device: resident images only - the keypoints stay on the device (fm.sift_extract)."""
    global _SIFT_POOL
    import os
    import torch
    from concurrent.futures import Future, ThreadPoolExecutor

    workers = max(1, int(os.environ.get("APS_SIFT_WORKERS", workers)))
    dev = _capi.is_torch(images[0]) and images[0].is_cuda
    if dev and ready is None:
        torch.cuda.synchronize()  # the images were produced on torch's stream; worker streams must see them
    route = _group_route(input) if dev else None
    if route:
        # resident views: groups of consecutive images of one shape, one pool task per group, one future per image
        det, extract_batch, group_views, group_workers = route
        if det not in _GROUP_POOLS:
            _GROUP_POOLS[det] = ThreadPoolExecutor(max_workers=group_workers, initializer=_init_worker,
                                                   initargs=(_capi.lib.aps_get_device(),))
        group_pool = _GROUP_POOLS[det]
        groups = []
        for k, img in enumerate(images):
            if groups and len(groups[-1]) < group_views and tuple(images[groups[-1][0]].shape) == tuple(img.shape) \
                    and images[groups[-1][0]].device == img.device:
                groups[-1].append(k)
            else:
                groups.append([k])
        futs = [Future() for _ in images]

        def work_group(ks):
            for k in ks:
                futs[k].set_running_or_notify_cancel()
            try:
                _capi.check(_capi.lib.aps_set_thread_device(images[ks[0]].device.index))
                if ready is not None:
                    for k in ks:
                        ready[k].synchronize()
                res = extract_batch(input, [images[k] for k in ks], device_out=True, points_device=bool(points_device),
                                    compact=len(images) > 96)
                _sync()  # this thread's stream
            except BaseException as e:
                for k in ks:
                    futs[k].set_exception(e)
                return
            for k, r in zip(ks, res):
                futs[k].set_result(r)

        for ks in groups:
            group_pool.submit(work_group, ks)
        return futs
    if _SIFT_POOL is None:
        _SIFT_POOL = ThreadPoolExecutor(max_workers=workers, initializer=_init_worker, initargs=(_capi.lib.aps_get_device(),))
    pool = _SIFT_POOL

    # every worker binds the device of the image it is handed (or the submitting thread's device for host images)
    # instead of inheriting the process-wide default, which is whatever device ANY thread selected last
    here = _capi.lib.aps_get_device()

    def work(k):
        _capi.check(_capi.lib.aps_set_thread_device(images[k].device.index if dev else here))
        if ready is not None:
            ready[k].synchronize()
        r = fm.extract_features(input, images[k], device_out=dev, points_device=bool(dev and points_device), compact=len(images) > 96)
        _sync()  # this thread's stream
        return r

    return [pool.submit(work, k) for k in range(len(images))]


def extract_features(input, images, times=None):
    """loadImages' parfor body (loadImages.m:82-99): one getFeaturePoints per image, descriptors resident."""
    t0 = time.perf_counter()
    descs, kps = [], []
    for d, p in sift_many(input, images):
        descs.append(d)
        kps.append(p)
    if times is not None:
        times.add("features", t0)
    return descs, kps


def match_and_verify(input, descs, kps, seed=0, times=None, pair_subset=None, plots=None):
    """featureMatchingPairwise + imageMatching (main.m:95-107) in CSR form.

    Returns dict(pairs=[(i,j)], models=[3x3 j->i], inliers=[K x 2 index arrays], numMatches n x n).
    plots: an optional dict that receives, for every pair handed to RANSAC (refineMatch's pairs: candidates with at least 4
    matches), {(i, j): {'putative': K x 2, 'inliers': K' x 2}} - the 1-based index lists refineMatch plots under
    input.showKeypointsPlot (imageMatching.m:257-269), before and whatever the acceptance test of :150 says; a pair whose
    model was not found has no inliers."""
    n = len(descs)
    t0 = time.perf_counter()
    if any(isinstance(d, fm.binaryFeatures) for d in descs):  # detector = 'FAST': the batched Hamming matcher, same CSR
        pair_ptr, ii, jj, _ = fm.match_pairwise_binary_csr(descs, input["Ratiothreshold"], input["Matchingthreshold"], True)
    else:
        pair_ptr, ii, jj, _ = fm.match_pairwise_csr(descs, input["Ratiothreshold"], input["Matchingthreshold"], True)
    order = fm.pair_order(n)
    if times is not None:
        times.add("matching", t0)
    t0 = time.perf_counter()
    # top-m candidate selection (imageMatching.m:76-100, im.candidate_positions) straight from the CSR counts
    n_match = np.diff(pair_ptr).astype(np.int64)
    put = np.zeros((n, n), np.int64)
    put[im.pair_index_arrays(n)] = n_match
    pw = im.candidate_positions(n_match, n, int(input["mBrownLowe"]))
    work = [order[p] + (int(pair_ptr[p]), int(pair_ptr[p + 1])) for p in pw[n_match[pw] >= 4].tolist()]  # imageMatching.m:133
    out = {"pairs": [], "models": [], "inliers": [], "numMatches": np.zeros((n, n)), "putative": put}
    if work:
        counts = [e - s for (_, _, s, e) in work]
        wptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        src = np.concatenate([kps[j][jj[s:e].astype(np.int64) - 1] for (_, j, s, e) in work])
        dst = np.concatenate([kps[i][ii[s:e].astype(np.int64) - 1] for (i, _, s, e) in work])
        models, mask, found, ninl = im.ransac_batch_drawn(src, dst, wptr, counts, input, seed)
        for w, (i, j, s, e) in enumerate(work):
            nf = e - s
            ni = int(ninl[w]) if found[w] else 0
            if plots is not None:
                sel = np.nonzero(mask[wptr[w]:wptr[w + 1]])[0] if found[w] else np.zeros(0, np.int64)
                both = np.stack([ii[s:e], jj[s:e]], axis=1).astype(np.int64)
                plots[(i, j)] = {"putative": both, "inliers": both[sel]}
            if ni > 8 + 0.3 * nf:  # imageMatching.m:150
                sel = np.nonzero(mask[wptr[w]:wptr[w + 1]])[0]
                out["pairs"].append((i, j))
                out["models"].append(models[w])
                out["inliers"].append(np.stack([ii[s:e][sel], jj[s:e][sel]], axis=1).astype(np.int64))
                out["numMatches"][i, j] = ni
    if times is not None:
        times.add("image_matching", t0)
    return out


def connected_components(numMatches):
    """graph(numMatches,'upper') + conncomp (imageMatchingPanoramaConComps.m:43-45)."""
    # union-find over the (few hundred) edges; components are numbered by their smallest member, ascending - what
    # scipy.sparse.csgraph.connected_components returns (it was 0.8 ms of argument checking per call for 64 nodes)
    a = np.asarray(numMatches) > 0
    n = a.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    ii, jj = np.nonzero(a)
    for i, j in zip(ii.tolist(), jj.tolist()):
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    labels = np.empty(n, np.int32)
    seen = {}
    for v in range(n):
        r = find(v)
        if r not in seen:
            seen[r] = len(seen)
        labels[v] = seen[r]
    return len(seen), labels


def cameras_from_models(n, pairs, models, num_matches, Ks):
    """Minimal stand-in for the reference's HOST camera initialisation (initializeCameraMatrices.m:332-455:
    maximum spanning tree over the match graph + rotation propagation) for callers that KNOW the intrinsics Ks.
    When they are unknown, use recognize_panoramas / stitch without Ks: they estimate the focal and run the bundle
    adjustment (bundleAdjustment.bundleAdjustmentRKf).
    models[p] maps image-j pixels to image-i pixels for pairs[p] = (i, j): H = K_i R_i R_j' K_j^-1.
    Returns (cameras list or None for unreachable images, seed index)."""
    adj = {k: [] for k in range(n)}
    for p, (i, j) in enumerate(pairs):
        adj[i].append((num_matches[i, j], j, p, False))
        adj[j].append((num_matches[i, j], i, p, True))
    deg = [sum(w for w, *_ in adj[k]) for k in range(n)]
    seed = int(np.argmax(deg))
    import heapq

    # the tree first (it depends on the weights only), then every edge's relative rotation in ONE batched svd: edge by
    # edge the 63 small inv / svd calls of a 64-view set were most of this step's 1.7 ms
    reached = {seed}
    edges = []  # (parent, child, pair, child-is-the-pair's-first-image) in visiting order
    heap = [(-w, seed, nb, p, inv) for (w, nb, p, inv) in adj[seed]]
    heapq.heapify(heap)
    while heap:
        _, a, b, p, inv = heapq.heappop(heap)
        if b in reached:
            continue
        reached.add(b)
        edges.append((a, b, p, inv))
        for (w, nb, pp, inv2) in adj[b]:
            if nb not in reached:
                heapq.heappush(heap, (-w, b, nb, pp, inv2))
    R = {seed: np.eye(3)}
    if edges:
        Kinv = {}
        Ms = []
        for (_, _, p, _) in edges:
            i, j = pairs[p]
            if i not in Kinv:
                Kinv[i] = np.linalg.inv(Ks[i])
            Ms.append(Kinv[i] @ models[p] @ Ks[j])  # ~ R_i R_j'
        U, _, Vt = np.linalg.svd(np.stack(Ms))
        Rall = U @ Vt  # (stacked products and determinants: the per-matrix routines, called once)
        Rall = np.where((np.linalg.det(Rall) < 0)[:, None, None], -Rall, Rall)
        for e, (a, b, p, inv) in enumerate(edges):
            Rij = Rall[e]
            # a == i, b == j: R_j = Rij' R_i ; a == j, b == i: R_i = Rij R_j
            R[b] = Rij.T @ R[a] if not inv else Rij @ R[a]
    cams = [({"K": Ks[k], "R": R[k], "f": float(Ks[k][0, 0]), "noRotation": 0} if k in R else None) for k in range(n)]
    return cams, seed


def straightening(cameras, up_angle_t=(60, 60, 105), theta_t=90):
    """Host step, PP/straightening/straightening.m:74-176: global rotation S that makes the cameras' X axes
    horizontal (Brown-Lowe), R <- R*S, with the reference's skip rules.  3x3 algebra per component."""
    cams = [c for c in cameras if c is not None]
    if len(cams) < 2:
        return cameras
    X = np.stack([c["R"][0, :] for c in cams], axis=1)
    _, _, Vt = np.linalg.svd(X @ X.T)
    up = Vt[-1]
    avgY = np.mean(np.stack([c["R"][1, :] for c in cams], axis=1), axis=1)
    avgY = avgY / np.linalg.norm(avgY)
    if up @ avgY < 0:
        up = -up
    Zsum = np.sum(np.stack([c["R"][2, :] for c in cams], axis=1), axis=1)
    xhat = np.cross(up, Zsum)
    if np.linalg.norm(xhat) < np.finfo(float).eps:
        e1 = np.array([1.0, 0, 0]) if abs(up[0]) <= 0.99 else np.array([0, 0, 1.0])
        xhat = np.cross(up, e1)
    if np.linalg.norm(xhat) < np.finfo(float).eps:
        return cameras
    xhat = xhat / np.linalg.norm(xhat)
    zhat = np.cross(xhat, up)
    if np.linalg.norm(zhat) < np.finfo(float).eps:
        return cameras
    zhat = zhat / np.linalg.norm(zhat)
    S = np.stack([xhat, up, zhat], axis=1)
    theta = np.degrees(np.arccos(np.clip((np.trace(S) - 1) / 2, -1, 1)))
    up_angle = np.degrees(np.arccos(np.clip(abs(up[1]), -1, 1)))
    if up_angle_t[0] < up_angle < up_angle_t[2]:
        return cameras
    if up_angle > up_angle_t[1] and theta > theta_t:
        return cameras
    out = []
    for c in cameras:
        out.append(None if c is None else dict(c, R=c["R"] @ S))
    return out


def _component_ba(input, members, pairs, models, num_matches, keypoints, inliers, image_sizes, evaluator=None):
    """bundleAdjustmentRKf over one connected component (recognizePanoramas.m:135-176): the component's verified pairs,
    their inlier lists and homographies in local indices.  Returns (cameras in member order, seed index into members,
    stats of the bundle adjustment)."""
    from . import bundleAdjustment as ba

    loc = {k: q for q, k in enumerate(members)}
    m = len(members)
    nm = np.zeros((m, m))
    matches = [[None] * m for _ in range(m)]
    tforms = [[None] * m for _ in range(m)]
    for p, (i, j) in enumerate(pairs):
        if i in loc and j in loc:
            a, b = loc[i], loc[j]
            nm[a, b] = num_matches[i, j]
            matches[a][b] = np.asarray(inliers[p], np.int64)
            tforms[a][b] = np.asarray(models[p], np.float64)
            tforms[b][a] = np.linalg.inv(tforms[a][b])
    kps = [np.asarray(keypoints[k].cpu() if _capi.is_torch(keypoints[k]) else keypoints[k], np.float64) for k in members]
    sizes = np.array([[image_sizes[k][0], image_sizes[k][1], 3] for k in members], np.float64)
    cams, seed, stats = ba.bundleAdjustmentRKf(input, nm, matches, kps, sizes, tforms,
                                               **({} if evaluator is None else {"evaluator": evaluator}))
    out = [{k: c[k] for k in ("K", "R", "f", "noRotation") if k in c} for c in cams]
    if stats["noRotation"] or input.get("forcePlanarScan", False):
        for o, c in zip(out, cams):
            o["noRotation"] = 1
            o["H2refined"] = c["H2refined"]
    else:
        for q, c in enumerate(out):
            if not cams[q]["initialized"]:
                out[q] = None  # never reached by the incremental loop
    return out, seed, stats


def recognize_panoramas(n, pairs, models, num_matches, Ks, labels, cameras=None, keypoints=None, inliers=None,
                        image_sizes=None, input=None, ba_info=None):
    """recognizePanoramas.m:70-113 + straightening per panorama (main.m:110-118) over the match graph: every connected
    component with at least two images becomes one panorama with its own cameras and its own reference image.
    The reference runs bundleAdjustmentRKf per component (host code, out of scope); here the cameras are the
    caller's (`cameras`, e.g. from that bundle adjustment) or the host stand-in cameras_from_models, run per component
    from that component's best-connected image.  Components come in conncomp order (by lowest image index).
    With neither `cameras` nor `Ks`, the cameras are estimated per component instead - focal estimation, spanning-tree
    rotations and the incremental bundle adjustment of bundleAdjustmentRKf (bundleAdjustment.py; the normal equations on
    the device) - from `keypoints` (per image), `inliers` (per verified pair, 1-based index pairs as match_and_verify
    returns them), `image_sizes` ((rows, cols) per image) and `input` (default_input's BA keys); one dict of statistics
    per component is appended to `ba_info` when given.  Planar sets (noRotation or forcePlanarScan) keep the chained
    homographies (H2refined = H2seed) and are not straightened.
    Returns a list of dict(members=[global image indices], ref=index INTO members, cameras=[one per member])."""
    labels = np.asarray(labels)
    deg = (np.asarray(num_matches) + np.asarray(num_matches).T).sum(1)
    comps = []
    for c in range(int(labels.max()) + 1 if labels.size else 0):
        members = [int(k) for k in np.nonzero(labels == c)[0]]
        if len(members) < 2:
            continue  # 'Skipping bundle adjustment as only one image found' (recognizePanoramas.m:86-89)
        if cameras is not None:
            cams = [cameras[k] for k in members]
            ref = int(np.argmax(deg[members]))
        elif Ks is None:
            if keypoints is None or inliers is None or image_sizes is None:
                raise ValueError("without cameras or the intrinsics Ks, the bundle adjustment needs keypoints, inliers and "
                                 "image_sizes")
            cams, ref, stats = _component_ba(input or DEFAULT_INPUT, members, pairs, models, np.asarray(num_matches),
                                             keypoints, inliers, image_sizes)
            if not stats["noRotation"] and not (input or {}).get("forcePlanarScan", False):
                cams = straightening(cams)
            if ba_info is not None:
                ba_info.append(dict(stats, members=members))
        else:
            inside = set(members)
            sel = [p for p, (i, j) in enumerate(pairs) if i in inside and j in inside]
            cams_all, seed = cameras_from_models(n, [pairs[p] for p in sel], [models[p] for p in sel], num_matches, Ks)
            cams = straightening([cams_all[k] for k in members])
            ref = members.index(seed)
        comp = keep_reached(members, ref, cams)
        if comp is not None:
            comps.append(comp)
    return comps


def keep_reached(members, ref, cams):
    """One entry of recognize_panoramas' result from a component's cameras: members whose camera is None (never reached by
    the spanning tree or the incremental loop) are dropped and `ref` is renumbered; fewer than two cameras left give None.
    (parallel.stitch_distributed applies the same rule to cameras it received from the rank that estimated them.)"""
    keep = [q for q, cam in enumerate(cams) if cam is not None]
    if len(keep) < 2:
        return None
    if len(keep) != len(members):
        ref = keep.index(ref) if ref in keep else 0
        members = [members[q] for q in keep]
        cams = [cams[q] for q in keep]
    return {"members": members, "ref": ref, "cameras": cams}


def fit_size(h, w, heightLimit, widthLimit):
    """Stage-1 size of resizeImagesToLimits 'fit' (resizeImagesToLimits.m:57-61): isotropic shrink into the box,
    imresize's scalar form gives ceil(s * size); images inside the box keep their size."""
    import math

    sc = min(heightLimit / h, widthLimit / w)
    if not np.isfinite(sc) or sc <= 0:
        sc = 1.0
    return (int(math.ceil(h * sc)), int(math.ceil(w * sc)), sc) if sc < 1 else (int(h), int(w), 1.0)


def resize_per_component(input, local_originals, labels, all_sizes):
    """imageMatchingPanoramaConComps.m:48-56: imagesProcessed(idxs) = resizeImagesToLimits(imagesOriginal(idxs), ...,
    'fit') for every connected component - the same rule as loadImages.m:66-68, applied per panorama: shrink into the
    box, then bring the component's images to ITS common largest size (resizeImagesToLimits.m:49-106).
    local_originals: dict image index -> uint8 image (numpy or CUDA tensor) held by this process; all_sizes: (h, w)
    of EVERY original (the common size of a component depends on members other processes hold).
    Returns dict image index -> resized image of the same kind."""
    from . import imageProcessing as ip

    HL, WL = float(input["heightLimit"]), float(input["widthLimit"])
    labels = np.asarray(labels)
    out = {}
    for c in range(int(labels.max()) + 1):
        idxs = [int(k) for k in np.nonzero(labels == c)[0]]
        orig = [tuple(int(v) for v in all_sizes[k][:2]) for k in idxs]
        too_large = any(h > HL or w > WL for (h, w) in orig)
        if not too_large and len(set(orig)) == 1:
            for k in idxs:
                if k in local_originals:
                    out[k] = local_originals[k]  # all the same size, nothing to do (:49-55)
            continue
        st1 = [fit_size(h, w, HL, WL) for (h, w) in orig]
        common = None
        if len({(a, b) for (a, b, _) in st1}) > 1:
            common = (max(a for (a, _, _) in st1), max(b for (_, b, _) in st1))
        for k, (h1, w1, sc) in zip(idxs, st1):
            if k not in local_originals:
                continue
            a = local_originals[k]  # numpy stays numpy, a CUDA tensor stays resident (aps_imresize_u8 takes either)
            if sc < 1:
                a = ip.imresize(a, sc, "bicubic")
            if common is not None:  # every image of the set, also those already at that size (resizeImagesToLimits.m:100-104)
                a = ip.imresize(a, common, "bicubic")
            out[k] = a
    return out


def rescale_K(K, old_hw, new_hw):
    """Intrinsics of an image after imresize from old_hw to new_hw = (rows, cols): pixel x scales with the column count,
    y with the row count (imresize may be anisotropic when a set is brought to a common size).  The reference has no
    such step - its cameras come out of the bundle adjustment on the resized images; this serves the host stand-in,
    which takes the intrinsics as an input."""
    sy, sx = new_hw[0] / old_hw[0], new_hw[1] / old_hw[1]
    if sx == 1.0 and sy == 1.0:
        return np.asarray(K, np.float64)
    return np.diag([sx, sy, 1.0]) @ np.asarray(K, np.float64)


def imageMatchingPanoramaConComps(input, images_original, images_processed, descs, kps, seed=0, times=None, plots=None):
    """[allMatchesRefined, numMatches, initialTforms, imagesProcessed, ..., concomps] =
    imageMatchingPanoramaConComps(...) (imageMatchingPanoramaConComps.m:39-91) in CSR form: first-pass matching and
    verification, connected components, and - with input.resizeImage and input.resizeImagePanoramaCluster set and
    more than one component - the second pass on images resized per component.
    plots: match_and_verify's; it holds the lists of the final pass.
    Returns (result dict of match_and_verify, images_processed, descs, kps, ncomp, labels, second_pass: bool)."""
    res = match_and_verify(input, descs, kps, seed, times, plots=plots)
    ncomp, labels = connected_components(res["numMatches"])
    second = int(input.get("resizeImage", 0)) == 1 and int(input.get("resizeImagePanoramaCluster", 0)) == 1 and ncomp > 1
    if second:
        sizes = [(int(im_.shape[0]), int(im_.shape[1])) for im_ in images_original]
        resized = resize_per_component(input, dict(enumerate(images_original)), labels, sizes)
        images_processed = [resized[k] for k in range(len(images_original))]
        descs, kps = extract_features(input, images_processed, times)
        if plots is not None:
            plots.clear()
        res = match_and_verify(input, descs, kps, seed, times, plots=plots)
    return res, images_processed, descs, kps, ncomp, labels, second


def shift_K(K, origin):
    """Intrinsics in the frame of a view with origin (x0, y0): its pixel (1, 1) is the old pixel (x0, y0), so
    cx' = cx - (x0 - 1), cy' = cy - (y0 - 1)."""
    K = np.array(K, np.float64)
    K[0, 2] -= origin[0] - 1
    K[1, 2] -= origin[1] - 1
    return K


def undistort_prologue(input, images, images_original, Ks, times=None):
    """stitch's first step under input['cameraIntrinsics']: ip.undistortImage on every image (resident images stay resident)
    and on every image of images_original when given, into input['undistortOutputView'] ('valid' by default).
    Returns (images, images_original, Ks carried into the new frames or None, the per-image records of info['undistort'])."""
    from . import imageProcessing as ip

    t0 = time.perf_counter()
    lenses = input["cameraIntrinsics"]
    if isinstance(lenses, ip.cameraIntrinsics):
        lenses = [lenses] * len(images)
    if len(lenses) != len(images) or not all(isinstance(L, ip.cameraIntrinsics) for L in lenses):
        raise ValueError("input.cameraIntrinsics: one cameraIntrinsics, or a list with one per image")
    view = input.get("undistortOutputView", "valid")
    out, records = [], []
    for img, L in zip(images, lenses):
        J, origin = ip.undistortImage(img, L, view)
        out.append(J)
        records.append({"origin": origin, "size": (int(J.shape[0]), int(J.shape[1])), "K": shift_K(L.K, origin)})
    if images_original is not None:
        if len(images_original) != len(images):
            raise ValueError("images_original must have one image per image")
        images_original = [ip.undistortImage(img, L, view)[0] for img, L in zip(images_original, lenses)]
    if Ks is not None:
        Ks = [shift_K(K, r["origin"]) for K, r in zip(Ks, records)]
    if times is not None:
        times.add("undistort", t0)
    return out, images_original, Ks, records


def stitch(input, images, Ks=None, cameras=None, tile=(2048, 2048), seed=0, device_out=True, profile=False,
           images_original=None):
    """main.m for one dataset.  images: list of uint8 H x W x 3 (torch CUDA tensors stay resident).
    cameras: optional externally supplied cameras (e.g. from the reference's own bundle adjustment);
    otherwise they are initialised on the host from the verified homographies and the intrinsics Ks.  With neither,
    they are estimated (focal estimation + bundle adjustment, recognize_panoramas); info then holds
    times['bundle_adjustment'] and 'ba': per component the estimated focal, the initial and final RMSE, the LM's
    normal-equation evaluations and noRotation.
    Every connected component of at least two images is rendered (displayPanorama.m:88-116).  With
    input['showPanoramaImgsNums'] and input['showCropBoundingBox'] both true, info['annotated'] holds, per component, the
    panorama with the images' outlines and numbers (renderPanorama's second output, drawn on the device).
    With input['showKeypointsPlot'] true, info['match_plots'] holds {(i, j): {'original', 'putative', 'inliers'}}, the three
    pictures refineMatch shows for a pair handed to RANSAC (im.matchPlots on the final pass's images; resident with device_out),
    info['match_plot_lists'] the index lists they were drawn from and info['keypoints'] the points those index; over
    input['keypointsPlotPairs'] when given (a pair RANSAC never saw is a ValueError), over all those pairs otherwise.  When
    the pictures would exceed input['keypointsPlotLimitBytes'] (default 2^31) the call raises ValueError before drawing any.
    The panoramas and every other entry of info are the same with and without the flag.
    With input['cameraIntrinsics'] (one imageProcessing.cameraIntrinsics for all images, or a list with one per image; the key
    is not in DEFAULT_INPUT) every image, and every image of images_original, is undistorted first (undistort_prologue) into
    the view input['undistortOutputView'] ('valid' by default, so that no fill pixel reaches the blend; or 'same'), and
    everything after runs on the undistorted images: Ks, when given, are carried into the new frame, and
    info['images_processed'], info['keypoints'], the match plots and the cameras are in the undistorted frame.
    info['undistort'] lists per image {'origin': (x0, y0), 'size': (h, w), 'K': the lens' K in the new frame}, and
    times['undistort'] is added.  Without the key nothing of this runs and the results are what they were.
    Returns (panoramas [one per component, in component order], info dict with per-stage wall times in seconds)."""
    times = StageTimes()
    plots = {} if input.get("showKeypointsPlot") else None
    n = len(images)
    undistorted = None
    if "cameraIntrinsics" in input:
        images, images_original, Ks, undistorted = undistort_prologue(input, images, images_original, Ks, times)
    descs, kps = extract_features(input, images, times)
    first_hw = [(int(im_.shape[0]), int(im_.shape[1])) for im_ in images]
    first_counts = [len(k) for k in kps]
    res, images, descs, kps, ncomp, labels, second = imageMatchingPanoramaConComps(
        input, images if images_original is None else images_original, images, descs, kps, seed, times, plots=plots)
    sizes = [(int(im_.shape[0]), int(im_.shape[1]), 3) for im_ in images]
    if plots is not None:  # refused before the cameras and the render, which cost more than the check
        plot_pairs = _match_plot_pairs(input, plots, sizes)
    if second and Ks is not None:  # the intrinsics follow the per-component resize
        Ks = [rescale_K(K, first_hw[k], sizes[k][:2]) for k, K in enumerate(Ks)]
    t0 = time.perf_counter()
    ba_info = None
    if Ks is None and cameras is None:  # estimate the cameras: focal estimation + bundle adjustment per component
        ba_info = []
        comps = recognize_panoramas(n, res["pairs"], res["models"], res["numMatches"], None, labels, None, keypoints=kps,
                                    inliers=res["inliers"], image_sizes=[s[:2] for s in sizes], input=input, ba_info=ba_info)
        times.add("bundle_adjustment", t0)
    else:
        comps = recognize_panoramas(n, res["pairs"], res["models"], res["numMatches"], Ks, labels, cameras)
        times.add("host_cameras", t0)
    panos = []
    t0 = time.perf_counter()
    opts = {"anglePower": 2, "blending": input["blending"], "pyrLevels": input["bands"], "pyrSigma": input["MBBsigma"],
            "canvasColor": input["canvasColor"], "tile": tile, "cropBorder": bool(input.get("cropBorder", True))}  # displayPanorama.m:101
    if input.get("multibandWeights") is not None:  # 'tent' / 'maxweight' (renderPanorama.multiband_weights)
        opts["multibandWeights"] = input["multibandWeights"]
    annotate = bool(input.get("showPanoramaImgsNums")) and bool(input.get("showCropBoundingBox"))
    if annotate:  # displayPanorama.m:109-110; the panoramas are the same bytes with and without
        opts.update(showPanoramaImgsNums=True, showCropBoundingBox=True)
    annotated = []
    for c in comps:
        members = c["members"]
        pano, ann = rp.renderPanorama(input, [images[k] for k in members], [sizes[k] for k in members],
                                      c["cameras"], input["panorama2DisplaynSave"], c["ref"], opts,
                                      device_out=device_out)
        panos.append(pano)
        annotated.append(ann)
    _sync()
    times.add("render", t0)
    cams = [None] * n
    for c in comps:
        for k, cam in zip(c["members"], c["cameras"]):
            cams[k] = cam
    info = {"times": dict(times), "n_features": [len(k) for k in kps], "n_pairs_verified": len(res["pairs"]),
            "n_components": int(ncomp), "putative": res["putative"], "result": res, "cameras": cams,
            "components": comps, "labels": labels, "second_pass": bool(second), "n_features_first_pass": first_counts,
            "images_processed": images}
    if ba_info is not None:
        info["ba"] = ba_info
    if undistorted is not None:
        info["undistort"] = undistorted
    if annotate:
        info["annotated"] = annotated
    if plots is not None:
        info["match_plot_lists"] = {p: plots[p] for p in plot_pairs}
        info["keypoints"] = kps  # (what the lists index: the final pass's keypoints, one n x 2 (x, y) array per image)
        info["match_plots"] = _match_plots(images, kps, plots, plot_pairs, device_out)
    return panos, info


def _match_plot_pairs(input, plots, sizes):
    """The pairs input.showKeypointsPlot is served for: input.keypointsPlotPairs, or every pair RANSAC saw; checked against
    those pairs and against input.keypointsPlotLimitBytes."""
    asked = input.get("keypointsPlotPairs")
    pairs = list(plots) if asked is None else [(int(i), int(j)) for i, j in asked]
    unseen = [p for p in pairs if p not in plots]
    if unseen:
        raise ValueError(f"keypointsPlotPairs: no RANSAC ran on {unseen} (0-based (i, j), i < j, candidate pairs with at least 4 matches)")
    need, limit = im.match_plot_bytes(sizes, pairs), int(input.get("keypointsPlotLimitBytes", 2 ** 31))
    if need > limit:
        raise ValueError(f"showKeypointsPlot: the pictures of {len(pairs)} pairs take {need} bytes, above keypointsPlotLimitBytes = "
                         f"{limit}; name the pairs to plot in keypointsPlotPairs")
    return pairs


def _match_plots(images, kps, plots, pairs, device_out):
    """im.matchPlots for stitch: resident pictures with device_out, numpy arrays otherwise, whatever kind the images are."""
    import torch

    used = sorted({k for p in pairs for k in p})  # (only the images of the plotted pairs move)
    if device_out:
        views = {k: images[k] if _capi.is_torch(images[k]) and images[k].is_cuda else torch.as_tensor(np.asarray(images[k])).cuda()
                 for k in used}
    else:
        views = {k: images[k].cpu().numpy() if _capi.is_torch(images[k]) else np.asarray(images[k]) for k in used}
    return im.matchPlots(views, kps, {p: plots[p]["putative"] for p in pairs}, {p: plots[p]["inliers"] for p in pairs}, pairs)
