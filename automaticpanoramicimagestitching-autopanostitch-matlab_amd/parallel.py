"""Multi-GPU sharding of the hot path: one process per GPU, torch.distributed (backend "nccl" == RCCL over
xGMI on ROCm; "gloo" on CPU for the tests, and on device tensors through host staging - see _staged()).

What shards how:
  1. SIFT            : images are independent (loadImages.m:82-99) -> image i on rank i % world.
  2. exchange        : ONE all-gather of the descriptor blocks (+ a small one for keypoint coordinates and
                       counts) so every rank holds all F x 128 descriptors.
  3. match           : the pair list of featureMatchingPairwise.m:48 is partitioned over ranks, balanced by
                       N_i * N_j; the match index lists are all-gathered on the device (a few MB) and stay there.
  4. RANSAC          : candidate pairs (imageMatching.m:121) round-robin over ranks; draws are keyed by the
                       global pair index so the result does not depend on the sharding; the fixed-size verdicts
                       (model, found, inlier count) are combined with one all-reduce.
  5. host segment    : every rank repeats the tiny deterministic graph/camera step (no broadcast needed):
                       connected components, one camera set + reference per component (recognizePanoramas.m).
                       Without intrinsics the cameras are ESTIMATED instead (bundleAdjustmentRKf / bundleAdjustmentH,
                       normal equations on the device): the RANSAC inlier lists are all-gathered once, every component
                       is estimated by one rank (balanced by members^2) and its packed result is broadcast.
  6. render          : source images are all-gathered once (uint8, started before SIFT); EVERY connected component
                       is rendered (displayPanorama.m:88-116): components first (whole panoramas to ranks, balanced
                       by canvas area, when there are at least as many as ranks), tiles second (tiles t % world of
                       one canvas, renderPanorama.m:342-406, when there are fewer).  A planar set is composited whole
                       by the rank that estimated it (no tiles).
There is no other collective on the data path.
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch
import torch.distributed as dist


def world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


def _multi(ws):
    """True when the multi-rank code path has to run.  APS_PARALLEL_FORCE_COLLECTIVES=1 (a test hook) takes that path with a
    ONE-rank process group too: every collective, hand-over and stream wait of the N > 1 driver then runs on the real
    backend (RCCL refuses two ranks on one GPU, so this is how a one-GPU box exercises the nccl calls)."""
    return ws > 1 or (os.environ.get("APS_PARALLEL_FORCE_COLLECTIVES") == "1" and dist.is_available() and dist.is_initialized())


def _staged(t=None):
    """gloo moves host memory: collectives on device tensors are staged through the host (used by the 2-rank
    equality test, which runs both ranks on one GPU; production is "nccl" = RCCL, device to device)."""
    return dist.get_backend() == "gloo" and (t is None or t.is_cuda)


def _all_gather_into(out, inp, async_op=False):
    if _staged(inp):
        ho = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(ho, inp.cpu())
        out.copy_(ho)
        return None
    return dist.all_gather_into_tensor(out, inp, async_op=async_op)


def _all_reduce(t, op=None):
    op = dist.ReduceOp.SUM if op is None else op
    if _staged(t):
        h = t.cpu()
        dist.all_reduce(h, op=op)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=op)
    return t


def _broadcast(t, src):
    if _staged(t):
        h = t.cpu()
        dist.broadcast(h, src)
        t.copy_(h)
    else:
        dist.broadcast(t, src)
    return t


def _gather(t, parts, dst):
    if _staged(t):
        hp = [torch.empty(t.shape, dtype=t.dtype) for _ in parts] if parts is not None else None
        dist.gather(t.cpu(), hp, dst=dst)
        if parts is not None:
            for a, b in zip(parts, hp):
                a.copy_(b)
    else:
        dist.gather(t, parts, dst=dst)


def _is_cuda_tensor(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def shard_indices(n, world_size, rank):
    """Image i lives on rank i % world (block-cyclic keeps pixel counts balanced for equal-size images)."""
    return [i for i in range(n) if i % world_size == rank]


def partition_weighted(weights, world_size):
    """Longest-processing-time greedy partition of items with the given costs; returns owner[item]."""
    order = np.argsort(-np.asarray(weights, np.float64), kind="stable")
    load = np.zeros(world_size)
    owner = np.zeros(len(weights), np.int64)
    for it in order:
        r = int(np.argmin(load))
        owner[it] = r
        load[r] += weights[it]
    return owner


def partition_pairs_blocked(pairs, weights, n, world_size, scatter=False):
    """Owner of every image pair for the matching stage.  The matcher prepares every descriptor set a rank's pairs touch
    (a fixed cost per image and rank), so the pairs are dealt in BLOCKS of the pair matrix instead of one by one: images
    are cut into ceil(sqrt(2 * world)) groups, the pairs are walked group-pair by group-pair (stable inside one), and the
    walk is cut into `world` contiguous segments of equal total weight.  A rank then touches the images of one or two
    group pairs (at 8 ranks and 64 views: ~32-48 of them instead of all 64); the balance is that of a prefix-sum cut: within
    one pair's weight of even.  The result depends on (pairs, weights, n, world) only - every rank computes the same.
    scatter (off): the groups are drawn by a fixed pseudo-random permutation of the images instead of by index ranges.
    The weights N_i N_j are what the proof pass costs; the survivor pass costs what the pairs OVERLAP, which nobody knows
    yet - but image sets come in capture order, neighbours in index overlap, and index-range groups put most overlapping
    pairs into the diagonal blocks.  Measured on the 64 x 4K scene at 8 ranks (scripts/probe/probe_rank_costs.py,
    profiles/r04h_rank_costs.txt): overlapping pairs per rank 33-97 -> 55-79, slowest rank 13.2 -> 12.9 ms, descriptor
    sets per rank 25-42 -> 28-48: the proof pass is 2/3 of a rank's matching whatever its pairs overlap, so the spread of
    the survivor pass is worth 2 % and costs preparation; index ranges stay the default."""
    P = len(pairs)
    owner = np.zeros(P, np.int64)
    if world_size <= 1 or P == 0:
        return owner
    nb = int(np.ceil(np.sqrt(2.0 * world_size)))
    B = max(1, -(-n // nb))
    arr = np.asarray(pairs, np.int64).reshape(P, 2)
    if scatter:
        place = np.empty(n, np.int64)
        place[np.random.RandomState(20240 + n).permutation(n)] = np.arange(n)
        ga, gb = place[arr[:, 0]] // B, place[arr[:, 1]] // B
    else:
        ga, gb = arr[:, 0] // B, arr[:, 1] // B
    key = np.minimum(ga, gb) * (nb + 1) + np.maximum(ga, gb)
    walk = np.argsort(key, kind="stable")
    w = np.asarray(weights, np.float64)[walk]
    total = float(w.sum())
    if total <= 0:
        owner[walk] = np.arange(P) * world_size // P
        return owner
    mid = np.cumsum(w) - 0.5 * w  # a pair belongs to the segment its midpoint falls into
    owner[walk] = np.minimum((mid * world_size / total).astype(np.int64), world_size - 1)
    return owner


def allgather_ragged(local, group=None):
    """All-gather of per-rank tensors whose first dimension differs: one count exchange + ONE padded
    all-gather.  Returns the list of per-rank tensors (on the same device as `local`)."""
    ws, _ = world()
    if not _multi(ws):
        return [local]
    n_local = torch.tensor([local.shape[0]], dtype=torch.int64, device=local.device)
    cnt_all = torch.zeros(ws, dtype=torch.int64, device=local.device)
    _all_gather_into(cnt_all, n_local)
    counts = [int(c) for c in cnt_all.cpu().tolist()]
    m = max(max(counts), 1)
    pad = torch.zeros((m,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    out = torch.empty((ws * m,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    _all_gather_into(out, pad)
    out = out.view((ws, m) + tuple(local.shape[1:]))
    return [out[r, : counts[r]] for r in range(ws)]


def gather_by_owner(local_items, owner_of, n, make_tensor, split_sizes_local):
    """Generic helper: every rank holds some of n ragged items; after the call every rank holds all of them.
    local_items: dict idx -> tensor [len_i, ...]; owner_of(idx) -> rank.  Items of one rank are concatenated
    in ascending idx order, exchanged with allgather_ragged, and split again with the all-gathered lengths."""
    ws, rank = world()
    mine = sorted(local_items)
    lens = torch.zeros(n, dtype=torch.int64)
    for i in mine:
        lens[i] = local_items[i].shape[0]
    dev = make_tensor.device
    lens = lens.to(dev)
    if _multi(ws):
        _all_reduce(lens)
    lens = lens.cpu().tolist()
    cat = torch.cat([local_items[i] for i in mine]) if mine else make_tensor[:0]
    parts = allgather_ragged(cat)
    out = [None] * n
    for r in range(ws):
        off = 0
        for i in range(n):
            if owner_of(i) == r:
                out[i] = parts[r][off: off + lens[i]]
                off += lens[i]
    return out


def exchange_items(local_ids, local_arrays, n_items, owner_of, width, dtype, dev):
    """Every rank owns some of n_items ragged numpy arrays ([len_i, width]); returns the list of all n_items
    arrays on every rank.  One all-reduce of the lengths + ONE padded all-gather of the concatenated payload
    (no per-item tensors)."""
    ws, rank = world()
    if not _multi(ws):
        out = [None] * n_items
        for i, a in zip(local_ids, local_arrays):
            out[i] = a
        return out
    lens = torch.zeros(n_items, dtype=torch.int64)
    for i, a in zip(local_ids, local_arrays):
        lens[i] = a.shape[0]
    lens = lens.to(dev)
    _all_reduce(lens)
    lens = lens.cpu().numpy()
    order = np.argsort(np.asarray(local_ids, np.int64), kind="stable") if len(local_ids) else np.zeros(0, np.int64)
    cat = (np.concatenate([local_arrays[k].reshape(-1, width) for k in order]) if len(order)
           else np.zeros((0, width), dtype))
    parts = allgather_ragged(torch.from_numpy(np.ascontiguousarray(cat)).to(dev))
    parts = [p_.cpu().numpy() for p_ in parts]
    out = [None] * n_items
    offs = [0] * ws
    for i in range(n_items):
        r = owner_of(i)
        out[i] = parts[r][offs[r]: offs[r] + lens[i]]
        offs[r] += int(lens[i])
    return out


class ImageGather:
    """The all-gather of the uint8 source images, started early and collected late: the images exist before
    anything is computed, the render needs them at the very end, and the ~1.6 GB (64 x 4K) it moves over xGMI
    would otherwise sit on the critical path between RANSAC and render.  Rank r owns the images i % world == r;
    sizes may differ and a rank may own none (n < world): a small all-reduce of the shapes comes first."""

    def __init__(self, local_images, n, dev=None):
        self.ws, self.rank = world()
        self.n = n
        self.local = local_images
        self.work = None
        if not _multi(self.ws):
            return
        if dev is None:
            dev = next(iter(local_images.values())).device if local_images else torch.device("cuda")
        shp = torch.zeros((n, 3), dtype=torch.int64, device=dev)
        for i, im_ in local_images.items():
            shp[i] = torch.tensor([int(im_.shape[0]), int(im_.shape[1]), int(im_.shape[2]) if im_.dim() == 3 else 1],
                                  dtype=torch.int64, device=dev)
        _all_reduce(shp)
        self.shapes = [tuple(int(v) for v in row) for row in shp.cpu().tolist()]
        per = (n + self.ws - 1) // self.ws  # slots per rank (the last ones may stay empty)
        flat = max(max(h * w * c for (h, w, c) in self.shapes), 1)
        self.send = torch.empty((per, flat), dtype=torch.uint8, device=dev)  # (padding is never read: the shapes are known)
        for slot, i in enumerate(sorted(local_images)):
            v = local_images[i].reshape(-1)
            self.send[slot, : v.numel()] = v
        self.recv = torch.empty((self.ws * per, flat), dtype=torch.uint8, device=dev)
        self.per = per
        self.work = _all_gather_into(self.recv, self.send, async_op=True)

    def sizes(self):
        """(rows, cols) of all n images, known on every rank from the start (the shapes travel before the pixels)."""
        if not _multi(self.ws):
            return [(int(self.local[i].shape[0]), int(self.local[i].shape[1])) for i in range(self.n)]
        return [(h, w) for (h, w, _) in self.shapes]

    def finish(self):
        """Blocks until the collective has completed (idempotent).  Called before the matching stage: the int8 screening
        kernel claims whole CUs (match_screen_i8_kernel), so a collective left running beside it would only time-slice
        against it - and nothing may share a SIMD with its waves."""
        if _multi(self.ws) and self.work is not None:
            self.work.wait()
            self.work = None
            if self.recv.is_cuda:
                torch.cuda.current_stream().synchronize()

    def wait(self):
        if not _multi(self.ws):
            return [self.local[i] for i in range(self.n)]
        self.finish()
        out = []
        for i in range(self.n):
            h, w, c = self.shapes[i]
            out.append(self.recv[(i % self.ws) * self.per + i // self.ws, : h * w * c].reshape(h, w, c))
        return out


class FeatureExchange:
    """The descriptor exchange in chunks that overlap the extraction: image i lives on rank
    i % world in slot i // world; the slots are cut into `rounds` chunks, and as soon as a rank's images of a chunk are
    extracted the chunk is all-gathered (descriptors: one padded collective, keypoints: a second, small one) while the
    worker streams go on with the next chunk.  Per chunk the only host visit is the count exchange (one small
    all-gather), which the main thread waits for while the GPU keeps extracting.  Every rank runs the same rounds, also
    those in which it owns no image.
    futures: dict image index -> future resolving to (descriptors [k,128] float32 tensor, keypoints [k,2] float64
    numpy or tensor); dev: device of the exchanged tensors."""

    def __init__(self, futures, n, dev, rounds=None):
        self.ws, self.rank = world()
        self.n, self.dev = n, dev
        self.per = (n + self.ws - 1) // self.ws
        if rounds is None:
            # a rank's images are extracted APS_SIFT_WORKERS at a time: with no more images than workers they all finish
            # together and chunks have nothing to hide behind - one exchange then (8 ranks x 8 views), else one chunk per
            # batch of workers, four at most (2 ranks x 32 views)
            workers = max(1, int(os.environ.get("APS_SIFT_WORKERS", 10)))
            rounds = min(4, (self.per + workers - 1) // workers)
        rounds = max(1, min(int(rounds), self.per))
        self.chunk = (self.per + rounds - 1) // rounds
        self.rounds = (self.per + self.chunk - 1) // self.chunk
        self.futures = futures
        self.parts = []  # per round: (slot0, nslot, counts [ws, nslot], desc buffer, kps buffer, handles)

    def run(self):
        """Issues every round (blocking on the local futures of each in turn); returns self."""
        ws, rank, C = self.ws, self.rank, self.chunk
        for r in range(self.rounds):
            s0 = r * C
            ns = min(C, self.per - s0)
            mine = [(s, s * ws + rank) for s in range(s0, s0 + ns) if s * ws + rank < self.n]
            got = {s: self.futures[i].result() for (s, i) in mine}
            cnt = torch.zeros(ns, dtype=torch.int64)
            for s, (d, _) in got.items():
                cnt[s - s0] = int(d.shape[0])
            cnt = cnt.to(self.dev)
            cnt_all = torch.empty(ws * ns, dtype=torch.int64, device=self.dev)
            _all_gather_into(cnt_all, cnt)
            counts = cnt_all.cpu().view(ws, ns)  # the one host visit of the round
            m = max(int(counts.max()), 1)
            send_d = torch.empty((ns, m, 128), dtype=torch.float32, device=self.dev)  # (rows past a slot's count are never read)
            send_k = torch.empty((ns, m, 2), dtype=torch.float64, device=self.dev)
            for s, (d, p) in got.items():
                k = int(d.shape[0])
                send_d[s - s0, :k] = d
                send_k[s - s0, :k] = p if torch.is_tensor(p) else torch.from_numpy(np.ascontiguousarray(p))
            # (the futures resolve after their worker's stream has drained; the packing above and the collectives below are
            # ordered by torch's current stream)
            recv_d = torch.empty((ws, ns, m, 128), dtype=torch.float32, device=self.dev)
            recv_k = torch.empty((ws, ns, m, 2), dtype=torch.float64, device=self.dev)
            h1 = _all_gather_into(recv_d.view(ws * ns, m, 128), send_d, async_op=True)
            h2 = _all_gather_into(recv_k.view(ws * ns, m, 2), send_k, async_op=True)
            self.parts.append((s0, ns, counts, recv_d, recv_k, (h1, h2), (send_d, send_k)))
        return self

    def wait(self):
        """(descriptors, keypoints) of all n images on every rank, as views into the gathered chunk buffers."""
        descs, kps = [None] * self.n, [None] * self.n
        for (s0, ns, counts, recv_d, recv_k, handles, _keep) in self.parts:
            for hnd in handles:
                if hnd is not None:
                    hnd.wait()
            for r in range(self.ws):
                for q in range(ns):
                    i = (s0 + q) * self.ws + r
                    if i < self.n:
                        k = int(counts[r, q])
                        descs[i] = recv_d[r, q, :k]
                        kps[i] = recv_k[r, q, :k]
        return descs, kps


def tile_rects(H, W, tile):
    """The tile loop of renderPanorama.m:342-406 / aps_render_tiles: rows outer, columns inner."""
    TH, TW = int(tile[0]), int(tile[1])
    return [(r0, c0, min(TH, H - r0), min(TW, W - c0)) for r0 in range(0, H, TH) for c0 in range(0, W, TW)]


def tile_ranges(H, W, tile, world_size):
    """Contiguous runs of the row-major tile list, one per rank, cut where the cumulative tile AREA passes k / world of
    the canvas (the last tile row and column are partial): [(begin, end)] * world.  A rank's tiles are neighbours, so its
    render converts only the views under its band of the canvas (64 x 4K on 8 ranks: ~20 of 64, where tiles dealt
    t % world met 47 - profiles/r04b_rank_costs.txt) and its output is ~one rectangle."""
    rects = tile_rects(H, W, tile)
    area = np.cumsum([ht * wt for (_, _, ht, wt) in rects], dtype=np.float64)
    cuts = [0]
    for k in range(1, world_size):
        # first tile whose cumulative area reaches k / world of the total; never before the previous cut
        cuts.append(max(cuts[-1], int(np.searchsorted(area, area[-1] * k / world_size, side="left")) + 1 if len(rects) else 0))
    cuts.append(len(rects))
    cuts = [min(c, len(rects)) for c in cuts]
    return [(cuts[r], max(cuts[r], cuts[r + 1])) for r in range(world_size)]


def gather_tiles_to_root(pano, tile, root=0, ranges=None):
    """Rank r holds the tiles t % world == r of `pano` (H x W x C, zero elsewhere) - or, with `ranges` (tile_ranges), the
    tiles ranges[r][0] <= t < ranges[r][1].  Instead of an all-reduce of the whole canvas, every rank sends exactly its
    tiles to `root` (xGMI is point to point: the transfers of the other ranks run side by side), which copies them into
    place.  Returns pano (complete on root only)."""
    ws, rank = world()
    if not _multi(ws):
        return pano
    H, W = int(pano.shape[0]), int(pano.shape[1])
    rects = tile_rects(H, W, tile)
    C_ = int(pano.shape[2])
    if ranges is not None:
        owner = np.full(len(rects), -1, np.int64)
        for r, (b, e) in enumerate(ranges):
            owner[b:e] = r
        assert (owner >= 0).all(), "tile ranges must cover the canvas"
    else:
        owner = np.arange(len(rects)) % ws
    sizes = [sum(ht * wt * C_ for t, (_, _, ht, wt) in enumerate(rects) if owner[t] == r) for r in range(ws)]
    cap = max(max(sizes), 1)
    buf = torch.zeros(cap, dtype=pano.dtype, device=pano.device)
    off = 0
    for t, (r0, c0, ht, wt) in enumerate(rects):
        if owner[t] == rank:
            m = ht * wt * C_
            buf[off:off + m] = pano[r0:r0 + ht, c0:c0 + wt].reshape(-1)
            off += m
    parts = [torch.empty_like(buf) for _ in range(ws)] if rank == root else None
    _gather(buf, parts, root)
    if rank == root:
        for r in range(ws):
            if r == root:
                continue
            off = 0
            for t, (r0, c0, ht, wt) in enumerate(rects):
                if owner[t] == r:
                    m = ht * wt * C_
                    pano[r0:r0 + ht, c0:c0 + wt] = parts[r][off:off + m].reshape(ht, wt, C_)
                    off += m
    return pano


def submit_features(input, local_images, image_events=None, first=None):
    """Starts the feature extraction of this rank's images on the worker streams and returns at once: the handle that
    stitch_distributed(features=...) accepts instead of extracting itself.  What a loop that stitches set after set calls
    for the NEXT set from the current call's after_matching hook (round 6): from there on the current stitch runs RANSAC
    (three latency-bound launches), replicated host work and the bandwidth-bound render - the extraction of the next set
    fills the gaps between them and shares the memory system with the render (it may NOT run beside the int8 matching
    kernels: they keep their SIMDs to themselves, and the matcher opens with a bandwidth-bound preparation).
    local_images / image_events: as for stitch_distributed.
    first: submit only the first `first` images now (a few worker streams fill the idle chip without crowding the latency-bound
    RANSAC launches of the current set); submit_features_rest(handle) submits the others (e.g. from the after_ransac hook)."""
    from . import pipeline as pl

    ws, _ = world()
    mine_img = sorted(local_images)
    if not mine_img:
        return {"images": [], "futures": [], "resident": False, "rest": None}
    dev = local_images[mine_img[0]].device
    resident = (not _multi(ws)) and dev.type == "cuda" and all(_is_cuda_tensor(local_images[i]) for i in mine_img)
    k = len(mine_img) if first is None else max(0, min(int(first), len(mine_img)))

    def submit(idx):
        ready = [image_events[i] for i in idx] if image_events is not None else None
        return pl.sift_submit(input, [local_images[i] for i in idx], ready=ready, points_device=resident) if idx else []

    handle = {"images": mine_img, "futures": submit(mine_img[:k]), "resident": resident, "rest": None}
    if k < len(mine_img):
        handle["rest"] = lambda: submit(mine_img[k:])
    return handle


def submit_features_rest(handle):
    """Submits the images submit_features(first=...) left out; a handle without any is left alone."""
    if handle is not None and handle.get("rest") is not None:
        rest, handle["rest"] = handle["rest"], None
        handle["futures"] = list(handle["futures"]) + list(rest())
    return handle


def _match_pass(input, local_images, n, seed, times, dev, image_events=None, before_match=None, after_features=None,
                features=None, after_matching=None, after_ransac=None, want_inliers=False):
    """Steps 1-4 on the current images: SIFT on the local shard, the descriptor exchange, the sharded pair matching
    and the sharded RANSAC verification (main.m:88-107 up to imageMatching).  Everything that is exchanged stays on
    the device; the host sees counts, candidate lists and the 3 x 3 models.
    features: the handle of submit_features() for exactly these images (extraction already under way), or None.
    after_matching: optional callable run when the match lists are complete, before candidate selection and RANSAC.
    want_inliers (set when the cameras have to be estimated, and only then): every rank keeps the inlier index pairs of the
    pairs it verified itself, ONE ragged all-gather brings them to every rank, and the result gains "inliers" (per entry of
    "pairs" the K x 2 1-based keypoint indices pipeline.match_and_verify returns) and "keypoints" (host copies of kps_t).
    Returns dict(counts, kps_t, pairs, models, num_matches, n_match, order)."""
    from . import featureMatching as fm
    from . import imageMatching as im

    ws, rank = world()
    submit_features_rest(features)  # (a handle whose second part was never submitted)
    use_global = not int(input.get("matchFeaturesPairwise", 1))  # main.m:95-99
    host_lists = bool(os.environ.get("APS_PARALLEL_HOST_LISTS"))  # A/B switch: lists through the host (round-1 path)
    order = fm.pair_order(n)
    ready = [image_events[i] for i in sorted(local_images)] if image_events is not None else None
    chunk = int(os.environ.get("APS_MATCH_OVERLAP_CHUNK", "0"))
    if not _multi(ws) and not use_global and not host_lists and chunk > 0 and n > chunk and len(local_images) == n:
        kps_t, counts, n_match, ia_d, ib_d, gpos = _features_matched_in_chunks(input, local_images, n, chunk, ready, times, dev)
    else:
        # 1) SIFT on the local shard; 2) the exchange of descriptors and keypoints
        descs, kps_t, counts = _features_exchanged(input, local_images, n, ready, features, before_match, times, dev)
        if after_features is not None:
            after_features()  # caller's hook: the worker streams are idle from here until the next extraction
        # 3) match: pair list partitioned by N_i * N_j; the index lists stay on the device
        n_match, ia_d, ib_d, gpos = _match_lists(input, descs, counts, n, use_global, host_lists, times, dev)
    if after_matching is not None:
        after_matching()  # caller's hook: no int8 kernel runs from here on (e.g. submit_features() for the next set)

    # 4) candidate selection (redundant, deterministic; im.candidate_positions) + RANSAC sharded round-robin
    t0 = time.perf_counter()
    pw = im.candidate_positions(n_match, n, int(input["mBrownLowe"]))
    work = pw[n_match[pw] >= 4].tolist()  # imageMatching.m:133
    rows = list(range(rank, len(work), ws))  # work item k is verified by rank k % ws
    times.add("im_select", t0)
    t0 = time.perf_counter()
    # model (9), found, inliers per candidate pair: a device tensor only when it has to be all-reduced
    rec = (torch.zeros((max(len(work), 1), 11), dtype=torch.float64, device=dev) if _multi(ws)
           else np.zeros((max(len(work), 1), 11), np.float64))
    my_inl = torch.zeros((0, 2), dtype=torch.int32, device=dev) if want_inliers else None
    if rows:
        batch = _ransac_own_pairs(input, kps_t, ia_d, ib_d, gpos, n_match, order, work, rows, n, seed, want_inliers, times, t0)
        if after_ransac is not None:
            after_ransac()
        t0 = time.perf_counter()
        my_inl = _record_own_pairs(rec, my_inl, batch, work, rows, gpos, ia_d, ib_d, dev)
    elif after_ransac is not None:
        after_ransac()  # (a rank without candidate pairs of its own)
    pairs, models, num_matches, verified, vninl = _merge_verdicts(rec, work, n_match, order, n)
    out = {"counts": counts, "kps_t": kps_t, "pairs": pairs, "models": models, "num_matches": num_matches,
           "n_match": n_match, "order": order}
    if want_inliers:
        # the owner (k % ws) and the length (ninl) of every verified pair are known from `rec`: the offsets into the per-rank
        # blocks follow without a second exchange (inlier_slices)
        parts = [p_.cpu().numpy() for p_ in allgather_ragged(my_inl)]
        out["inliers"] = split_inliers(parts, verified, vninl, ws)
        out["keypoints"] = [k.cpu().numpy() for k in kps_t]
    times.add("im_merge", t0)
    return out


def _features_matched_in_chunks(input, local_images, n, chunk, ready, times, dev):
    """The overlap-chunk arm of _match_pass: stages 1 and 3 interleaved.
    One rank, optional (APS_MATCH_OVERLAP_CHUNK=<images per chunk>, default off): feature extraction and matching overlap.
    The pair order is j-major (featureMatchingPairwise.m:48), so the pairs whose later image lies in a chunk of images form
    one contiguous run of it: as soon as a chunk is extracted, that run is matched on this thread's stream while the
    worker streams go on with the next images.  The match lists are the same, only earlier.  Measured on the 64 x 4K
    scene it buys nothing (236.5 ms against 236.8; chunks of 8: 263): the screening kernel has to keep its SIMDs to
    itself (see match_screen_i8_kernel), so the overlap is time slicing at CU granularity, paid for with repeated
    descriptor preparation.  Kept as a switch for scenes with fewer, larger images.
    Takes: all n images local, `ready` events per image.  Returns (kps_t, counts, n_match, ia_d, ib_d, gpos): what
    _features_exchanged and _match_lists return together, without the descriptors.  Collectives: none.  Streams: the match lists
    are written on the library's stream of this thread; kps_t are uploads on torch's.  Times: features, exchange, matching."""
    from . import featureMatching as fm
    from . import pipeline as pl

    order = fm.pair_order(n)
    t0 = time.perf_counter()
    futs = pl.sift_submit(input, [local_images[i] for i in range(n)], ready=ready)
    descs, kps_t, pps, ias, ibs = [], [], [np.zeros(1, np.int64)], [], []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        for i in range(lo, hi):
            d, p = futs[i].result()
            descs.append(d)
            kps_t.append(torch.from_numpy(p).to(dev))
        if hi == n:
            times.add("features", t0)  # wall time until the last image is extracted (part of the matching ran under it)
            t0 = time.perf_counter()
        p0, p1 = lo * (lo - 1) // 2 if lo else 0, hi * (hi - 1) // 2
        if p1 > p0:
            pp_k, ia_k, ib_k, _ = fm.match_pairs_csr(descs, order[p0:p1], input["Ratiothreshold"], input["Matchingthreshold"],
                                                     True, device_out=True)
            pps.append(pp_k[1:] + pps[-1][-1])
            ias.append(ia_k)
            ibs.append(ib_k)
    pp = np.concatenate(pps).astype(np.int64)
    ia_d, ib_d = torch.cat(ias), torch.cat(ibs)
    times.add("exchange", time.perf_counter())
    times.add("matching", t0)
    return kps_t, [int(d.shape[0]) for d in descs], np.diff(pp), ia_d, ib_d, pp[:-1]


def _features_exchanged(input, local_images, n, ready, features, before_match, times, dev):
    """Stages 1 and 2 of _match_pass: SIFT on the local shard, then every rank holds every image's features.
    Takes: this rank's images, the `ready` events in ascending image order (or None), the submit_features() handle (or None).
    Returns (descs, kps_t, counts): per image the resident [k, 128] descriptors, the resident [k, 2] float64 keypoints and k.
    Collectives (more than one rank): FeatureExchange's per round one count all-gather and two padded all-gathers; the
    before_match hook fires here, after the last of them has been waited for.  One rank: none.
    Streams: more than one rank - the device has been synchronised, every stream may read the outputs; one rank - the worker
    streams have drained (the futures resolve after that), host keypoints are uploads on torch's stream.
    Times: features (until the last local image is extracted), exchange (the rest)."""
    from . import pipeline as pl

    ws, _ = world()
    mine_img = sorted(local_images)
    t0 = time.perf_counter()
    if _multi(ws):
        # The exchange runs in chunks BESIDE the extraction (FeatureExchange): a chunk is all-gathered while the worker streams
        # extract the next one, so only the last chunk's collective is left on the critical path.
        if features is not None:
            assert features["images"] == mine_img, "submit_features() was called for other images"
            futs = dict(zip(mine_img, features["futures"]))
        else:
            futs = dict(zip(mine_img, pl.sift_submit(input, [local_images[i] for i in mine_img], ready=ready))) if mine_img else {}
        ex = FeatureExchange(futs, n, dev).run()
        times.add("features", t0)  # (the last local image is extracted; all but the last chunk have been sent)
        t0 = time.perf_counter()
        descs, kps_t = ex.wait()
        if before_match is not None:
            before_match()  # e.g. the early image all-gather: no collective may run beside the matching kernels
        if dev.type == "cuda":
            torch.cuda.synchronize()  # gathered blocks are produced on RCCL's / torch's streams, consumed on the library's
    else:
        ldesc, lkps = {}, {}
        if mine_img:
            # resident images: the keypoints never leave the device (the host copy and the 64 small uploads after the last
            # image were 2 ms of every step); host images: uploaded as soon as their image is done
            resident = dev.type == "cuda" and all(_is_cuda_tensor(local_images[i]) for i in mine_img)
            if features is not None:
                assert features["images"] == mine_img and features["resident"] == resident, "submit_features() was called for other images"
                futs = features["futures"]
            else:
                futs = pl.sift_submit(input, [local_images[i] for i in mine_img], ready=ready, points_device=resident)
            for i, f in zip(mine_img, futs):
                d, p = f.result()
                ldesc[i] = d
                lkps[i] = p if resident else torch.from_numpy(p).to(dev)
        times.add("features", t0)
        t0 = time.perf_counter()
        descs = [ldesc[i] for i in range(n)]
        kps_t = [lkps[i] for i in range(n)]
    counts = [int(d.shape[0]) for d in descs]
    times.add("exchange", t0)
    return descs, kps_t, counts


def _match_lists(input, descs, counts, n, use_global, host_lists, times, dev):
    """Stage 3 of _match_pass: the putative matches of every image pair, as one pair of resident index lists on every rank.
    Takes: all descriptors and counts (on every rank alike).  Returns (n_match, ia_d, ib_d, gpos): the match count of every pair
    in fm.pair_order(n) order, the 1-based keypoint indices of all matches as two resident int32 lists, and where each pair's
    run starts in them.
    Collectives (more than one rank, pairwise matcher): one all-reduce of the counts, then allgather_ragged of the lists (a count
    all-gather and one padded all-gather).  The global matcher and one rank: none.
    Streams: the matcher writes on the library's stream; _sync_lib() drains it before the collective reads the lists on
    torch's / RCCL's.  Times: matching."""
    from . import featureMatching as fm

    ws, rank = world()
    order = fm.pair_order(n)
    t0 = time.perf_counter()
    if _multi(ws):
        w = [float(counts[i]) * float(counts[j]) for (i, j) in order]
        pown = partition_pairs_blocked(order, w, n, ws)
        my = [p for p in range(len(order)) if pown[p] == rank]
        my_pairs = [order[p] for p in my]
    else:  # (one rank: every pair, handed over as the cached array - no per-step walk over 2016 tuples)
        my = slice(None)
        my_pairs = fm.pair_order_array(n)
    if use_global:
        # featureMatchingGlobal (the reference's default, inputs.m:46): pooled exact k-NN + per-query filter.  Every rank
        # holds all descriptors after the exchange and computes the (deterministic) result itself: no further exchange.
        pp, ia_d, ib_d = fm.match_global_csr(descs, input["Ratiothreshold"], int(input.get("k", 4)), device_out=True)
        my = slice(None)
    else:
        pp, ia_d, ib_d, _ = fm.match_pairs_csr(descs, my_pairs, input["Ratiothreshold"],
                                               input["Matchingthreshold"], True, device_out=not host_lists)
        if host_lists:
            ia_d = torch.from_numpy(ia_d.astype(np.int32)).to(dev)
            ib_d = torch.from_numpy(ib_d.astype(np.int32)).to(dev)
    n_match = np.zeros(len(order), np.int64)
    n_match[my] = np.diff(pp)
    if _multi(ws) and not use_global:
        nm = torch.from_numpy(n_match).to(dev)
        _all_reduce(nm)
        n_match = nm.cpu().numpy()
        _sync_lib()  # the lists were written on the library's stream; the collective below reads them on torch's / RCCL's
        parts = allgather_ragged(torch.stack([ia_d, ib_d], 1).contiguous())
        base = np.concatenate([[0], np.cumsum([int(p_.shape[0]) for p_ in parts])])
        allidx = torch.cat(parts)
        ia_d, ib_d = allidx[:, 0], allidx[:, 1]
        # start of pair p in the concatenated lists: rank base + the lengths of that rank's earlier pairs
        gpos = np.zeros(len(order), np.int64)
        for r in range(ws):
            sel = np.nonzero(pown == r)[0]
            if sel.size:
                gpos[sel] = int(base[r]) + np.concatenate([[0], np.cumsum(n_match[sel])[:-1]])
    else:
        gpos = pp[:-1].astype(np.int64)
    times.add("matching", t0)
    return n_match, ia_d, ib_d, gpos


def _ransac_own_pairs(input, kps_t, ia_d, ib_d, gpos, n_match, order, work, rows, n, seed, want_inliers, times, t0):
    """Stage 5 of _match_pass: this rank's RANSAC batch.
    Takes: the resident keypoints and match lists, the candidate work list (positions in the pair order) and `rows`, the
    entries of it this rank verifies (not empty); t0, the start of the im_gather window.
    Returns (cnts, wptr, models, mask, found, ninl): the match count per own pair, their prefix sums, and ransac_batch_drawn's
    host results.  Collectives: none.  Streams: everything runs on the library's stream and has been read back when the call
    returns - the caller fires after_ransac directly after it.  Times: im_gather, im_ransac."""
    from . import imageMatching as im

    mine = [work[k] for k in rows]
    cnts = [int(n_match[p]) for p in mine]
    wptr = np.concatenate([[0], np.cumsum(cnts)]).astype(np.int64)
    # imageMatching.m:121-135 (keypoints{i}(matches(:,1),:), keypoints{j}(matches(:,2),:)) as one library launch over
    # the resident keypoint tables and match lists (a host fancy-index of ~1e6 rows costs tens of milliseconds)
    dst, src = im.gather_match_points(kps_t, ia_d, ib_d, gpos[mine], wptr, [order[p][0] for p in mine],
                                      [order[p][1] for p in mine])
    times.add("im_gather", t0)
    t0 = time.perf_counter()
    # Draws are keyed so that they do not depend on the sharding: by the global pair index - or, when the cameras are to be
    # estimated, by candidate_keys: the estimate starts from these models, and a set of images has to get the same
    # cameras alone and beside other sets, and in a set of its own those of pipeline.stitch.
    keys = mine
    if want_inliers:
        ck = candidate_keys([order[p] for p in work], n)
        keys = [ck[k] for k in rows]
    models, mask, found, ninl = im.ransac_batch_drawn(src, dst, wptr, cnts, input, seed, keys=keys)
    times.add("im_ransac", t0)
    return cnts, wptr, models, mask, found, ninl


def _record_own_pairs(rec, my_inl, batch, work, rows, gpos, ia_d, ib_d, dev):
    """Stage 6 of _match_pass: this rank's rows of the verdict table and, when my_inl is not None, its verified pairs' inliers.
    Takes: `rec` (one row of model (9), found, inlier count per work item; a device tensor when it will be all-reduced),
    `batch` as _ransac_own_pairs returns it.  Writes rec[rows]; returns my_inl: None, or the K x 2 int32 resident keypoint
    indices of the inliers of this rank's verified pairs, in work order.  Collectives: none.  Streams: torch's (one upload and
    one indexed write; one device gather of the match lists, which the RANSAC batch has long finished reading)."""
    cnts, wptr, models, mask, found, ninl = batch
    vals = np.concatenate([models.reshape(len(rows), 9), found.reshape(-1, 1).astype(np.float64),
                           ninl.reshape(-1, 1).astype(np.float64)], axis=1)
    if torch.is_tensor(rec):
        rec[torch.tensor(rows, dtype=torch.int64, device=dev)] = torch.from_numpy(vals).to(dev)
    else:
        rec[rows] = vals
    if my_inl is None:
        return None
    # rows of this rank's verified pairs in work order: mask -> positions in the resident match lists, one device
    # gather; the threshold is the one applied to the all-reduced verdicts (_merge_verdicts), so every rank agrees on who sends
    pos = []
    for q, k in enumerate(rows):
        if found[q] and int(ninl[q]) > 8 + 0.3 * cnts[q]:
            sel = np.nonzero(mask[wptr[q]:wptr[q + 1]])[0]
            if sel.size != int(ninl[q]):
                raise RuntimeError("pair %d: %d mask entries for %d inliers" % (work[k], sel.size, int(ninl[q])))
            pos.append(int(gpos[work[k]]) + sel)
    if pos:
        at = torch.from_numpy(np.concatenate(pos).astype(np.int64)).to(dev)
        my_inl = torch.stack([ia_d[at], ib_d[at]], 1).to(torch.int32).contiguous()
    return my_inl


def _merge_verdicts(rec, work, n_match, order, n):
    """Stage 7 of _match_pass: every rank's verdicts on every rank, and the verified pairs.
    Takes: `rec` with this rank's rows written and zeros elsewhere.  Returns (pairs, models, num_matches, verified, vninl): the
    pairs that pass imageMatching.m:150 in work order, their 3 x 3 models, the n x n inlier counts, and for split_inliers the
    positions of those pairs in the work list with their inlier counts.
    Collectives (more than one rank): one all-reduce of rec.  Streams: torch's; the result is on the host."""
    if torch.is_tensor(rec):
        _all_reduce(rec)  # every row is written by exactly one rank, zero elsewhere
        rec = rec.cpu().numpy()
    pairs, models, num_matches = [], [], np.zeros((n, n))
    verified, vninl = [], []
    if work:
        nf = n_match[np.asarray(work, np.int64)]
        ni = np.where(rec[: len(work), 9] != 0, rec[: len(work), 10].astype(np.int64), 0)
        for k in np.nonzero(ni > 8 + 0.3 * nf)[0].tolist():  # imageMatching.m:150
            i, j = order[work[k]]
            pairs.append((i, j))
            models.append(rec[k, :9].reshape(3, 3).copy())
            num_matches[i, j] = ni[k]
            verified.append(k)
            vninl.append(int(ni[k]))
    return pairs, models, num_matches, verified, vninl


def _sync_lib():
    from . import pipeline as pl

    pl._sync()


# ---- camera estimation without intrinsics: the inlier exchange and the per-component result -------------------------------
def candidate_keys(work_pairs, n):
    """Key of the RANSAC draws of every candidate pair when the cameras are estimated: the pair's position among the
    candidate pairs of ITS OWN connected set of the candidate graph (the work list as edges), in work order.
    The candidate graph is known before RANSAC, on every rank alike.  Image sets that share no candidate pair - the
    panoramas-to-be of a mixed collection - are then verified exactly as each would be alone, whatever else is in the
    collection and wherever its images stand in it; a collection that hangs together gets the positions in the whole work
    list, which are the keys of pipeline.match_and_verify's single batch."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in work_pairs:
        ri, rj = find(int(i)), find(int(j))
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    seen = {}
    keys = []
    for i, _ in work_pairs:
        r = find(int(i))
        keys.append(seen.get(r, 0))
        seen[r] = keys[-1] + 1
    return keys


def inlier_slices(verified, ninl, world_size):
    """Where the inlier rows of every verified pair lie in the per-rank blocks of the inlier all-gather.
    verified: positions (into the RANSAC work list) of the pairs that passed imageMatching.m:150, ascending; ninl: their
    inlier counts; work item k was verified by rank k % world_size, and a rank sends the rows of its verified pairs
    concatenated in work order.  Returns [(rank, begin, end)] in the order of `verified`: nothing but the all-reduced
    verdicts is needed, so no second exchange."""
    offs = [0] * world_size
    out = []
    for k, c in zip(verified, ninl):
        r = int(k) % world_size
        out.append((r, offs[r], offs[r] + int(c)))
        offs[r] += int(c)
    return out


def split_inliers(parts, verified, ninl, world_size):
    """The gathered per-rank inlier blocks (K_r x 2 each) cut into one K x 2 int64 array per verified pair."""
    out = []
    for r, b, e in inlier_slices(verified, ninl, world_size):
        if e > int(parts[r].shape[0]):
            raise ValueError("rank %d sent %d inlier rows, the verdicts announce at least %d" % (r, int(parts[r].shape[0]), e))
        out.append(np.asarray(parts[r][b:e], np.int64))
    return out


# One float64 tensor per connected component carries what its owner estimated:
#   [0] m, number of members   [1] ref (index into the members)   [2] layout version   [3] total length in words
#   m camera records of 30 words: [0] field mask (1 K, 2 R, 4 f, 8 noRotation, 16 H2refined; 0 = the camera is None),
#       [1] f, [2] noRotation, [3:12] K, [12:21] R, [21:30] H2refined, matrices row-major, absent fields zero
#   the statistics: for every name of _STAT_SCALARS two words (tag: 0 absent, 1 None, 2 float, 3 integer; value),
#       lm_stop as 1 + _STAT_STR words (length, -1 = absent; code points), camList and focals as 1 + m words each
#       (length, -1 = absent; values)
# The length depends on m alone, so every rank can size the receive buffer; floats travel as their own bits.
_COMP_VERSION = 1
_CAM_WORDS = 30
_CAM_FIELDS = (("K", 1, 3), ("R", 2, 12), ("H2refined", 16, 21))
_STAT_SCALARS = ("f_init", "noRotation", "evaluations", "rmse_init", "rmse_final", "lm_iterations", "E_init", "E_final",
                 "seconds")
_STAT_STR = 16
_STAT_LISTS = ("camList", "focals")


def component_words(m):
    """Length of the packed result of a component of m images."""
    return 4 + _CAM_WORDS * m + 2 * len(_STAT_SCALARS) + 1 + _STAT_STR + len(_STAT_LISTS) * (1 + m)


def pack_component(cams, ref, stats):
    """(cameras in member order, ref, statistics dict of pipeline._component_ba) -> float64[component_words(m)]."""
    import numbers

    m = len(cams)
    buf = np.zeros(component_words(m), np.float64)
    buf[:4] = (m, int(ref), _COMP_VERSION, buf.size)
    for q, cam in enumerate(cams):
        if cam is None:
            continue
        rec = buf[4 + _CAM_WORDS * q: 4 + _CAM_WORDS * (q + 1)]
        unknown = set(cam) - {"K", "R", "f", "noRotation", "H2refined"}
        if unknown:
            raise KeyError("camera field(s) without a place in the packed layout: %s" % sorted(unknown))
        mask = 0
        if "f" in cam:
            mask |= 4
            rec[1] = cam["f"]
        if "noRotation" in cam:
            mask |= 8
            rec[2] = int(cam["noRotation"])
        for name, bit, at in _CAM_FIELDS:
            if name in cam:
                mask |= bit
                rec[at: at + 9] = np.asarray(cam[name], np.float64).reshape(9)
        rec[0] = mask
    unknown = set(stats) - set(_STAT_SCALARS) - set(_STAT_LISTS) - {"lm_stop"}
    if unknown:
        raise KeyError("statistic(s) without a place in the packed layout: %s" % sorted(unknown))
    at = 4 + _CAM_WORDS * m
    for name in _STAT_SCALARS:
        if name in stats:
            v = stats[name]
            if v is None:
                buf[at] = 1
            elif isinstance(v, numbers.Integral):
                if abs(int(v)) > 2 ** 53:
                    raise ValueError("%s = %d does not fit a float64 word" % (name, int(v)))
                buf[at], buf[at + 1] = 3, int(v)
            else:
                buf[at], buf[at + 1] = 2, v
        at += 2
    buf[at] = -1
    if "lm_stop" in stats:
        s = str(stats["lm_stop"])
        if len(s) > _STAT_STR:
            raise ValueError("lm_stop %r is longer than %d characters" % (s, _STAT_STR))
        buf[at] = len(s)
        buf[at + 1: at + 1 + len(s)] = [ord(ch) for ch in s]
    at += 1 + _STAT_STR
    for name in _STAT_LISTS:
        buf[at] = -1
        if name in stats:
            v = list(stats[name])
            if len(v) > m:
                raise ValueError("%s has %d entries for %d images" % (name, len(v), m))
            buf[at] = len(v)
            buf[at + 1: at + 1 + len(v)] = v
        at += 1 + m
    return buf


def unpack_component(buf):
    """float64[component_words(m)] -> (cameras, ref, statistics): the inverse of pack_component, bit for bit."""
    buf = np.asarray(buf, np.float64)
    m, ref = int(buf[0]), int(buf[1])
    if int(buf[2]) != _COMP_VERSION or int(buf[3]) != buf.size or buf.size != component_words(m):
        raise ValueError("not a packed component result of this layout")
    cams = []
    for q in range(m):
        rec = buf[4 + _CAM_WORDS * q: 4 + _CAM_WORDS * (q + 1)]
        mask = int(rec[0])
        if mask == 0:
            cams.append(None)
            continue
        cam = {}
        if mask & 1:
            cam["K"] = rec[3:12].reshape(3, 3).copy()
        if mask & 2:
            cam["R"] = rec[12:21].reshape(3, 3).copy()
        if mask & 4:
            cam["f"] = float(rec[1])
        if mask & 8:
            cam["noRotation"] = int(rec[2])
        if mask & 16:
            cam["H2refined"] = rec[21:30].reshape(3, 3).copy()
        cams.append(cam)
    stats = {}
    at = 4 + _CAM_WORDS * m
    for name in _STAT_SCALARS:
        tag = int(buf[at])
        if tag:
            stats[name] = None if tag == 1 else int(buf[at + 1]) if tag == 3 else float(buf[at + 1])
        at += 2
    if buf[at] >= 0:
        stats["lm_stop"] = "".join(chr(int(c)) for c in buf[at + 1: at + 1 + int(buf[at])])
    at += 1 + _STAT_STR
    for name in _STAT_LISTS:
        if buf[at] >= 0:
            v = buf[at + 1: at + 1 + int(buf[at])]
            stats[name] = [int(x) for x in v] if name == "camList" else [float(x) for x in v]
        at += 1 + m
    return cams, ref, stats


def component_owners(sizes, world_size):
    """Rank that estimates (and, for a planar set, renders) each component.  The weight (number of members)^2 is a stand-in
    for the cost of the incremental LM - it adds one image per round and every round solves for all cameras so far - not a
    measured cost model."""
    return partition_weighted([float(s) * float(s) for s in sizes], world_size)


def _estimate_components(input, n, res, labels, image_sizes, dev):
    """Step 5 without intrinsics: what pipeline.recognize_panoramas does for Ks = None, sharded by component.  The owner of a
    component runs pipeline._component_ba (focal, spanning-tree rotations, incremental LM with the normal equations on its
    GPU) and the straightening, packs the result and broadcasts it; EVERY rank, the owner included, goes on with the
    unpacked bytes.  A rank first estimates all of its components and only then enters the broadcasts, so the LM loops of
    different ranks run side by side.  One rank, no process group: the same path without the collective.
    Returns (comps as recognize_panoramas returns them, each with "owner"; ba_info: one statistics dict per component)."""
    from . import pipeline as pl

    ws, rank = world()
    multi = _multi(ws)
    labels = np.asarray(labels)
    todo = []
    for c in range(int(labels.max()) + 1 if labels.size else 0):
        members = [int(k) for k in np.nonzero(labels == c)[0]]
        if len(members) >= 2:  # recognizePanoramas.m:86-89
            todo.append(members)
    owners = component_owners([len(m_) for m_ in todo], ws) if multi else np.zeros(len(todo), np.int64)
    packed = {}
    for ci, members in enumerate(todo):
        if int(owners[ci]) != rank:
            continue
        t0 = time.perf_counter()
        cams, ref, stats = pl._component_ba(input, members, res["pairs"], res["models"], np.asarray(res["num_matches"]),
                                            res["keypoints"], res["inliers"], image_sizes)
        if not stats["noRotation"] and not input.get("forcePlanarScan", False):
            cams = pl.straightening(cams)
        packed[ci] = pack_component(cams, ref, dict(stats, seconds=time.perf_counter() - t0))
    comps, ba_info = [], []
    for ci, members in enumerate(todo):
        buf = packed.get(ci)
        if multi:
            t = (torch.from_numpy(buf) if buf is not None else torch.empty(component_words(len(members)), dtype=torch.float64)).to(dev)
            buf = _broadcast(t, int(owners[ci])).cpu().numpy()
        cams, ref, stats = unpack_component(buf)
        ba_info.append(dict(stats, members=members, owner=int(owners[ci])))
        comp = pl.keep_reached(members, ref, cams)
        if comp is not None:
            comps.append(dict(comp, owner=int(owners[ci])))
    return comps, ba_info


def _is_planar(input, cams):
    """renderPanorama.m:78-90: the sets that bypass the ray renderer (the test rp.renderPanorama itself makes)."""
    return bool(cams) and (cams[0].get("noRotation", 0) == 1 or bool(input.get("forcePlanarScan", False)))


def stitch_distributed(input, local_images, n, Ks=None, tile=(2048, 2048), seed=0, cameras=None, pano_root=None,
                       local_originals=None, image_events=None, after_features=None, features=None, after_matching=None,
                       after_ransac=None):
    """The whole stitch with the work sharded over the ranks of the default process group (see module doc).
    local_images: dict image index -> uint8 H x W x 3 CUDA tensor for the indices shard_indices(n, world, rank).
    pano_root: None = every panorama is combined on every rank; r = only rank r receives the tiles / panoramas of the
    others (cheaper; the other ranks return what they rendered themselves).
    local_originals: the unresized originals of the local images; with input.resizeImage and
    input.resizeImagePanoramaCluster set and more than one connected component they are resized per component and the
    extract -> match -> verify chain runs a second time (imageMatchingPanoramaConComps.m:48-91).
    image_events: dict image index -> torch CUDA event that marks the local image as uploaded (end-to-end runs issue
    the host-to-device copies on a side stream; SIFT of image k then waits for event k only).
    after_features: optional callable run once the (first-pass) feature extraction has finished and before the matching
    starts - the point from which the per-image worker streams are idle; a caller that streams the PREVIOUS result to
    the host starts that copy here, where it cannot sit in front of a worker stream's kernels in a shared hardware queue.
    features: the handle submit_features() returned for these very images (their extraction was started earlier, e.g. from
    the previous call's after_matching hook); after_matching: optional callable run when the (first-pass) match lists are
    complete - the point from which no int8 kernel runs any more in this call; after_ransac: the same after this rank's
    RANSAC batch (its three launches are latency-bound: beside a busy chip they take 6 instead of 2.3 ms).
    Ks = None and cameras = None: the cameras are estimated as pipeline.stitch estimates them (focal estimation, bundle
    adjustment, straightening; bundleAdjustmentH for planar sets with input.planarBundleAdjustment), every component on ONE
    rank (_estimate_components) whose result is broadcast; info["ba"] then holds one statistics dict per component (those of
    pipeline.stitch plus "owner" and the owner's wall "seconds") and times["bundle_adjustment"] replaces
    times["host_cameras"].  Planar sets (cameras with noRotation = 1, or input.forcePlanarScan) are rendered whole by one
    rank through the planar compositor, also when `cameras` are given.
    input['showPanoramaImgsNums'] / input['showCropBoundingBox'] are ignored here: no annotated panorama is produced (a
    rank renders a shard of the tiles; annotate the combined result with renderPanorama.annotate_panorama, or use
    pipeline.stitch, whose info['annotated'] carries it).  input['showKeypointsPlot'] is ignored here too, as the annotation
    flags are: no match plots are produced (pipeline.stitch fills info['match_plots'], or call imageMatching.matchPlots).
    Returns (panorama of the component that holds the best-connected image, uint8 H x W x 3 CUDA tensor; info dict
    with info["panoramas"]: one entry per connected component of at least two images, in component order)."""
    from . import pipeline as pl

    if input.get("detector", "SIFT") == "FAST":
        # the descriptor all-gather and the sharded matchers are built for 128-wide float rows
        raise NotImplementedError("stitch_distributed does not take binary descriptors (detector = 'FAST'); use pipeline.stitch")
    if "cameraIntrinsics" in input:
        # the ranks exchange image sizes and intrinsics of the frame the images came in
        raise NotImplementedError("stitch_distributed does not undistort (input.cameraIntrinsics); use pipeline.stitch, or "
                                  "imageProcessing.undistortImage on the images first")
    ws, rank = world()
    dev = next(iter(local_images.values())).device if local_images else torch.device("cuda", torch.cuda.current_device())
    times = pl.StageTimes()

    # 0) the render will need every source image everywhere: start that all-gather now, collect it at step 6
    t0 = time.perf_counter()
    if _multi(ws) and image_events is not None:
        for ev in image_events.values():
            ev.synchronize()  # the early image all-gather reads every local image
        image_events = None
    img_gather = ImageGather(local_images, n, dev)
    times.add("exchange", t0)
    estimate = Ks is None and cameras is None  # no intrinsics: step 5 estimates the cameras and needs the RANSAC inliers
    cam_key = "bundle_adjustment" if estimate else "host_cameras"

    # 1-4) features, exchange, matching, RANSAC
    res = _match_pass(input, local_images, n, seed, times, dev, image_events, before_match=img_gather.finish,
                      after_features=after_features, features=features, after_matching=after_matching, after_ransac=after_ransac,
                      want_inliers=estimate)

    # 5) host segment (redundant on every rank): components, second pass if asked for, cameras per component
    t0 = time.perf_counter()
    ncomp, labels = pl.connected_components(res["num_matches"])
    times.add(cam_key, t0)
    if (int(input.get("resizeImage", 0)) == 1 and int(input.get("resizeImagePanoramaCluster", 0)) == 1 and ncomp > 1
            and local_originals is not None):
        # imageMatchingPanoramaConComps.m:48-91: images resized per component (the common size is that of the
        # component), features re-extracted, everything re-matched and re-verified; the component labels of the
        # FIRST pass are kept (the reference does not recompute them)
        t0 = time.perf_counter()
        local_images, Ks, img_gather = _second_pass_inputs(input, local_images, local_originals, labels, Ks, n, dev, img_gather)
        times.add("exchange", t0)
        res = dict(_match_pass(input, local_images, n, seed, times, dev, before_match=img_gather.finish, want_inliers=estimate),
                   second_pass=True, counts_first_pass=res["counts"])
    t0, ba_info = time.perf_counter(), None
    if estimate:
        comps, ba_info = _estimate_components(input, n, res, labels, img_gather.sizes(), dev)
    else:
        comps = pl.recognize_panoramas(n, res["pairs"], res["models"], res["num_matches"], Ks, labels, cameras)
    times.add(cam_key, t0)

    # 6) render every component
    t0 = time.perf_counter()
    images = img_gather.wait()
    if _multi(ws):
        torch.cuda.synchronize()  # the collective ran on RCCL's stream; the library reads the images on its own
    times.add("exchange", t0)
    t0 = time.perf_counter()
    opts = {"anglePower": 2, "blending": input["blending"], "pyrLevels": input["bands"], "pyrSigma": input["MBBsigma"],
            "canvasColor": input["canvasColor"], "tile": tile, "cropBorder": bool(input.get("cropBorder", True))}  # displayPanorama.m:101
    if input.get("multibandWeights") is not None:  # 'tent' / 'maxweight' (renderPanorama.multiband_weights)
        opts["multibandWeights"] = input["multibandWeights"]
    geos, by_component, comp_owner = _render_plan(input, comps, images, opts)
    panos = []
    for ci, c in enumerate(comps):
        sizes, geo = geos[ci]
        views = [images[k] for k in c["members"]]
        owner = int(comp_owner[ci]) if ci in comp_owner else None
        if geo is None:
            pano = _render_planar(input, c, views, sizes, opts, owner, pano_root, dev)
        else:
            gains = _component_gains(input, c, views, geo, times, dev) if input.get("gainCompensation") else None
            if by_component:
                pano = _render_ray_whole(input, c, views, sizes, opts, gains, geo, owner, pano_root, dev)
            else:
                pano = _render_ray_tiles(input, c, views, sizes, opts, gains, geo, pano_root)
        panos.append(pano)
    times.add("render", t0)
    return _main_panorama(res, comps, panos, ncomp, labels, times, ba_info, n, dev)


def _hw_table(images, n, dev):
    """(n, 2) int64 device table of (rows, cols) of the images a rank holds (dict index -> image), zero rows for the others:
    summed over the ranks it is the table of all n."""
    t = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    for k, im_ in images.items():
        t[k, 0], t[k, 1] = int(im_.shape[0]), int(im_.shape[1])
    return t


def _second_pass_inputs(input, local_images, local_originals, labels, Ks, n, dev, img_gather):
    """The inputs of the second match pass (imageMatchingPanoramaConComps.m:48-91): this rank's originals resized per component.
    Takes: the first pass's local images and image all-gather, the local originals, the first pass's component labels.
    Returns (local_images, Ks, img_gather): the resized local images (resident: no host hop), the intrinsics rescaled to them
    (pipeline.rescale_K; None stays None) and the all-gather of the NEW images, started.
    Collectives (more than one rank): one all-reduce of the originals' sizes, one of the first-pass and new sizes side by
    side, then the first image all-gather is waited for and ImageGather's own (a shape all-reduce, the asynchronous all-gather).
    Streams: torch's throughout."""
    from . import pipeline as pl

    ws, _ = world()
    szs = _hw_table(local_originals, n, dev)
    if _multi(ws):
        _all_reduce(szs)
    first_hw = _hw_table(local_images, n, dev)
    local_images = pl.resize_per_component(input, local_originals, labels, szs.cpu().tolist())
    new_hw = _hw_table(local_images, n, dev)
    if _multi(ws):
        both_hw = torch.cat([first_hw, new_hw], 1)
        _all_reduce(both_hw)
        first_hw, new_hw = both_hw[:, :2], both_hw[:, 2:]
    if Ks is not None:  # the intrinsics follow the per-component resize (pipeline.rescale_K)
        fh, nh = first_hw.cpu().tolist(), new_hw.cpu().tolist()
        Ks = [pl.rescale_K(K, fh[k], nh[k]) for k, K in enumerate(Ks)]
    img_gather.wait()
    return local_images, Ks, ImageGather(local_images, n, dev)


def _render_plan(input, comps, images, opts):
    """Who renders what.  The geometry of every canvas (host, f64) decides the sharding: components to ranks when there are at
    least as many ray-rendered ones as ranks, tiles of each canvas otherwise; a planar set has no ray-render geometry, goes
    whole to one rank and takes no part in that decision.
    Returns (geos, by_component, comp_owner): per component (sizes of its members, canvas geometry or None for a planar
    set); whether ray-rendered components go whole to ranks; component index -> rank for every component rendered whole
    (empty on one rank).  Collectives: none - every rank computes the same plan."""
    from . import renderPanorama as rp

    ws, _ = world()
    mode = input["panorama2DisplaynSave"]
    geos, ray = [], []
    for ci, c in enumerate(comps):
        sizes = [(int(images[k].shape[0]), int(images[k].shape[1]), 3) for k in c["members"]]
        if _is_planar(input, c["cameras"]):
            geos.append((sizes, None))
            continue
        o_ = rp.default_opts(opts, c["cameras"], c["ref"])
        geos.append((sizes, rp.canvas_geometry(c["cameras"], sizes, mode, c["ref"], o_)))
        ray.append(ci)
    by_component = _multi(ws) and len(ray) >= ws
    comp_owner = {}
    if by_component:
        comp_owner = dict(zip(ray, partition_weighted([float(geos[ci][1]["H"]) * float(geos[ci][1]["W"]) for ci in ray], ws)))
    flat = [ci for ci in range(len(comps)) if geos[ci][1] is None]
    if flat and _multi(ws):
        # the rank that estimated the set renders it; sets that came with `cameras` are dealt by the same rule
        dealt = component_owners([len(comps[ci]["members"]) for ci in flat], ws)
        comp_owner.update({ci: comps[ci].get("owner", int(dealt[q])) for q, ci in enumerate(flat)})
    return geos, by_component, comp_owner


def _component_gains(input, c, views, geo, times, dev):
    """gainCompensationRKf between cameras and render (renderPanorama.m:303-330) for one ray-rendered component, on every rank.
    The device sums in an unspecified order, so rank 0's gains are broadcast: every tile must be rendered with the same
    numbers.  Returns the gains (host).  Collectives (more than one rank): one broadcast from rank 0.
    Times: gain_compensation (inside render)."""
    from . import gainCompensation as gc

    tg = time.perf_counter()
    gains = gc.gainCompensationRKf(views, c["cameras"], input["panorama2DisplaynSave"], c["ref"], input, geo)
    if _multi(world()[0]):
        gt_ = torch.from_numpy(np.ascontiguousarray(gains)).to(dev)
        _broadcast(gt_, 0)
        gains = gt_.cpu().numpy()
    times.add("gain_compensation", tg)
    return gains


def _render_planar(input, c, views, sizes, opts, owner, pano_root, dev):
    """A planar scan (renderPanorama.m:78-90), whole, on its owner (one rank: here): no canvas_geometry, no
    gainCompensationRKf; rp.renderPanorama routes to pureNonRotationalPanoramas, which runs gainCompensationH itself when the
    opts ask for it (:584-591).  Returns what _deliver_panorama returns (one rank: the panorama).
    Collectives (more than one rank): _deliver_panorama's.  Streams: the library's stream is drained before the hand-over."""
    from . import pipeline as pl
    from . import renderPanorama as rp

    ws, rank = world()
    popts = dict(opts, **{k: input[k] for k in ("gainCompensation", "sigmaN", "sigmag") if k in input})
    pano = None
    if not _multi(ws) or owner == rank:
        pano, _ = rp.renderPanorama(input, views, sizes, c["cameras"], input["panorama2DisplaynSave"], c["ref"], popts,
                                    device_out=True)
        pl._sync()
    if _multi(ws):
        pano = _deliver_panorama(pano, owner, pano_root, dev)
    return pano


def _render_ray_whole(input, c, views, sizes, opts, gains, geo, owner, pano_root, dev):
    """Components first: a ray-rendered component, whole, on its owner (more than one rank only).  Returns what
    _deliver_panorama returns.  Collectives: _deliver_panorama's.  Streams: the library's stream is drained before the hand-over."""
    from . import pipeline as pl
    from . import renderPanorama as rp

    pano = None
    if owner == world()[1]:
        pano, _ = rp.renderPanorama(input, views, sizes, c["cameras"], input["panorama2DisplaynSave"], c["ref"], opts,
                                    gains=gains, device_out=True, geo=geo)
        pl._sync()
    return _deliver_panorama(pano, owner, pano_root, dev)


def _render_ray_tiles(input, c, views, sizes, opts, gains, geo, pano_root):
    """Tiles second: every rank renders a contiguous, area-balanced run of one canvas's tile list (one rank: all of it).
    Returns the panorama: complete on every rank (pano_root None), or on pano_root only.
    Collectives (more than one rank): one MAX all-reduce of the canvas, or gather_tiles_to_root.
    Streams: the library's stream is drained after the render; the device is synchronised before the collective reads the
    canvas and after it, before the crop reads the combined one."""
    from . import pipeline as pl
    from . import renderPanorama as rp

    ws, rank = world()
    tranges = tile_ranges(int(geo["H"]), int(geo["W"]), rp.effective_tile(opts, geo), ws) if _multi(ws) else None
    subset = ("range",) + tranges[rank] if tranges is not None else None
    pano, _ = rp.renderPanorama(input, views, sizes, c["cameras"], input["panorama2DisplaynSave"], c["ref"], opts,
                                gains=gains, device_out=True, tile_subset=subset, geo=geo,
                                # (runs gathered to a root cover the canvas: nothing outside a rank's run is read)
                                zero_rest=not (tranges is not None and pano_root is not None))
    pl._sync()
    if _multi(ws):
        torch.cuda.synchronize()
        if pano_root is None:
            _all_reduce(pano, dist.ReduceOp.MAX)  # disjoint tiles, zero elsewhere
        else:
            pano = gather_tiles_to_root(pano, rp.effective_tile(opts, geo), pano_root, ranges=tranges)
        torch.cuda.synchronize()
        if opts["cropBorder"] and (pano_root is None or rank == pano_root):
            pano = rp.cropNonzeroBbox(pano, opts["canvasColor"])[0]  # the combined canvas (renderPanorama.m:430-432)
    return pano


def _main_panorama(res, comps, panos, ncomp, labels, times, ba_info, n, dev):
    """The panorama of the component that holds the best-connected image, and stitch_distributed's info dict."""
    main = 0
    if comps:
        deg = (res["num_matches"] + res["num_matches"].T).sum(1)
        best = int(np.argmax(deg))
        main = next((ci for ci, c in enumerate(comps) if best in c["members"]), 0)
    pano = panos[main] if panos else torch.zeros((0, 0, 3), dtype=torch.uint8, device=dev)
    info = {"times": dict(times), "n_features": res["counts"], "n_pairs_verified": len(res["pairs"]),
            "n_components": int(ncomp), "panorama_shape": tuple(int(v) for v in pano.shape) if pano is not None else None,
            "members": comps[main]["members"] if comps else [], "cameras": _scatter_cameras(comps, n),
            "pairs": res["pairs"], "models": res["models"], "components": comps, "panoramas": panos, "labels": labels,
            "second_pass": bool(res.get("second_pass", False)), "n_features_first_pass": res.get("counts_first_pass")}
    if ba_info is not None:
        info["ba"] = ba_info
    return pano, info


def _scatter_cameras(comps, n):
    cams = [None] * n
    for c in comps:
        for k, cam in zip(c["members"], c["cameras"]):
            cams[k] = cam
    return cams


def _deliver_panorama(pano, owner, root, dev):
    """A panorama rendered whole by `owner`: to `root` only (point to point), or to every rank (broadcast) when root
    is None.  Ranks that neither rendered nor receive it return None."""
    ws, rank = world()
    shp = torch.zeros(3, dtype=torch.int64, device=dev)
    if rank == owner:
        shp = torch.tensor([int(v) for v in pano.shape], dtype=torch.int64, device=dev)
    _broadcast(shp, owner)
    shape = tuple(int(v) for v in shp.cpu().tolist())
    if root is None:
        if rank != owner:
            pano = torch.empty(shape, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        _broadcast(pano, owner)
        return pano
    if owner == root:
        return pano if rank == root else None
    if rank == owner:
        torch.cuda.synchronize()
        if _staged(pano):
            dist.send(pano.cpu(), dst=root)
        else:
            dist.send(pano, dst=root)
        return pano
    if rank == root:
        if dist.get_backend() == "gloo":
            h = torch.empty(shape, dtype=torch.uint8)
            dist.recv(h, src=owner)
            return h.to(dev)
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
        dist.recv(out, src=owner)
        return out
    return None
