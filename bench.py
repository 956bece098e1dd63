#!/usr/bin/env python3
"""bench.py — the BASELINE.json metric on MI355X: MPix/s end-to-end stitch (SIFT -> blend), 64 x 4K images.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one full pass of the hot path over the batch of 64 synthetic 4K views (configs[2] of
BASELINE.json): SIFT on every image -> all-pairs exhaustive descriptor matching + Lowe ratio -> batched
RANSAC -> [host: match graph, camera initialisation] -> spherical inverse warp + 5-band multiband blend.
Images are generated on the GPU (seeded, procedural) and are resident in HBM before the timed region.
With N > 1 the SAME 64-image job is sharded over the ranks (strong scaling, see parallel.py).

A plain run does what the headline figure needs and nothing else: it sets up, warms up, times the K steps and prints
ONE JSON line from rank 0 with the contract fields (metric, value, unit, higher_is_better, dtype, ms_per_step, ...).
`--dump-outputs DIR` also writes what the last timed step computed to DIR/<name>.npy (see dump_outputs).

With `--full` the line also carries everything else the bench measures, in legs and passes of their own:
  "roofline"     : the dominant kernel (the int8-MFMA screening pass of the descriptor matcher) against its MFMA
                   roofline, timed with HIP events on the stream the kernel runs on (aps_profile_*);
  "value_end_to_end": the same steps with the images starting in pinned host memory (uploads overlapped with SIFT);
  "value_resident": the same steps without the final device-to-host copy of the panorama;
  "cpu_baseline" : the CPU oracle (oracle/, kind "port") timed on a bounded 2x2-view sample of the same
                   workload on this box's host cores (rank 0, N = 1 only);
and the sequential and gain-compensated series, the per-kernel and per-stage tables, the GPU clock/power sample and the
matcher / SIFT probes.  The --cpu-baseline / --end-to-end / --global-probe / --with-gain switches select among those legs.
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# (the package sets this too on import; here it is certain to precede the process's first HIP call - see <pkg>/__init__.py)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

MFMA_F32_PEAK_TFLOPS = 157.3    # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
MFMA_BF16_PEAK_TFLOPS = 2500.0  # same table, "Peak BF16/FP16 MFMA" dense
MFMA_I8_PEAK_TOPS = 5000.0      # same guide, matrix-core table: I8 32x32x32 = 2x the BF16 rate per clock (dense)
HBM_PEAK_GBS = 8000.0           # same table, HBM3E peak (6.29 TB/s is the measured copy rate)
NX, NY, W, H, FOCAL, OVERLAP, FINEST_PX = 8, 8, 3840, 2160, 8000.0, 0.4, 16.0


def csrc_sha256():
    """Hash of the kernel sources (what scripts/hbm_traffic.sh stamps into the PMC pass it writes)."""
    d = glob.glob(os.path.join(ROOT, "automaticpanoramicimagestitching-autopanostitch-matlab_amd", "csrc", "*.hip")) + \
        glob.glob(os.path.join(ROOT, "automaticpanoramicimagestitching-autopanostitch-matlab_amd", "csrc", "*.h"))
    hsh = hashlib.sha256()
    for f in sorted(d):
        hsh.update(os.path.basename(f).encode())
        hsh.update(open(f, "rb").read())
    return hsh.hexdigest()


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks = GPUs of this node (default: WORLD_SIZE when launched by torch.distributed.run, else 1)")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--grid", type=str, default=f"{NX}x{NY}", help="views as NXxNY (default 8x8 = 64)")
    ap.add_argument("--size", type=str, default=f"{W}x{H}")
    ap.add_argument("--bands", type=int, default=5)
    ap.add_argument("--cpu-baseline", choices=["auto", "off"], default="auto")
    ap.add_argument("--cameras", choices=["estimated", "truth"], default="estimated",
                    help="cameras for the render stage: initialised from the verified homographies (default) "
                         "or the synthetic ground truth")
    ap.add_argument("--matcher", choices=["pairwise", "global"], default="pairwise",
                    help="pairwise = featureMatchingPairwise, all pairs exhaustive (the BASELINE configs[2] workload, default); "
                         "global = featureMatchingGlobal, the reference's default switch (inputs.m:46): pooled exact k-NN (k = 4) "
                         "of all descriptors against themselves + per-query filter")
    ap.add_argument("--save-pano", type=str, default="", help="write a downscaled PNG of the panorama (debug)")
    ap.add_argument("--end-to-end", choices=["auto", "off"], default="auto",
                    help="after the timed steps (inputs resident in HBM -> cropped uint8 panorama in pinned host memory), time the "
                         "same steps with the images starting in pinned host memory (SURVEY 8(d): first byte uploaded -> "
                         "panorama on the host); reported as value_end_to_end next to `value`")
    ap.add_argument("--global-probe", choices=["auto", "off"], default="auto",
                    help="after the timed steps, one pass of the reference's default matcher (featureMatchingGlobal) on the same "
                         "views, reported as global_matcher_probe (off: for profiling runs that want per-step launch counts)")
    ap.add_argument("--pipeline", choices=["auto", "off"], default="auto",
                    help="auto: consecutive steps overlap as the reference's loop over image sets (PP/main.m:83-137) allows - the next "
                         "set's feature extraction starts when the current set's match lists are complete; off: strictly one after the "
                         "other (always reported as value_sequential)")
    ap.add_argument("--with-gain", choices=["auto", "off"], default="auto",
                    help="after the timed steps, time the same steps with input.gainCompensation = 1 (the reference's default, "
                         "PP/inputs.m:94); reported as value_with_gain")
    ap.add_argument("--config", type=int, choices=[0, 1, 3, 4], default=None,
                    help="one of the OTHER BASELINE.json configs on one GPU, as its own JSON line with roofline / cpu_baseline / stages "
                         "(the default invocation is configs[2], the headline): 0 = two-view planar homography stitch, 1 = 20-view ring "
                         "(Grand-Canyon-sized set, spherical, 3 bands), 3 = the 256 x 4K image set, 4 = 500 mixed 2K views -> six "
                         "equirectangular panoramas; synthetic realisations of BASELINE.md section 2 / SURVEY 8(d)")
    ap.add_argument("--reference-defaults", action="store_true",
                    help="with --config 1: the reference's default switches (PP/inputs.m:46,94,99-101): global matcher, gain compensation on, 3 bands")
    ap.add_argument("--gain-compensation", action="store_true",
                    help="also run gainCompensationRKf (device overlap statistics + host solve) before the render; "
                         "off in the headline configuration, which follows BASELINE.json configs[2]")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the extra legs (sequential, gain, end-to-end series, CPU baseline, matcher and SIFT "
                         "probes), kernel timing, rooflines, stage tables and the GPU clock/power sample (off: the headline only)")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (float32 / float64, "
                         "a fixed sample of the panorama; see dump_outputs)")
    return ap.parse_args()


def cpu_baseline(synth, input_, f, bands, pano_area=None):
    """The oracle chain on a bounded sample: a 2x2 block of 4K views (33.2 MPix in), all 6 pairs."""
    import oracle

    w, h = W, H
    imgs, cams = synth.make_scene(2, 2, w, h, f, OVERLAP, device="cuda", finest_px=FINEST_PX)
    imgs = [i.cpu().numpy() for i in imgs]
    t0 = time.perf_counter()
    feats = [oracle.sift(im, input_["Sigma"], input_["NumLayersInOctave"], input_["ContrastThreshold"],
                         input_["EdgeThreshold"]) for im in imgs]
    t_sift = time.perf_counter() - t0
    t0 = time.perf_counter()
    matches = {}
    for j in range(1, 4):
        for i in range(j):
            matches[(i, j)] = oracle.match_features(feats[i][0], feats[j][0], input_["Ratiothreshold"],
                                                    input_["Matchingthreshold"], True, 2)[0]
    t_match = time.perf_counter() - t0
    t0 = time.perf_counter()
    rng = np.random.default_rng(0)
    for (i, j), m in matches.items():
        if len(m) < 4:
            continue
        s = np.stack([rng.permutation(len(m))[:4] + 1 for _ in range(564)]).astype(np.uint32)
        oracle.ransac_homography(feats[j][1][m[:, 1] - 1], feats[i][1][m[:, 0] - 1], s, input_["maxDistance"],
                                 input_["inliersConfidence"], input_["maxIter"])
    t_ransac = time.perf_counter() - t0
    import apsamd
    from importlib import import_module

    rp = import_module(apsamd.__name__ + ".renderPanorama")
    sizes = [(h, w, 3)] * 4
    o = rp.default_opts({"anglePower": 2}, cams, 0)
    geo = rp.canvas_geometry(cams, sizes, "spherical", 0, o)
    t0 = time.perf_counter()
    oracle.render(imgs, cams, geo, (2048, 2048), 2.0, "multiband", bands, 1.0)
    t_render = time.perf_counter() - t0
    total = t_sift + t_match + t_ransac + t_render
    mpix = 4 * w * h / 1e6
    # What the same port would need for the whole 64-view job, modelled from the pieces timed above: SIFT and RANSAC scale
    # with the view / candidate-pair count, the exhaustive matcher with the PAIR count (2016 pairs of ~20k x 20k), the
    # render with the canvas area.
    n_views, n_pairs = NX * NY, NX * NY * (NX * NY - 1) // 2
    n_cand = n_views * 6 // 2
    canvas_ratio = (pano_area / float(geo["W"] * geo["H"])) if pano_area else n_views / 4.0
    t64 = (n_views / 4.0) * t_sift + (n_pairs / 6.0) * t_match + (n_cand / 6.0) * t_ransac + canvas_ratio * t_render
    out = {
        "value": round(mpix / total, 3), "unit": "MPix/s", "cores": int(oracle.NUM_THREADS), "kind": "port",
        "sample": f"2x2 block of the {w}x{h} views ({mpix:.1f} MPix in): oracle SIFT x4 ({t_sift:.1f}s), 6 pairs "
                  f"exhaustive match ({t_match:.1f}s), RANSAC ({t_ransac:.1f}s), spherical render + {bands}-band blend of the "
                  f"{geo['W']}x{geo['H']} canvas ({t_render:.1f}s); all-pairs matching grows quadratically with the "
                  "view count, so the 64-view CPU rate is lower than this sample's (modelled_64_views)",
        "modelled_64_views": {
            "value": round(n_views * w * h / 1e6 / t64, 3), "unit": "MPix/s", "seconds": round(t64, 1),
            "how": f"{n_views}/4 x SIFT sample + {n_pairs}/6 x match sample + {n_cand}/6 x RANSAC sample + "
                   f"{canvas_ratio:.1f} x render sample (canvas area ratio); same {int(oracle.NUM_THREADS)} threads"},
    }
    try:
        out["cfg1_single_thread"] = cpu_cfg1_single_thread(synth)
    except Exception as e:  # a report, never a reason to lose the bench line
        out["cfg1_single_thread"] = {"value": None, "sample": f"failed: {e}"}
    return out


def cpu_cfg1_single_thread(synth):
    """BASELINE.json configs[0] ("MATLAB CPU path with parfor off"): two 1024 x 768 views related by a homography through
    the oracle chain on ONE thread - SIFT x2, exhaustive match, RANSAC, planar-scan composite (two image warps + two
    weight warps + 3-band blend), the chain tests/test_config0_gpu.py compares stage by stage."""
    import oracle

    w, h, f = 1024, 768, 1100.0
    imgs, _ = synth.make_scene(2, 1, w, h, f, 0.55, seed=77, device="cuda", finest_px=4.0)
    imgs = [i.cpu().numpy() for i in imgs]
    prev = int(oracle.NUM_THREADS)
    oracle.set_num_threads(1)
    try:
        t0 = time.perf_counter()
        feats = [oracle.sift(im) for im in imgs]
        m, _ = oracle.match_features(feats[0][0], feats[1][0], 0.6, 1.5, True, 2)
        rng = np.random.default_rng(0)
        s = np.stack([rng.permutation(len(m))[:4] + 1 for _ in range(564)]).astype(np.uint32)
        Hm, _, found, _ = oracle.ransac_homography(feats[1][1][m[:, 1] - 1], feats[0][1][m[:, 0] - 1], s, 5.5, 99.9, 500)
        if not found:
            raise RuntimeError("the cfg1 pair was not verified")
        Hn = Hm / Hm[2, 2]
        c = np.array([[1, 1, 1], [w, 1, 1], [w, h, 1], [1, h, 1.0]]).T
        q = Hn @ c
        xs, ys = np.concatenate([q[0] / q[2], [1, w]]), np.concatenate([q[1] / q[2], [1, h]])
        x0, x1, y0, y1 = xs.min(), xs.max(), ys.min(), ys.max()
        ow, oh = int(np.floor(x1 - x0 + 0.5)), int(np.floor(y1 - y0 + 0.5))
        sx, sy = (x1 - x0) / ow, (y1 - y0) / oh
        tent = np.outer(oracle.tent(h), oracle.tent(w)).astype(np.float32)
        Iw = [oracle.image_warp_h(im.astype(np.float32) / 255.0, T, oh, ow, x0, y0, sx, sy, 0.0) for im, T in zip(imgs, (np.eye(3), Hn))]
        Ww = [np.clip(oracle.image_warp_h(tent, T, oh, ow, x0, y0, sx, sy, 0.0), 0, 1) for T in (np.eye(3), Hn)]
        oracle.multiband_blend(np.stack(Iw), np.stack(Ww), 3, 1.0)
        dt = time.perf_counter() - t0
    finally:
        oracle.set_num_threads(prev)
    mp = 2 * w * h / 1e6
    return {"value": round(mp / dt, 3), "unit": "MPix/s", "cores": 1, "seconds": round(dt, 2),
            "sample": f"2 views {w}x{h} ({mp:.2f} MPix): SIFT x2, exhaustive match ({len(m)} matches), RANSAC homography, "
                      f"planar-scan composite {ow}x{oh} with a 3-band blend; oracle, one thread"}


class GpuStateSampler:
    """Clock and power of THIS rank's GPU while a step runs, read from the amdgpu driver's hwmon files (plain file reads from a
    host thread: no other program is started, no GPU API is touched - a process that has initialised the GPU must not exec).
    The chip is power-limited under the dense int8 stream of the matching stage (1.9-2.0 GHz of 2.4), so two boxes that read
    3 % apart can be told apart by the clock they held.  Nothing here is inside the timed region."""

    def __init__(self, device_index):
        self.files, self.samples, self._stop, self._thr = None, [], False, None
        try:
            want = self._pci_of(device_index)
            for card in sorted(glob.glob("/sys/class/drm/card[0-9]*")):
                if "-" in os.path.basename(card):
                    continue
                pci = os.path.basename(os.path.realpath(os.path.join(card, "device"))).lower()
                fr = glob.glob(os.path.join(card, "device", "hwmon", "hwmon*", "freq1_input"))
                pw = glob.glob(os.path.join(card, "device", "hwmon", "hwmon*", "power1_input")) or \
                    glob.glob(os.path.join(card, "device", "hwmon", "hwmon*", "power1_average"))
                if fr and pw and (want is None or pci == want):
                    self.files = (fr[0], pw[0], pci)
                    if want is not None:
                        break
            if want is None:
                self.files = None  # several cards and no way to tell which one is ours
        except Exception:
            self.files = None

    @staticmethod
    def _pci_of(device_index):
        import ctypes

        buf = ctypes.create_string_buffer(64)
        for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
            try:
                if ctypes.CDLL(name).hipDeviceGetPCIBusId(buf, 64, int(device_index)) == 0:
                    return buf.value.decode().lower()
            except OSError:
                continue
        return None

    def _run(self):
        fr, pw, _ = self.files
        while not self._stop:
            try:
                self.samples.append((time.perf_counter(), int(open(fr).read()) / 1e6, int(open(pw).read()) / 1e6))
            except (OSError, ValueError):
                pass
            time.sleep(0.002)

    def start(self):
        if self.files:
            import threading

            self._thr = threading.Thread(target=self._run, daemon=True)
            self._thr.start()

    def stop(self):
        self._stop = True
        if self._thr:
            self._thr.join()

    def window(self, t_a, t_b):
        sel = [(f, p) for t, f, p in self.samples if t_a <= t <= t_b]
        if not sel:
            return None
        return {"sclk_mhz_median": round(float(np.median([f for f, _ in sel])), 0), "sclk_mhz_min": round(min(f for f, _ in sel), 0),
                "power_w_median": round(float(np.median([p for _, p in sel])), 0), "samples": len(sel)}


def sift_standalone_probe(pl, capi, input_, image):
    """One view through the extraction on ONE stream, its launch sites bracketed by HIP events (outside the timed region): the
    kernels' stand-alone times.  In the timed steps ten streams run side by side and the event intervals of a launch site
    overlap (the `sift_blur` entry sums 5x the stage's wall time), so per-kernel rates of the extraction come from here."""
    from importlib import import_module

    fm = import_module(pl.__name__.rsplit(".", 1)[0] + ".featureMatching")
    best = None
    for _ in range(3):
        capi.profile_enable(1)
        capi.profile_reset()
        d, p_ = fm.sift_extract(input_, image, device_out=True, points_device=True)
        capi.check(capi.lib.aps_synchronize())
        prof = capi.profile_all()
        capi.profile_enable(False)
        best = prof
    h, w = int(image.shape[0]), int(image.shape[1])
    oct_px = 4.0 * h * w * 4.0 / 3.0  # pixels of all octaves of the doubled base
    ms = {k: v[0] for k, v in best.items() if k.startswith("sift_")}
    out = {"ms_per_view": {k: round(v, 4) for k, v in ms.items()}, "features": int(d.shape[0])}
    if ms.get("sift_blur"):
        # six blurs per octave, each reading and writing one plane: 6 x 8 B per octave pixel (+ the base: 3 B in, 4 B out per doubled pixel)
        b = 48.0 * oct_px + 3.0 * h * w + 16.0 * h * w
        out["blur_chain"] = {"algorithmic_bytes": b, "GB/s": round(b / (ms["sift_blur"] * 1e-3) / 1e9, 1),
                             "frac": round(b / (ms["sift_blur"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    if ms.get("sift_extrema"):
        b = 28.0 * oct_px  # the seven Gaussian planes of every octave, once
        out["extrema_sweep"] = {"algorithmic_bytes": b, "GB/s": round(b / (ms["sift_extrema"] * 1e-3) / 1e9, 1),
                                "frac": round(b / (ms["sift_extrema"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    return out


def global_matcher_probe(pl, capi, input_, images):
    """featureMatchingGlobal (the reference's default matcher) on the bench's views: SIFT once (untimed), then three passes of
    the pooled matcher (normalise, screened exact 4-NN, per-query filter); the last is reported (the first two still grow the
    calling thread's workspaces: 202 / 177 / 177 ms in a same-process series, scripts/probe/ab_global.py)."""
    import ctypes
    from importlib import import_module

    fm = import_module(pl.__name__.rsplit(".", 1)[0] + ".featureMatching")
    descs = [d for d, _ in pl.sift_many(input_, images)]
    best = None
    for _ in range(3):
        capi.profile_enable(2)
        capi.profile_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pp, _, _ = fm.match_global_csr(descs, input_["Ratiothreshold"], 4, device_out=True)
        capi.check(capi.lib.aps_synchronize())
        dt = time.perf_counter() - t0
        prof = capi.profile_all()
        capi.profile_enable(False)
        best = (dt, prof, int(pp[-1]))
    rows, surv = ctypes.c_int64(0), ctypes.c_int64(0)
    capi.check(capi.lib.aps_knn_global_screen_stats(ctypes.byref(rows), ctypes.byref(surv)))
    F = float(sum(int(d.shape[0]) for d in descs))
    dt, prof, n_match = best
    ms_screen = prof.get("match_screen_i8_bounds", (0.0, 0))[0]
    return {
        "ms": round(1e3 * dt, 2), "pool_rows": int(F), "matches": n_match,
        "rows_searched_share": round(surv.value / rows.value, 4) if rows.value else None,
        "kernels_ms": {k: round(v[0], 3) for k, v in prof.items() if v[0] > 0.05},
        # the int8 proof pass streams every ordered pair of different images once: 2 * 128 * (F^2 - sum n_i^2) integer MACs x 2
        "screen_tops": round(2.0 * 128.0 * (F * F - sum(float(d.shape[0]) ** 2 for d in descs)) / (ms_screen * 1e-3) / 1e12, 1) if ms_screen else None,
        "screen_frac_of_int8_peak": round(2.0 * 128.0 * (F * F - sum(float(d.shape[0]) ** 2 for d in descs)) / (ms_screen * 1e-3) / 1e12 / MFMA_I8_PEAK_TOPS, 4) if ms_screen else None,
        "note": "pooled exact 4-NN of all descriptors against themselves + per-query filter (featureMatchingGlobal.m:69-161): int8 "
                "proof pass over every ordered image pair (bounds per row and image), rows the filter provably drops are not "
                "searched, the others only in the images that can hold one of their four nearest (f16 candidate kernel in "
                "list mode, exact rescoring); lists bit-identical to the plain exact search",
    }


def cpu_sample(synth, input_, w, h, f, overlap, finest, bands, mode, seed, n_views, n_pairs, n_cand, pano_area):
    """The oracle chain (C + OpenMP port) on a 2 x 2 block of a config's own views, and the whole config modelled from its
    pieces (SIFT by views, exhaustive matching by pairs, RANSAC by candidate pairs, render by canvas area)."""
    import oracle
    import apsamd
    from importlib import import_module

    imgs, cams = synth.make_scene(2, 2, w, h, f, overlap, seed=seed, device="cuda", finest_px=finest)
    imgs = [i.cpu().numpy() for i in imgs]
    t0 = time.perf_counter()
    feats = [oracle.sift(im, input_["Sigma"], input_["NumLayersInOctave"], input_["ContrastThreshold"], input_["EdgeThreshold"]) for im in imgs]
    t_sift = time.perf_counter() - t0
    t0 = time.perf_counter()
    matches = {(i, j): oracle.match_features(feats[i][0], feats[j][0], input_["Ratiothreshold"], input_["Matchingthreshold"], True, 2)[0]
               for j in range(1, 4) for i in range(j)}
    t_match = time.perf_counter() - t0
    t0 = time.perf_counter()
    rng = np.random.default_rng(0)
    for (i, j), m in matches.items():
        if len(m) >= 4:
            smp = np.stack([rng.permutation(len(m))[:4] + 1 for _ in range(564)]).astype(np.uint32)
            oracle.ransac_homography(feats[j][1][m[:, 1] - 1], feats[i][1][m[:, 0] - 1], smp, input_["maxDistance"], input_["inliersConfidence"], input_["maxIter"])
    t_ransac = time.perf_counter() - t0
    rp = import_module(apsamd.__name__ + ".renderPanorama")
    sizes = [(h, w, 3)] * 4
    geo = rp.canvas_geometry(cams, sizes, mode, 0, rp.default_opts({"anglePower": 2}, cams, 0))
    t0 = time.perf_counter()
    oracle.render(imgs, cams, geo, (2048, 2048), 2.0, "multiband", bands, 1.0)
    t_render = time.perf_counter() - t0
    total = t_sift + t_match + t_ransac + t_render
    ratio = pano_area / float(geo["W"] * geo["H"])
    t_all = (n_views / 4.0) * t_sift + (n_pairs / 6.0) * t_match + (n_cand / 6.0) * t_ransac + ratio * t_render
    mp = 4 * w * h / 1e6
    return {"value": round(mp / total, 3), "unit": "MPix/s", "cores": int(oracle.NUM_THREADS), "kind": "port",
            "sample": f"2x2 block of this config's {w}x{h} views ({mp:.1f} MPix in): oracle SIFT x4 ({t_sift:.1f}s), 6 pairs exhaustive match "
                      f"({t_match:.1f}s), RANSAC ({t_ransac:.1f}s), {mode} render + {bands}-band blend of {geo['W']}x{geo['H']} ({t_render:.1f}s)",
            "modelled_whole_config": {"value": round(n_views * w * h / 1e6 / t_all, 3), "unit": "MPix/s", "seconds": round(t_all, 1),
                                      "how": f"{n_views}/4 x SIFT + {n_pairs}/6 x match + {n_cand}/6 x RANSAC + {ratio:.1f} x render of the sample"}}


DUMP_SAMPLE_PX = 1 << 21       # panorama pixels drawn for panorama_sample (x 3 channels x 4 B: 24 MiB at most)
DUMP_BLOCK_BYTES = 24 << 20    # panorama_block_mean stays below this (the block side doubles from 16 until it does)


def save_pano(path, pano):
    """--save-pano: a downscaled PNG of the panorama (debug)."""
    from PIL import Image

    small = pano[:: max(1, pano.shape[0] // 1200), :: max(1, pano.shape[0] // 1200)].cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(small).save(path)


def dump_outputs(out_dir, pano, info):
    """--dump-outputs: what the last timed step handed its caller (stitch_distributed's panorama and info), as out_dir/<name>.npy
    in float32 / float64, under 64 MB in all.  The cropped uint8 panorama (737 MB for the headline job) is written as the mean of
    every b x b block (every pixel enters one; sums of uint8 are exact, so the means are too) and as the exact values at a fixed,
    seeded sample of pixels (panorama_sample_index: flat row-major indices); beside them its shape, the feature count of every
    view, the verified pairs with their homographies, the component's members and every view's camera (NaN: no camera)."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"n_features": np.asarray(info["n_features"], np.float64),
              "pairs": np.asarray(info["pairs"], np.float64).reshape(-1, 2),
              "models": np.asarray(info["models"], np.float64).reshape(-1, 3, 3),
              "members": np.asarray(info["members"], np.float64)}
    cams = info["cameras"]
    for key in ("K", "R"):
        arrays["cameras_" + key] = np.stack([np.asarray(c[key], np.float64) if c is not None else np.full((3, 3), np.nan)
                                             for c in cams]) if cams else np.zeros((0, 3, 3))
    shape = tuple(int(v) for v in pano.shape) if pano is not None else (0, 0, 3)
    arrays["panorama_shape"] = np.asarray(shape, np.float64)
    h_, w_ = shape[0], shape[1]
    if h_ and w_:
        b = 16
        while (h_ // b) * (w_ // b) * 3 * 4 > DUMP_BLOCK_BYTES:
            b *= 2
        hb, wb = h_ // b, w_ // b
        if hb and wb:
            sums = pano[: hb * b, : wb * b].to(torch.int32).reshape(hb, b, wb, b, 3).sum(dim=(1, 3))
            arrays["panorama_block_mean"] = (sums.cpu().numpy().astype(np.float64) / (b * b)).astype(np.float32)
            arrays["panorama_block_side"] = np.asarray([b], np.float64)
        idx = np.unique(np.random.default_rng(20240601).integers(0, h_ * w_, size=min(DUMP_SAMPLE_PX, h_ * w_)))
        rows = torch.from_numpy(idx // w_).to(pano.device)
        cols = torch.from_numpy(idx % w_).to(pano.device)
        arrays["panorama_sample"] = pano[rows, cols].cpu().numpy().astype(np.float32)
        arrays["panorama_sample_index"] = idx.astype(np.float64)
    total = sum(a.nbytes for a in arrays.values())
    if total > 64_000_000:
        raise RuntimeError(f"--dump-outputs: {total} bytes, over the 64 MB limit")
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(arrays)


def run_config(args):
    """`bench.py --config N`: BASELINE.json configs[N] (N != 2) on ONE GPU - the same contract as the headline line (W warm-up
    steps, K timed steps between device synchronisations, inputs resident in HBM, ONE JSON line with roofline / cpu_baseline /
    stages), on the synthetic realisations tests/test_config0_gpu.py, test_config1_gpu.py and test_fullsize_gpu.py stitch."""
    import ctypes
    import apsamd
    from importlib import import_module

    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    torch.cuda.set_device(0)
    capi = apsamd._capi
    capi.check(capi.lib.aps_set_device(0))
    synth = import_module(apsamd.__name__ + ".synth")
    pl = import_module(apsamd.__name__ + ".pipeline")
    par = import_module(apsamd.__name__ + ".parallel")
    fm = import_module(apsamd.__name__ + ".featureMatching")
    im = import_module(apsamd.__name__ + ".imageMatching")
    rp = import_module(apsamd.__name__ + ".renderPanorama")
    cfg, ref = args.config, bool(args.reference_defaults)
    if cfg == 0:
        w, h, f, name = 1024, 768, 1100.0, "BASELINE.json configs[0]: two 1024x768 views related by a homography, SIFT -> exhaustive match -> RANSAC -> planar-scan composite (host-orchestrated over the device imageWarp / multiband operators), 3 bands"
        views, cams = synth.make_scene(2, 1, w, h, f, 0.55, seed=77, device="cuda", finest_px=4.0)
        input_ = pl.default_input(bands=3)
        mode = "planar"
    elif cfg == 1:
        w, h, f = 1600, 1200, 1400.0
        views, cams = synth.make_scene(10, 2, w, h, f, 0.35, seed=2024, device="cuda", finest_px=4.0)
        input_ = pl.default_input(bands=3)
        if ref:
            input_.update(matchFeaturesPairwise=0, k=4, gainCompensation=1)
        name = ("BASELINE.json configs[1]: 20 views of 1600x1200 (10x2 ring, f=1400, 35% overlap), spherical, 3-band multiband" +
                (", the reference's default switches (global matcher k=4, gain compensation on; PP/inputs.m:46,94,99-101)" if ref else ", all-pairs exhaustive matcher"))
        mode = "spherical"
    elif cfg == 3:
        w, h, f = W, H, FOCAL
        cams = synth.grid_cameras(32, 8, w, h, f, np.radians(11.25), np.radians(9.2), 1.0, 12345)
        views = [synth.render_view(c, h, w, 12345, "cuda", finest_px=FINEST_PX) for c in cams]
        input_ = pl.default_input(bands=5)
        name = "BASELINE.json configs[3]'s image set on ONE GPU: 256 views of 3840x2160 (32x8 full ring, f=8000), all 32640 pairs, spherical, 5 bands (the 8-GPU sharding needs the node)"
        mode = "spherical"
    else:
        w, h, f = 2048, 1080, 2400.0
        fov_x = 2 * np.arctan(w / (2 * f))
        worlds = [(10, 6, 0.40), (10, 7, 0.40), (10, 8, 0.40), (10, 9, 0.45), (19, 5, 1.0 - (2 * np.pi / 19) / fov_x), (15, 7, 0.45)]
        views, cams = [], []
        for wi, (nx_, ny_, ov) in enumerate(worlds):
            v_, c_ = synth.make_scene(nx_, ny_, w, h, f, ov, seed=1000 + 17 * wi, device="cuda", finest_px=10.0)
            views += v_
            cams += c_
        perm = np.random.default_rng(9).permutation(len(views))
        views, cams = [views[k] for k in perm], [cams[k] for k in perm]
        input_ = pl.default_input(bands=5, panorama2DisplaynSave="equirectangular")
        name = "BASELINE.json configs[4] on ONE GPU: 500 mixed 2048x1080 views of six worlds, all 124750 pairs -> connected components -> six equirectangular panoramas, 5 bands"
        mode = "equirectangular"
    torch.cuda.synchronize()
    n = len(views)
    Ks = [c["K"] for c in cams]
    local = dict(enumerate(views))
    views_host = [v.cpu().numpy() for v in views] if cfg == 0 else None

    def sync():
        capi.check(capi.lib.aps_synchronize())
        torch.cuda.synchronize()

    def step():
        t_s = time.perf_counter()
        if cfg == 0:
            times = pl.StageTimes()
            t0 = time.perf_counter()
            feats = pl.sift_many(input_, views)
            times.add("features", t0)
            t0 = time.perf_counter()
            cells = fm.featureMatchingPairwise(input_, [d for d, _ in feats], 2)
            times.add("matching", t0)
            t0 = time.perf_counter()
            m = cells[0][1].astype(np.int64)
            p1, p2 = np.asarray(feats[0][1])[m[:, 0] - 1].astype(np.float64), np.asarray(feats[1][1])[m[:, 1] - 1].astype(np.float64)
            Hm, mask, found = im.estimateTransformationRANSAC(p2, p1, "projective", input_, sample_idx=im.draw_samples([len(m)], 564, seed=11)[0])
            times.add("im_ransac", t0)
            if not found:
                raise RuntimeError("configs[0]: the pair was not verified")
            t0 = time.perf_counter()
            pcams = [{"H2refined": np.eye(3), "noRotation": 1}, {"H2refined": Hm / Hm[2, 2], "noRotation": 1}]
            # (the planar-scan path, renderPanorama.m:519-699, is host-orchestrated like the reference's: numpy canvases
            # over the device imageWarp / multiBandBlending operators; it takes the views from host memory)
            pano_, _ = rp.renderPanorama(input_, views_host, [(h, w, 3)] * 2, pcams, "planar", 0,
                                         {"blending": "multiband", "pyrLevels": 3, "pyrSigma": 1.0, "canvasColor": "black"})
            pano_ = torch.from_numpy(np.ascontiguousarray(pano_))
            times.add("render", t0)
            info_ = {"times": dict(times), "n_features": [int(d.shape[0]) for d, _ in feats], "n_pairs_verified": 1, "panoramas": [pano_], "n_components": 1}
        else:
            pano_, info_ = par.stitch_distributed(input_, local, n, Ks, (2048, 2048), 0, None, pano_root=0)
        sync()
        info_["t_step"] = time.perf_counter() - t_s
        return pano_, info_

    warm_prof = {}
    n_warm = max(args.warmup, 2)  # (the per-image / per-tile launch sites are bracketed in the LAST warm-up step: never the process's first step)
    for k in range(n_warm):
        last = k == n_warm - 1
        if last:
            capi.profile_enable(1)
            capi.profile_reset()
        pano, info = step()
        if last:
            warm_prof = capi.profile_all()
            capi.profile_enable(False)
    capi.profile_enable(2)
    capi.profile_reset()
    sync()
    t0 = time.perf_counter()
    infos = []
    for _ in range(args.steps):
        pano, info = step()
        shapes = [tuple(int(v) for v in p_.shape) for p_ in info.get("panoramas", [pano])]
        info.pop("panoramas", None)
        info["shapes"] = shapes
        infos.append(info)
    sync()
    dt = time.perf_counter() - t0
    prof = {k: (v[0], v[1]) for k, v in capi.profile_all().items()}
    live = set(prof)
    capi.profile_enable(False)
    for k, v in warm_prof.items():
        if k not in prof:
            prof[k] = (v[0] * args.steps, v[1] * args.steps)
    info = infos[-1]
    counts = info["n_features"]
    mpix_in = n * w * h / 1e6
    walls = [i["t_step"] for i in infos]
    Fsum = float(sum(counts))
    pair_w = sum(float(counts[i]) * float(counts[j]) for j in range(1, n) for i in range(j))
    glob = not input_.get("matchFeaturesPairwise", 1)
    flops = 2.0 * 128.0 * ((Fsum * Fsum - sum(float(c) ** 2 for c in counts)) if glob else pair_w)
    a_cov = float(n * w * h)
    a_pano = float(sum(s_[0] * s_[1] for s_ in info["shapes"]))

    def roof(keys, name_, bound, work, peak, unit):
        ms = sum(prof.get(k, (0.0, 0))[0] for k in keys)
        if ms <= 0:
            return None
        scale = 1e12 if unit in ("TFLOP/s", "TOP/s") else 1e9
        ach = work * args.steps / (ms * 1e-3) / scale
        return {"bound": bound, "kernel": name_, "achieved": round(ach, 2), "peak": peak, "unit": unit, "frac": round(ach / peak, 4), "traffic": None,
                "algorithmic_work_per_step": work, "ms_per_step": round(ms / args.steps, 3),
                "launches_per_step": sum(prof.get(k, (0.0, 0))[1] for k in keys) // max(args.steps, 1),
                "timed": "live over the timed steps" if keys[0] in live else "during the last warm-up step"}

    cands = [roof(["match_screen_i8_bounds"] if glob else ["match_screen_i8"], "match_screen_i8x16_kernel (int8 proof pass" + (", bounds form of the pooled matcher)" if glob else ")"),
                  "mfma", flops, MFMA_I8_PEAK_TOPS, "TOP/s"),
             roof(["render_pyr_down", "render_collapse"], "multiband chain (rw_down_fused x levels, rw_up x levels incl. paint)", "hbm", 64.0 * a_cov + 32.0 * a_pano, HBM_PEAK_GBS, "GB/s"),
             roof(["render_warp"], "rw_warp_staged_kernel", "hbm", 16.0 * a_cov + 3.0 * a_cov, HBM_PEAK_GBS, "GB/s"),
             roof(["multiband"], "planar-scan multiband blend (aps_multiband_blend: 64 B per canvas pixel and layer)", "hbm", 64.0 * a_pano * n, HBM_PEAK_GBS, "GB/s")]
    t_feat = sum(i["times"].get("features", 0.0) for i in infos) / len(infos)
    if t_feat > 0:
        ach = 574.0 * a_cov / t_feat / 1e9
        cands.append({"bound": "hbm", "kernel": "SIFT stage (all kernels of all views on their worker streams, wall time of the stage)", "achieved": round(ach, 2),
                      "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None, "algorithmic_work_per_step": 574.0 * a_cov,
                      "ms_per_step": round(1e3 * t_feat, 3), "timed": "live over the timed steps"})
    cands = [c for c in cands if c]
    dominant = max(cands, key=lambda c: c["ms_per_step"]) if cands else None
    rows, surv = ctypes.c_int64(0), ctypes.c_int64(0)
    capi.check(capi.lib.aps_match_screen_stats(ctypes.byref(rows), ctypes.byref(surv)))
    out = {"metric": "MPix/s end-to-end stitch (SIFT->blend)", "value": round(mpix_in * args.steps / dt, 2), "unit": "MPix/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 2), "ms_per_step_median": round(1e3 * float(np.median(walls)), 2),
           "ms_per_step_min": round(1e3 * min(walls), 2), "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": name + "; inputs resident in HBM, panoramas left in HBM", "baseline_config_index": cfg, "reference_defaults": ref,
                      "views": n, "input_mpix": round(mpix_in, 1), "features_per_view": int(np.mean(counts)), "pairs_verified": info.get("n_pairs_verified"),
                      "components": info.get("n_components"), "panoramas": [[s_[1], s_[0]] for s_ in info["shapes"]],
                      "int8_screen_survivor_share": round(surv.value / rows.value, 4) if rows.value else None},
           "roofline": dominant, "rooflines_all": cands,
           "stages_ms_per_step": {k: round(1e3 * sum(i["times"].get(k, 0.0) for i in infos) / len(infos), 2) for k in info["times"]},
           "kernels": {k: {"ms_per_step": round(v[0] / args.steps, 3), "launches_per_step": v[1] // max(args.steps, 1)} for k, v in prof.items() if v[0] / args.steps > 0.005}}
    if args.cpu_baseline == "auto":
        try:
            if cfg == 0:
                out["cpu_baseline"] = dict(cpu_cfg1_single_thread(synth), kind="port")
            else:
                n_pairs = n * (n - 1) // 2
                out["cpu_baseline"] = cpu_sample(synth, input_, w, h, f, {1: 0.35, 3: 0.4, 4: 0.4}[cfg], {1: 4.0, 3: FINEST_PX, 4: 10.0}[cfg], input_["bands"],
                                                 "spherical", {1: 2024, 3: 12345, 4: 1000}[cfg], n, n_pairs, max(1, int(info.get("n_pairs_verified") or n)), a_pano)
        except Exception as e:  # a report, never a reason to lose the bench line
            out["cpu_baseline"] = {"value": None, "unit": "MPix/s", "cores": 0, "kind": "port", "sample": f"failed: {e}"}
    os.write(result_fd, (json.dumps(out) + "\n").encode())
    return 0


def launcher_command(n_gpus, argv, port=None):
    """The command `python bench.py --gpus N` (N > 1, no WORLD_SIZE in the environment) runs as a CHILD process: one rank
    per GPU under torch.distributed.run, rendezvous on 127.0.0.1 - the form the driver itself uses."""
    if port is None:
        import socket

        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def launch_ranks(n_gpus, argv):
    """Starts the N ranks before this process has made any GPU call (it never makes one: a process that has initialised the
    GPU must not exec, and this one only waits), relays rank 0's single JSON line and returns the child's exit code."""
    import subprocess

    # (device_count() may call hipGetDeviceCount on this image; that is harmless HERE because this process never execs - it
    # starts the ranks as a CHILD and waits.  Keep it that way: no os.exec* below this line.)
    have = torch.cuda.device_count()
    if os.environ.get("APS_BENCH_RANK_PROBE") != "1" and os.environ.get("APS_BENCH_REHEARSE") != "1" and have < n_gpus:
        print(f"bench.py: --gpus {n_gpus} but this node shows {have} GPU(s)", file=sys.stderr)
        return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.Popen(launcher_command(n_gpus, argv), stdout=subprocess.PIPE, env=env, text=True)
    lines = [l for l in proc.stdout.read().splitlines() if l.strip()]
    rc = proc.wait()
    results = [l for l in lines if l.lstrip().startswith("{")]
    for l in lines:
        if l not in results:
            print(l, file=sys.stderr)
    if rc == 0 and len(results) != 1:
        print(f"bench.py: expected ONE result line from rank 0, got {len(results)}", file=sys.stderr)
        rc = 3
    if results:
        print(results[-1], flush=True)
    return rc


def rank_probe(args):
    """APS_BENCH_RANK_PROBE=1 (test hook, tests/test_parallel_cpu.py): what every rank does before it touches a GPU - the
    environment torch.distributed.run hands over, the --gpus / WORLD_SIZE check, a process group (gloo), one all-reduce, ONE
    JSON line from rank 0 - so that the launcher's argument handling and relay are covered without a device."""
    import torch.distributed as dist

    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    dist.all_reduce(t)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"probe": True, "n_gpus": world, "gpus_arg": args.gpus, "steps": args.steps, "warmup": args.warmup,
                          "rank_sum": float(t.item()), "master_addr": os.environ.get("MASTER_ADDR")}), flush=True)
    dist.destroy_process_group()
    return 0


def main():
    if os.environ.get("APS_BENCH_WATCHDOG"):  # debugging aid: dump every thread's stack and exit if the run takes longer
        import faulthandler

        faulthandler.dump_traceback_later(int(os.environ["APS_BENCH_WATCHDOG"]), exit=True)
    args = parse()
    if args.gpus is None:  # (not given: a launcher's WORLD_SIZE decides, a plain run is one GPU)
        args.gpus = int(os.environ.get("WORLD_SIZE", "1"))
    # `--gpus N` is what decides the rank count.  Launched by torch.distributed.run (the driver's form for N > 1) the
    # environment carries WORLD_SIZE, which must agree; launched plainly with N > 1 the ranks are started here as children.
    if "WORLD_SIZE" in os.environ:
        if int(os.environ["WORLD_SIZE"]) != args.gpus:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']} ranks were launched: pass --gpus "
                  f"{os.environ['WORLD_SIZE']} (or leave --gpus out) under this launcher", file=sys.stderr)
            sys.exit(2)
    elif args.gpus > 1:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    elif args.gpus < 1:
        print("bench.py: --gpus must be >= 1", file=sys.stderr)
        sys.exit(2)
    if os.environ.get("APS_BENCH_RANK_PROBE") == "1":
        sys.exit(rank_probe(args))
    if args.config is not None:
        if args.gpus != 1:
            print("bench.py: --config N runs on one GPU (the headline, configs[2], is the line that scales)", file=sys.stderr)
            sys.exit(2)
        if args.dump_outputs:
            print("bench.py: --dump-outputs writes the headline run's outputs; it does not apply to --config N", file=sys.stderr)
            sys.exit(2)
        sys.exit(run_config(args))
    if not args.full:  # a plain run: the headline figure only, none of the extra legs
        args.cpu_baseline = args.end_to_end = args.global_probe = args.with_gain = "off"
    # The contract is ONE JSON line on stdout.  Libraries write there too (RCCL prints a five-line version banner to stdout
    # when a communicator comes up): everything but the result line is sent to stderr by pointing fd 1 at fd 2 for the
    # run; the result is written to the saved descriptor at the end.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # APS_BENCH_REHEARSE=1 (test hook): every rank on device 0 over the gloo backend - RCCL refuses two ranks on one GPU, and a
    # one-GPU box has no other way to walk this file's N > 1 path (the shard arithmetic of the roofline entries, the
    # max-over-ranks reduction, rank 0's single line).  The numbers of such a run mean nothing.
    rehearse = os.environ.get("APS_BENCH_REHEARSE") == "1"
    if rehearse:
        local_rank = 0
    # APS_PARALLEL_FORCE_COLLECTIVES=1 (test hook, see parallel._multi): the N > 1 launch path - process group on "nccl",
    # barriers, the max-over-ranks reduction, every collective of the sharded driver - with a single rank, which is as far
    # as a one-GPU box can rehearse what `torchrun --nproc-per-node N bench.py --gpus N` does
    multi = world > 1 or os.environ.get("APS_PARALLEL_FORCE_COLLECTIVES") == "1"
    if multi:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29551")
        os.environ["APS_DEVICE"] = str(local_rank)
    torch.cuda.set_device(local_rank)

    import apsamd
    from importlib import import_module

    capi = apsamd._capi
    capi.check(capi.lib.aps_set_device(local_rank))
    if multi:
        import torch.distributed as dist

        if rehearse:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    synth = import_module(apsamd.__name__ + ".synth")
    pl = import_module(apsamd.__name__ + ".pipeline")
    par = import_module(apsamd.__name__ + ".parallel")

    nx, ny = (int(v) for v in args.grid.lower().split("x"))
    w, h = (int(v) for v in args.size.lower().split("x"))
    n = nx * ny
    f = FOCAL * w / W
    input_ = pl.default_input(bands=args.bands)
    if args.gain_compensation:
        input_["gainCompensation"] = 1
    if args.matcher == "global":
        input_["matchFeaturesPairwise"] = 0
        input_["k"] = 4

    # synthetic inputs, resident in HBM before anything is timed (each rank renders only its shard)
    cams = synth.grid_cameras(nx, ny, w, h, f, 2 * np.arctan(w / (2 * f)) * (1 - OVERLAP),
                              2 * np.arctan(h / (2 * f)) * (1 - OVERLAP), 1.0, 12345)
    mine = par.shard_indices(n, world, rank)
    local = {i: synth.render_view(cams[i], h, w, 12345, "cuda", finest_px=FINEST_PX) for i in mine}
    torch.cuda.synchronize()
    Ks = [c["K"] for c in cams]
    gt = cams if args.cameras == "truth" else None

    def barrier():
        drain()  # (defined below: the last panorama's copy to the host)
        capi.check(capi.lib.aps_synchronize())
        torch.cuda.synchronize()
        if multi:
            dist.barrier()
            torch.cuda.synchronize()

    # One step = the whole job: images (resident in HBM, or - end-to-end form - in pinned host memory) -> cropped uint8
    # panorama in PINNED HOST memory on the root.  SURVEY 8(d) ends the clock at "final uint8 panorama on the host", so
    # the device-to-host copy of the result belongs to every timed step; `value` starts with the inputs resident (the
    # bench contract), value_end_to_end also uploads them (side stream, SIFT of image k waits for copy k only, so PCIe
    # overlaps with the pyramid kernels).  value_resident (panorama left in HBM) is derived from the same steps' stage times.
    host_imgs, copy_stream = {}, None
    if args.end_to_end == "auto":
        host_imgs = {i: torch.empty(local[i].shape, dtype=torch.uint8, pin_memory=True).copy_(local[i]) for i in mine}
        copy_stream = torch.cuda.Stream(priority=-1)

    # The device-to-host copy of step k's panorama (737 MB, ~13 ms of PCIe) is started while step k + 1 is MATCHING and
    # lands in one of two pinned buffers: what a production loop that stitches set after set does.  (Started at once it
    # overlaps step k + 1's feature extraction instead and costs that stage more than it saves - measured +10-15 ms:
    # the HIP runtime maps the copy stream onto a hardware queue it shares with per-image worker streams, whose kernels
    # then wait behind the transfer; during the matching those streams are idle.)  Every panorama has landed before the
    # closing barrier of the timed region (drain()), so `value` is the rate at which finished panoramas reach the host;
    # the un-overlapped cost of one copy is reported as download_ms_alone, the latency of one isolated step as
    # ms_per_step_latency.
    # (a HIGH-priority stream: the runtime keeps separate hardware queues per priority level, so the transfer never sits
    # in a queue in front of a normal-priority stream's kernels - with a normal-priority copy stream the descriptor
    # preparation of the matching stage, forked over eight auxiliary streams, went from 1.8 to 10.6 ms)
    out_stream = torch.cuda.Stream(priority=-1)
    host_out = [None, None]
    pending = []    # copies in flight: (done event, host view, device tensor kept alive)
    deferred = []   # device panoramas whose copy has not been started yet
    out_slot = [0]

    def start_copy(pano_):
        need = pano_.numel()
        k = out_slot[0]
        out_slot[0] ^= 1
        if host_out[k] is None or host_out[k].numel() < need:
            host_out[k] = torch.empty(int(need * 1.05) + 1, dtype=torch.uint8, pin_memory=True)
        dst = host_out[k][:need].view(pano_.shape)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        with torch.cuda.stream(out_stream):
            out_stream.wait_event(ready)
            dst.copy_(pano_, non_blocking=True)
            done = torch.cuda.Event()
            done.record(out_stream)
        pending.append((done, dst, pano_))
        return dst

    def flush_deferred():
        while pending:  # (the copy before last: long finished)
            pending.pop(0)[0].synchronize()
        while deferred:
            start_copy(deferred.pop(0))

    # Round 6: the copy starts a few milliseconds INTO the matching, not at its first instruction: the matcher opens with its
    # bandwidth-bound operand preparation (~1.3 ms: a dozen short launches, one table upload), and beside the 737 MB download that
    # phase took 2.5-3.6 ms; the int8 screen that follows (60 ms) does not care.  A timer thread enqueues the copy (the main
    # thread is inside the matcher's C call by then, without the GIL); drain() joins it.
    import threading

    timers = []

    def flush_deferred_soon():
        if not deferred and not pending:
            return
        tm = threading.Timer(0.004, flush_deferred)
        timers.append(tm)
        tm.start()

    def drain():
        while timers:
            timers.pop(0).join()
        flush_deferred()
        while pending:
            pending.pop(0)[0].synchronize()

    def to_host(pano_, wait=False):
        if wait:
            drain()
            dst = start_copy(pano_)
            drain()
            return dst
        deferred.append(pano_)  # copied while the NEXT step is matching (or by drain() at the end of the run)
        return pano_

    dl_alone = []

    # Round 6: a loop that stitches set after set starts the NEXT set's feature extraction as soon as the current set's match
    # lists are complete (parallel.submit_features from the after_matching hook): RANSAC's latency-bound launches, the replicated
    # host work and the render's host part leave the GPU idle for ~5 ms of every step, and the bandwidth-bound render shares the
    # chip with the extraction better than either does alone.  Every step still does all of its own work inside the timed
    # region: the first timed step extracts its own features, the last one prefetches nothing (`pipelined` below).
    ahead = [None]  # (images, events, handle) of the next step, extraction under way
    prefetch_at = os.environ.get("APS_BENCH_PREFETCH_AT", "matching")  # (A/B: "ransac" starts it after this rank's RANSAC batch)
    prefetch_first = int(os.environ["APS_BENCH_PREFETCH_FIRST"]) if os.environ.get("APS_BENCH_PREFETCH_FIRST") else None
    pipelined = os.environ.get("APS_BENCH_PIPELINE", "1" if args.pipeline == "auto" else "0") == "1"
    if pipelined and os.environ.get("APS_BENCH_MAIN_PRIORITY", "1") != "0":
        # the main thread's launches (RANSAC, the render chain) must not queue behind the ten worker streams' kernels: the
        # runtime keeps separate hardware queues per priority level (157.5 against 162.0 ms per steady step, scripts/probe/ab_pipeline.sh)
        capi.check(capi.lib.aps_set_thread_stream_priority(1))

    def load_images(upload):
        if not upload:
            return local, None
        up, evs = {}, {}
        with torch.cuda.stream(copy_stream):
            for i in mine:
                up[i] = host_imgs[i].to("cuda", non_blocking=True)
                evs[i] = torch.cuda.Event()
                evs[i].record(copy_stream)
        return up, evs

    def step(upload=False, sync_download=False, prefetch_next=False):
        t_s = time.perf_counter()
        if ahead[0] is not None:
            imgs, evs, feat = ahead[0]
            ahead[0] = None
        else:
            imgs, evs = load_images(upload)
            feat = None

        def start_next():
            imgs_n, evs_n = load_images(upload)
            ahead[0] = (imgs_n, evs_n, par.submit_features(input_, imgs_n, evs_n, first=prefetch_first))

        def start_rest():
            if ahead[0] is not None:
                par.submit_features_rest(ahead[0][2])

        pano_, info_ = par.stitch_distributed(input_, imgs, n, Ks, (2048, 2048), 0, gt, pano_root=0, image_events=evs,
                                              after_features=flush_deferred_soon, features=feat,
                                              after_matching=start_next if prefetch_next and prefetch_at == "matching" else None,
                                              after_ransac=(start_next if prefetch_at == "ransac" else start_rest) if prefetch_next else None)
        t_d = time.perf_counter()
        if rank == 0 and pano_ is not None and pano_.numel():
            pano_ = to_host(pano_, wait=sync_download)
        info_["times"]["download"] = time.perf_counter() - t_d

        info_["t_stitch"] = t_d - t_s
        return pano_, info_

    # Kernel timing by HIP events on the library's streams.  Two event records per launch are not free when a step
    # issues ~5000 launches (2.7 % of the step), so the timed region brackets only the per-batch launch sites - which
    # include the dominant kernel, whose `roofline` is therefore measured live over the timed steps - and the
    # per-image / per-tile chains (SIFT, warp, pyramid) are bracketed during the last warm-up step instead.
    warm_prof, warm_steps = {}, 0
    pano_w = None
    for k in range(args.warmup):
        last = k == args.warmup - 1 and args.full
        if last:
            capi.profile_enable(1)
            capi.profile_reset()
        pano_w, _ = step(sync_download=True)
        if last:
            barrier()
            warm_prof, warm_steps = capi.profile_all(), 1
            capi.profile_enable(False)
    # the GPU's clock and power during one more untimed step, by stage (GpuStateSampler; rank 0 reports its own GPU)
    gpu_state = None
    if args.warmup > 0:  # (every rank takes the steps: they run the sharded driver's collectives)
        # Two more untimed steps in the STEADY-STATE form (the panorama's download deferred into the next step's matching): the
        # synchronous warm-up steps above never hold two panoramas at once, so the allocator's second 737 MB canvas used to be
        # malloc'ed - and its pages scrubbed - inside the second TIMED step (+12-18 ms there in every run's series).  The second
        # of the two is also the step the GPU's clock and power are sampled in.
        step()
        sampler = GpuStateSampler(local_rank) if args.full else None
        if sampler is not None:
            sampler.start()
        t_s0 = time.perf_counter()
        _, info_s = step()
        barrier()
        if sampler is not None:
            sampler.stop()
        if sampler is None or rank != 0:
            pass
        elif sampler.files:
            tm = info_s["times"]
            t_f = t_s0 + tm.get("features", 0.0) + tm.get("exchange", 0.0)
            t_m = t_f + tm.get("matching", 0.0)
            gpu_state = {"source": "amdgpu hwmon freq1_input / power1_input of " + sampler.files[2] + ", one untimed step, 2 ms sampling",
                         "features": sampler.window(t_s0 + 0.1 * (t_f - t_s0), t_f - 0.1 * (t_f - t_s0)),
                         "matching_screen": sampler.window(t_f + 0.05 * (t_m - t_f), t_f + 0.75 * (t_m - t_f)),
                         "render": sampler.window(t_s0 + info_s["t_stitch"] - tm.get("render", 0.0), t_s0 + info_s["t_stitch"])}
        else:
            gpu_state = {"source": None, "note": "no readable amdgpu hwmon files for this rank's GPU"}
    # the un-overlapped cost of one panorama copy (both pinned buffers exist by now): three synchronous copies of a
    # canvas-sized device buffer, the fastest counts (--full).  A plain run allocates and frees the buffer all the same: the
    # block it leaves in torch's cache is one the pipelined timed steps would otherwise malloc (+20 ms in a timed step).
    if rank == 0 and args.warmup > 0 and pano_w is not None and pano_w.numel():
        probe = torch.empty(tuple(pano_w.shape), dtype=torch.uint8, device="cuda")
        for _ in range(3 if args.full else 0):
            torch.cuda.synchronize()
            t_c = time.perf_counter()
            to_host(probe, wait=True)
            dl_alone.append(time.perf_counter() - t_c)
        del probe
    def run_series(k_steps, upload=False, pipe=False):
        """k_steps steps between two barriers; pipe: every step but the last starts the next one's feature extraction from
        its after_matching hook (the first extracts its own, so all the work of the k_steps stitches lies between the barriers).
        Returns (seconds, per-step infos, time marks after each step, the start time, the last panorama)."""
        barrier()
        t_b = time.perf_counter()
        infos_, marks_, pano_ = [], [], None
        for k_ in range(k_steps):
            pano_, info_ = step(upload=upload, prefetch_next=pipe and k_ + 1 < k_steps)
            # keep the step's numbers, not its panoramas: a list that pins every step's 737 MB output makes each step
            # hipMalloc a fresh canvas (up to 17 ms per step when the driver has to scrub the pages first) - a cost of the
            # bench's bookkeeping, not of a stitch.  The current panorama stays alive until the next one replaces it.
            info_.pop("panoramas", None)
            infos_.append(info_)
            marks_.append(time.perf_counter())
        barrier()
        return time.perf_counter() - t_b, infos_, marks_, t_b, pano_

    if args.full:
        capi.profile_enable(2 if warm_steps else 1)
        capi.profile_reset()
    dt, infos, marks, t0, pano = run_series(args.steps, pipe=pipelined)
    # wall time of each timed step (start of step k to start of step k + 1; the last one ends at the closing barrier, which
    # includes the last panorama's copy): their mean is ms_per_step, the median and the minimum make a 2 ms change visible
    step_walls = [b - a for a, b in zip([t0] + marks[:-1], marks[:-1] + [t0 + dt])]
    prof, screen_series = {}, []
    if args.full:
        prof = capi.profile_all()
        screen_series = capi.profile_series("match_screen_i8")
        capi.profile_enable(False)
    if args.dump_outputs and rank == 0:  # (the panorama is delivered to rank 0 only)
        dump_outputs(args.dump_outputs, pano, infos[-1])
    # The same steps strictly one after the other (value_sequential; the stage table comes from these steps: in the pipelined
    # series a step's "features" is only what was left to wait for and its "render" shares the chip with the next extraction).
    dt_seq, infos_seq, seq_walls = None, infos, None
    if pipelined and args.full:
        n_seq = max(2, min(args.steps, 8))
        capi.profile_enable(2 if warm_steps else 1)
        capi.profile_reset()
        dt_seq, infos_seq, marks_s, t0_s, _ = run_series(n_seq)
        seq_walls = [b - a for a, b in zip([t0_s] + marks_s[:-1], marks_s[:-1] + [t0_s + dt_seq])]
        # the per-batch launch sites that shared the chip with the next extraction in the pipelined steps (RANSAC, the render
        # chain, the crop) are reported from these sequential steps, where a kernel has the chip to itself like the int8
        # kernels always have; the matcher's entries stay those of the timed region
        for k_, v_ in capi.profile_all().items():
            if not k_.startswith("match"):
                prof[k_] = (v_[0] * args.steps / n_seq, v_[1] * args.steps // n_seq)
        capi.profile_enable(False)
    # The same steps with input.gainCompensation = 1 (the reference's default, PP/inputs.m:94; renderPanorama.m:303-330): the
    # overlap statistics on the device (gain_stats_kernel), the N x N x 3 sums back to the host, the host solve, the gains into
    # the warp.  Reported as value_with_gain; the headline follows BASELINE.json configs[2], which does not name the switch.
    dt_gain, infos_g = None, []
    if args.with_gain == "auto" and world == 1 and not input_.get("gainCompensation"):  # (N = 1 only, like the other extra legs)
        input_["gainCompensation"] = 1
        try:
            step(sync_download=True)  # warm-up (the statistics' workspaces)
            dt_gain, infos_g, _, _, _ = run_series(args.steps, pipe=pipelined)
        finally:
            input_["gainCompensation"] = 0
    dt_e2e = None
    if args.end_to_end == "auto":
        step(upload=True)  # warm-up: side stream
        dt_e2e, infos_h, _, _, pano_h = run_series(args.steps, upload=True, pipe=pipelined)
        info_h = infos_h[-1]
        if rank == 0 and (info_h["n_pairs_verified"], tuple(pano_h.shape)) != (infos[-1]["n_pairs_verified"], tuple(infos[-1]["panorama_shape"])):
            raise RuntimeError("the end-to-end step disagrees with the resident step on verified pairs / panorama size")
    # per-step view of both passes: live numbers win
    live = set(prof)
    prof = {k: (v[0], v[1]) for k, v in prof.items()}
    for k, v in warm_prof.items():
        if k not in prof:
            prof[k] = (v[0] * args.steps / warm_steps, v[1] * args.steps // warm_steps)
    if multi:
        t = torch.tensor([dt, dt_e2e or 0.0, dt_gain or 0.0, dt_seq or 0.0], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t[0].item())
        dt_e2e = float(t[1].item()) if dt_e2e is not None else None
        dt_gain = float(t[2].item()) if dt_gain is not None else None
        dt_seq = float(t[3].item()) if dt_seq is not None else None

    if rank == 0:
        info = infos[-1]
        # same input, seeded draws: every step must reproduce the same result (a race between streams shows up here)
        for other in infos[:-1]:
            if (other["n_pairs_verified"], tuple(other["panorama_shape"])) != \
                    (info["n_pairs_verified"], tuple(info["panorama_shape"])):
                raise RuntimeError("non-deterministic stitch: steps disagree on verified pairs / panorama size")
    if rank == 0 and not args.full:
        mpix_in = n * w * h / 1e6
        out = {"metric": "MPix/s end-to-end stitch (SIFT->blend), 64x4K images",
               "value": round(mpix_in * args.steps / dt, 2), "unit": "MPix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(1e3 * dt / args.steps, 2), "higher_is_better": True, "scaling": "strong",
               "ms_per_step_median": round(1e3 * float(np.median(step_walls)), 2), "ms_per_step_min": round(1e3 * min(step_walls), 2),
               "ms_per_step_series": [round(1e3 * x, 2) for x in step_walls],
               "vs_baseline": None, "dtype": "f32", "data": "synthetic", "pipelined": pipelined, "full": False}
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(out) + "\n").encode())
        if args.save_pano:
            save_pano(args.save_pano, pano)
    if rank == 0 and args.full:
        mpix_in = n * w * h / 1e6
        value = mpix_in * args.steps / dt
        dt_resident = sum(i["t_stitch"] for i in infos)
        counts = info["n_features"]
        # roofline of the dominant kernel: this rank's share of F_match = 2*128*sum N_i*N_j over ITS pairs
        order = [(i, j) for j in range(1, n) for i in range(j)]
        wts = [float(counts[i]) * float(counts[j]) for (i, j) in order]
        own = par.partition_weighted(wts, world) if world > 1 else np.zeros(len(order), np.int64)
        flops_rank0 = 2.0 * 128.0 * sum(wt for wt, o in zip(wts, own) if o == 0)
        if args.matcher == "global":  # 2 * 128 * F^2 for the pooled search (every ordered pair of rows)
            flops_rank0 = 2.0 * 128.0 * float(sum(counts)) ** 2
        # --- rooflines -------------------------------------------------------------------------------
        # algorithmic work per step: F_match = 2*128*sum N_i*N_j over this rank's pairs;
        # B_sift = 574 B per input pixel (materialised pyramid); B_warp = 16*A_cov + 3*sum(h*w);
        # B_blend = 64*A_cov + 32*A_pano, with A_cov ~= the summed input pixels (the canvas is rendered ~1:1).
        npix_rank0 = sum(w * h for i in range(n) if i % world == 0)
        a_cov = n * w * h / world
        a_pano = float(pano.shape[0] * pano.shape[1]) / world

        # HBM-side bytes per launch from the committed PMC pass of THIS workload (scripts/hbm_traffic.sh ->
        # profiles/*_hbm_traffic.json: L2 memory-side requests x 64 B, one bench step); null for other configs
        traffic_db, traffic_file, traffic_stale = {}, None, None
        tfiles = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic.json")))
        if world == 1 and (nx, ny, w, h, args.bands) == (8, 8, W, H, 5) and args.matcher == "pairwise" and tfiles:
            traffic_file = os.path.relpath(tfiles[-1], ROOT)
            db = json.load(open(tfiles[-1]))
            meta = db.pop("_meta", {})
            # The file is a REPLAY of a separate rocprofv3 --pmc pass (scripts/hbm_traffic.sh records the hash of the kernel
            # sources it ran): a pass taken before the last kernel change describes other kernels - then nothing is reported.
            if meta.get("csrc_sha256") == csrc_sha256():
                traffic_db = db
            else:
                traffic_stale = (f"{traffic_file} was taken from other kernel sources (csrc hash {str(meta.get('csrc_sha256'))[:12]} "
                                 f"!= {csrc_sha256()[:12]} now): traffic not reported; re-run scripts/hbm_traffic.sh")

        # vector instructions per kernel from the same kind of committed pass (scripts/hbm_traffic.sh, second pass), same guard
        valu_db = {}
        vfiles = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_valu.json")))
        if traffic_file is not None and vfiles:
            vdb = json.load(open(vfiles[-1]))
            if vdb.pop("_meta", {}).get("csrc_sha256") == csrc_sha256():
                valu_db = vdb

        def valu_of(prefixes):
            rows = [v for k, v in valu_db.items() if any(p in k for p in prefixes)]
            return sum(r["insts_valu_per_step"] for r in rows) if rows else None

        def traffic_of(prefixes, per_step=False):
            rows = [v for k, v in traffic_db.items() if any(p in k for p in prefixes)]
            launches = sum(r["launches_per_step"] for r in rows)
            if not rows or launches == 0:
                return None
            total = sum(r["read_bytes_per_step"] + r["write_bytes_per_step"] for r in rows)
            return round(total if per_step else total / launches)

        TRAFFIC_KEYS = {"match_screen_i8": ["match_screen_i8"], "match_cand_f16": ["match_cand_f16_kernel"], "match2nn": ["match2nn_kernel"],
                        "sift_blur": ["aps::blur_kernel<"], "render_warp": ["rw_warp_staged_kernel", "rw_warp_kernel"],
                        "render_pyr_down": ["rw_down_fused_kernel", "rw_down_kernel", "rw_up_kernel"]}
        SIFT_KERNELS = ["blur_kernel", "blur_march_kernel", "extrema_wave_kernel", "extrema_march_kernel", "extrema_kernel", "gray_up_kernel", "descr_kernel",
                        "orient_kernel", "refine_kernel", "decimate_kernel"]

        def roof(kernel, name, bound, work_per_step, peak, unit, note="", streams=1):
            keys = [kernel] if isinstance(kernel, str) else list(kernel)  # several launch sites of one chain are summed
            kernel = keys[0]
            ms = sum(prof.get(k, (0.0, 0))[0] for k in keys)
            launches = sum(prof.get(k, (0.0, 0))[1] for k in keys)
            if ms <= 0:
                return None
            scale = 1e12 if unit in ("TFLOP/s", "TOP/s") else 1e9
            ach = work_per_step * args.steps / (ms * 1e-3) / scale
            r = {"bound": bound, "kernel": name, "achieved": round(ach, 2), "peak": peak, "unit": unit,
                 "frac": round(ach / peak, 4), "traffic": traffic_of(TRAFFIC_KEYS.get(kernel, ["\0"])),
                 "algorithmic_work_per_step": work_per_step,
                 "launches_per_step": launches // max(args.steps, 1), "ms_per_step": round(ms / args.steps, 3),
                 # kernels issued from several concurrent streams: their event intervals overlap, so the summed
                 # duration over-counts wall time by up to the stream count
                 "concurrent_streams": streams, "wall_share_ms": round(ms / args.steps / streams, 3),
                 "timed": ("live over the timed steps" if kernel.startswith("match") or not pipelined else
                           "live over the sequential steps that follow the timed region (in the pipelined steps this launch site shares the chip with the next extraction)")
                 if kernel in live else "during the last warm-up step"}
            if r["traffic"] is not None:
                r["traffic_note"] = ("HBM-side bytes per launch: the L2's memory-side requests by size (TCC_BUBBLE x 128 B + 64-B + 32-B reads; "
                                     "64-B + 32-B writes: rocprofv3's own FETCH_SIZE / WRITE_SIZE terms) from separate rocprofv3 --pmc "
                                     f"pass of this workload ({traffic_file}, taken from these kernel sources); replayed from "
                                     "that committed file, not observed in this run")
                if bound == "hbm":  # what the memory system really moved per step for this chain, over the chain's time
                    per_step = traffic_of(TRAFFIC_KEYS.get(kernel, ["\0"]), per_step=True)
                    r["traffic_bytes_per_step"] = per_step
                    r["achieved_measured_bytes"] = round(per_step * args.steps / (ms * 1e-3) / 1e9, 2)
                    r["frac_measured_bytes"] = round(r["achieved_measured_bytes"] / peak, 4)
            elif traffic_stale:
                r["traffic_note"] = traffic_stale
            if bound == "hbm" and streams == 1:  # (event sums of concurrent streams overlap: no rate from those)
                iv = valu_of(TRAFFIC_KEYS.get(kernel, ["\0"]))
                if iv:  # the fraction of the chip's vector issue rate the chain's instructions take: 4 cycles per wave
                    # instruction on one of 1024 SIMDs at 2.4 GHz, over the chain's time
                    r["valu_frac"] = round(iv * 4.0 / 1024.0 / 2.4e9 / (ms / args.steps * 1e-3), 4)
                    r["valu_note"] = ("SQ_INSTS_VALU of a separate --pmc pass x 4 cycles / 1024 SIMDs / 2.4 GHz over the kernel time: "
                                      "where this exceeds `frac`, vector issue and not HBM is what the chain is bound by")
            if note:
                r["note"] = note
            return r

        import ctypes
        scr_rows, scr_surv = ctypes.c_int64(0), ctypes.c_int64(0)
        capi.check(capi.lib.aps_match_screen_stats(ctypes.byref(scr_rows), ctypes.byref(scr_surv)))
        surv_share = scr_surv.value / scr_rows.value if scr_rows.value else 1.0
        cands = [
            roof("match_screen_i8", ("match_screen_i8_kernel (v_mfma_i32_32x32x32_i8, APS_SCREEN_SHAPE=32" if os.environ.get("APS_SCREEN_SHAPE") == "32"
                                     else "match_screen_i8x16_kernel (v_mfma_i32_16x16x64_i8") +
                 ": every descriptor pair once on int8 copies, "
                 "exact integer accumulation, per-row top-2, proof that a row fails the ratio/threshold filter)", "mfma",
                 flops_rank0, MFMA_I8_PEAK_TOPS, "TOP/s",
                 "achieved counts the ALGORITHMIC 2*128*Ni*Nj INTEGER multiply-adds against the dense int8 MFMA peak (5 POP/s = "
                 "twice the bf16 rate per clock at 2.4 GHz; under a dense int8 stream on random operands the chip holds 1.98 GHz "
                 "with this MFMA shape, 1.71 GHz with 32x32x32: profiles/r04a_mfma_i8_shapes.txt); "
                 f"{100 * surv_share:.1f} % of the rows survive the screen and go through match_cand_f16_kernel in row-list "
                 "mode; the match lists are bit-identical to the all-f32 path"),
            roof("match_cand_f16", "match_cand_f16_kernel (v_mfma_f32_32x32x16_f16 screening product + exact f32 rescoring" +
                 (", row-list mode on the int8 screen's survivors)" if scr_rows.value else ")"), "mfma",
                 flops_rank0 * surv_share, MFMA_BF16_PEAK_TFLOPS, "TFLOP/s",
                 "achieved counts the ALGORITHMIC 2*128*(rows it is given)*Nj flops; the kernel executes 9/8 of that on the f16 "
                 "pipe (one extra 16-wide k-step carries -b2/2 and the column's rounding-loss bound); the exact f32 rescoring of "
                 "three candidates per row runs in the kernel's tail; results are certified bit-identical to the f32 path"),
            roof("match2nn", "match2nn_kernel (v_mfma_f32_32x32x2_f32, exact f32)", "mfma", flops_rank0,
                 MFMA_F32_PEAK_TFLOPS, "TFLOP/s"),
            roof("sift_blur", "blur_kernel<R> (separable Gaussian through LDS)", "hbm", 574.0 * npix_rank0,
                 HBM_PEAK_GBS, "GB/s", "574 B per input pixel is SURVEY 8(d)'s materialised-pyramid model (G and DoG "
                 "written and re-read); the build no longer stores DoG planes, so its real traffic is lower",
                 streams=int(os.environ.get("APS_SIFT_WORKERS", str(pl.SIFT_WORKERS_DEFAULT)))),
            roof(("render_pyr_down", "render_collapse"),
                 "multiband chain, all tiles level-major (rw_down_kernel x levels, rw_up_kernel x levels incl. paint)", "hbm",
                 64.0 * a_cov + 32.0 * a_pano, HBM_PEAK_GBS, "GB/s"),
            roof("render_warp", "rw_warp_kernel (ray -> project -> bilinear gather -> normalised weight, all tiles)", "hbm",
                 16.0 * a_cov + 3.0 * npix_rank0, HBM_PEAK_GBS, "GB/s"),
        ]
        cands = [c for c in cands if c]
        # the dominant kernel launch by launch (one per step): median and minimum beside the mean
        if screen_series and cands and cands[0]["kernel"].startswith("match_screen"):
            n_l = max(1, len(screen_series) // max(args.steps, 1))
            per = [sum(screen_series[k * n_l:(k + 1) * n_l]) for k in range(len(screen_series) // n_l)]
            cands[0]["ms_per_step_median"] = round(float(np.median(per)), 3)
            cands[0]["ms_per_step_min"] = round(float(min(per)), 3)
            cands[0]["frac_median"] = round(flops_rank0 / (float(np.median(per)) * 1e-3) / 1e12 / MFMA_I8_PEAK_TOPS, 4)
        for c_ in cands:  # every entry carries both fractions: the algorithmic one and the one on the bytes the memory system moved
            c_.setdefault("frac_measured_bytes", None)
        dominant = max(cands, key=lambda c: c["wall_share_ms"]) if cands else None
        # The feature-extraction STAGE as one roofline entry (its kernels run on ten streams side by side, so per-kernel
        # event sums overlap): algorithmic bytes of SURVEY 8(d)'s materialised-pyramid model, and the bytes the stage
        # really moves (PMC pass), over the stage's wall time.
        t_feat = sum(i["times"].get("features", 0.0) for i in infos_seq) / len(infos_seq)
        if t_feat > 0:
            sift_rows = [v for k, v in traffic_db.items() if any(n_ in k for n_ in SIFT_KERNELS)]
            sift_bytes = sum(r["read_bytes_per_step"] + r["write_bytes_per_step"] for r in sift_rows) if sift_rows else None
            ach = 574.0 * npix_rank0 / t_feat / 1e9
            cands.append({"bound": "hbm", "kernel": "SIFT stage: all kernels of this rank's views on their worker streams (wall time of the stage)",
                          "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                          "traffic": round(sift_bytes) if sift_bytes else None,
                          **({"traffic_note": traffic_stale} if traffic_stale and not sift_bytes else {}),
                          "achieved_measured_bytes": round(sift_bytes / t_feat / 1e9, 2) if sift_bytes else None,
                          "frac_measured_bytes": round(sift_bytes / t_feat / 1e9 / HBM_PEAK_GBS, 4) if sift_bytes else None,
                          "algorithmic_work_per_step": 574.0 * npix_rank0, "ms_per_step": round(1e3 * t_feat, 3),
                          "note": "574 B per input pixel is the survey's model (G and DoG planes written and re-read); DoG planes are "
                                  "not stored here, so `traffic` (bytes per STEP for this entry, all SIFT kernels) is lower; "
                                  "achieved_measured_bytes = traffic / stage wall time"})
        stages = {k: round(1e3 * sum(i["times"].get(k, 0.0) for i in infos_seq) / len(infos_seq), 2) for k in infos_seq[-1]["times"]}
        stages_pipe = ({k: round(1e3 * sum(i["times"].get(k, 0.0) for i in infos) / len(infos), 2) for k in infos[-1]["times"]}
                       if pipelined else None)
        # the descriptor-distance path as a STAGE (preparation, screen, list pass, fallback, filter and their gaps): the same
        # algorithmic 2*128*Ni*Nj over the stage's wall time, beside the dominant kernel's own fraction
        t_match = sum(i["times"].get("matching", 0.0) for i in infos) / len(infos)
        matching_stage = None
        if t_match > 0 and args.matcher == "pairwise":
            matching_stage = {"ms_per_step": round(1e3 * t_match, 3), "achieved": round(flops_rank0 / t_match / 1e12, 2), "peak": MFMA_I8_PEAK_TOPS,
                              "unit": "TOP/s", "frac": round(flops_rank0 / t_match / 1e12 / MFMA_I8_PEAK_TOPS, 4),
                              "kernels_ms": {k: round(v[0] / args.steps, 3) for k, v in prof.items() if k.startswith("match")},
                              "note": "wall time of the matching stage (host phases and read-backs included) against the int8 peak"}
        kernels = {k: {"ms_per_step": round(v[0] / args.steps, 3), "launches_per_step": v[1] // max(args.steps, 1)}
                   for k, v in prof.items()}
        out = {
            "metric": "MPix/s end-to-end stitch (SIFT->blend), 64x4K images",
            "value": round(value, 2), "unit": "MPix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 2), "higher_is_better": True, "scaling": "strong",
            "ms_per_step_median": round(1e3 * float(np.median(step_walls)), 2), "ms_per_step_min": round(1e3 * min(step_walls), 2),
            "ms_per_step_series": [round(1e3 * x, 2) for x in step_walls],
            # `value`: inputs resident in HBM when the timed region starts -> cropped uint8 panorama in pinned HOST memory.
            # value_end_to_end: pinned host uint8 images -> the same (PCIe both ways; SURVEY 8(d)'s "first byte uploaded").
            # value_resident: the same steps as `value` without the device-to-host copy of the panorama.
            "value_definition": "`value` follows the build contract of this bench line (\"whole-job throughput with inputs already resident "
                                "in HBM when the timed region starts; if the boundary hands over host buffers, the PCIe-inclusive rate is "
                                "noted elsewhere - it is never `value`\"): resident uint8 views -> cropped uint8 panorama in pinned host "
                                "memory.  BASELINE.md section 2 / SURVEY 8(d)'s clock (first input byte in pinned host memory -> final "
                                "panorama in host memory) is value_end_to_end / ms_per_step_end_to_end in this same line, 0.3-0.6 % "
                                "apart (both transfers overlap device work); the reference's default gainCompensation = 1 is value_with_gain.  "
                                "Consecutive steps are pipelined (see `pipeline`); strictly sequential steps are pipeline.value_sequential",
            "value_end_to_end": round(mpix_in * args.steps / dt_e2e, 2) if dt_e2e else None,
            "ms_per_step_end_to_end": round(1e3 * dt_e2e / args.steps, 2) if dt_e2e else None,
            "value_with_gain": round(mpix_in * args.steps / dt_gain, 2) if dt_gain else None,
            "ms_per_step_with_gain": round(1e3 * dt_gain / args.steps, 2) if dt_gain else None,
            "value_resident": round(mpix_in * args.steps / dt_resident, 2),
            "ms_per_step_resident": round(1e3 * dt_resident / args.steps, 2),
            # the panorama's device-to-host copy runs beside the next step's feature extraction (two pinned buffers); alone
            # it costs download_ms_alone, so one isolated step takes ms_per_step_latency
            "download_ms_alone": round(1e3 * min(dl_alone), 2) if dl_alone else None,
            "ms_per_step_latency": round(1e3 * (sum(i["t_stitch"] for i in infos_seq) / len(infos_seq) + (min(dl_alone) if dl_alone else 0.0)), 2),
            # strictly sequential steps of the same job (no extraction of the next set beside this set's RANSAC / render)
            "pipeline": ({"on": True, "how": "the reference stitches set after set (PP/main.m:83-137: for myImg = 1:foldersLen); here the NEXT "
                          "set's feature extraction (loadImages, main.m:88-91) is started when the current set's match lists are complete "
                          "(parallel.submit_features from stitch_distributed's after_matching hook) and runs beside RANSAC, the host's graph / "
                          "camera work and the render of the current set; results per set are unchanged (bench checks pairs and canvas), "
                          "every timed step's work lies inside the timed region (the first timed step extracts its own features, the last "
                          "one starts nothing), and the int8 matching kernels still run alone",
                          "value_sequential": round(mpix_in * len(infos_seq) / dt_seq, 2), "ms_per_step_sequential": round(1e3 * dt_seq / len(infos_seq), 2),
                          "ms_per_step_sequential_median": round(1e3 * float(np.median(seq_walls)), 2),
                          "ms_per_step_sequential_series": [round(1e3 * x, 2) for x in seq_walls],
                          "stages_ms_per_step_pipelined": stages_pipe,
                          "stages_note": "stages_ms_per_step (and the SIFT-stage roofline entry) are taken from the SEQUENTIAL steps; in the "
                                         "pipelined steps `features` is what was left to wait for and `render` shares the chip with the next extraction"}
                         if pipelined else {"on": False}),
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {
                "workload": f"{n} synthetic {w}x{h} overlapping views ({nx}x{ny} yaw/pitch grid, f={f:.0f}px, "
                            f"{int(OVERLAP * 100)}% overlap): SIFT -> " + ("all-pairs exhaustive 2-NN + Lowe ratio" if args.matcher == "pairwise" else "pooled exact 4-NN of all descriptors + per-query filter (featureMatchingGlobal)") + " -> batched RANSAC -> "
                            f"host match graph/cameras ({args.cameras}) -> spherical inverse warp + {args.bands}-band multiband blend, "
                            f"tile 2048 -> cropNonzeroBbox -> panorama copied to pinned host memory; BASELINE.json configs[2].  "
                            f"`value`: inputs resident in HBM before the timed region, every step's cropped uint8 panorama is "
                            f"copied to pinned host memory (the copy of step k overlaps the matching of step k+1, all copies "
                            f"complete inside the timed region); " + ("consecutive steps are pipelined like the reference's loop over image sets "
                            "(PP/main.m:83-137): the extraction of step k+1 starts when step k's match lists are complete and runs beside its "
                            "RANSAC, camera work and render - see `pipeline`; " if pipelined else "") +
                            f"value_end_to_end adds the host-to-device upload of the images (overlapped "
                            f"with SIFT); value_resident leaves the panorama in HBM",
                "input_mpix": round(mpix_in, 1), "features_per_view": int(np.mean(counts)),
                "pairs_matched": len(order), "pairs_verified": info["n_pairs_verified"],
                "int8_screen_survivor_share": round(surv_share, 4) if scr_rows.value else None,
                "panorama": [int(pano.shape[1]), int(pano.shape[0])], "parallelism": f"{world} rank(s), images/pairs/tiles sharded",
            },
            "roofline": dominant, "rooflines_all": cands, "matching_stage": matching_stage, "gpu_state": gpu_state,
            "stages_ms_per_step": stages,
            # the same stages in the end-to-end steps; "download" = everything outside stitch_distributed (queueing the
            # uploads, the device-to-host copy of the cropped panorama and the final synchronisation)
            "stages_ms_per_step_end_to_end": ({k: round(1e3 * sum(i["times"].get(k, 0.0) for i in infos_h) / len(infos_h), 2)
                                               for k in infos_h[-1]["times"]} if dt_e2e else None),
            "stages_ms_per_step_with_gain": ({k: round(1e3 * sum(i["times"].get(k, 0.0) for i in infos_g) / len(infos_g), 2)
                                             for k in infos_g[-1]["times"]} if dt_gain else None),
            "kernels": kernels,
        }
        if world == 1 and args.matcher == "pairwise" and (nx, ny) == (NX, NY) and args.global_probe == "auto":
            # The reference's DEFAULT matcher switch (inputs.m:46, featureMatchingGlobal) on the same 64 views, outside the
            # timed region: one pass of the pooled exact 4-NN + filter with its int8 proof pass, its stage time and kernels.
            try:
                out["global_matcher_probe"] = global_matcher_probe(pl, capi, input_, [local[i] for i in range(n)])
            except Exception as e:  # a report, never a reason to lose the bench line
                out["global_matcher_probe"] = {"ms": None, "note": f"failed: {e}"}
        if world == 1:
            try:  # (a report, never a reason to lose the bench line)
                out["sift_standalone"] = sift_standalone_probe(pl, capi, input_, local[0])
                for c_ in out["rooflines_all"]:
                    if c_["kernel"].startswith("blur_kernel") and out["sift_standalone"].get("blur_chain"):
                        c_["frac_standalone"] = out["sift_standalone"]["blur_chain"]["frac"]
                        c_["standalone_note"] = ("`frac` divides by event intervals summed over ten concurrent streams (5x the stage's wall "
                                                 "time); frac_standalone = the blur chain's algorithmic bytes (48 B per octave pixel + the "
                                                 "base) over its launch sites' time for one view alone on one stream (sift_standalone)")
            except Exception as e:
                out["sift_standalone"] = {"note": f"failed: {e}"}
        if world == 1 and args.cpu_baseline == "auto":
            try:
                out["cpu_baseline"] = cpu_baseline(synth, input_, f, args.bands, float(pano.shape[0] * pano.shape[1]))
            except Exception as e:  # the baseline is a report, never a reason to lose the bench line
                out["cpu_baseline"] = {"value": None, "unit": "MPix/s", "cores": 0, "kind": "port", "sample": f"failed: {e}"}
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(out) + "\n").encode())
        if args.save_pano:
            save_pano(args.save_pano, pano)
    if multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
