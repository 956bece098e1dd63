"""GPU: bench.py's own N > 1 path, rehearsed on one GPU.  `python bench.py --gpus 2` starts two ranks itself; with
APS_BENCH_REHEARSE=1 both sit on device 0 and talk over gloo (RCCL refuses two ranks on one GPU), so the shard arithmetic of the
bench line, the max-over-ranks reduction and rank 0's single JSON line are walked for real.  The stitch must not depend on the
rank count: verified pairs, feature counts and the cropped panorama's size equal the one-rank run's.  Three timed steps, so that
the pipelined form (the next step's extraction started from the after_matching hook of every rank) is walked at N = 2 as well."""
import json
import os
import subprocess
import sys
from importlib import import_module

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(n_gpus, env_extra):
    env = dict(os.environ, **env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "APS_PARALLEL_FORCE_COLLECTIVES"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n_gpus), "--steps", "3", "--warmup", "1", "--full",
                        "--grid", "3x3", "--size", "1280x720", "--bands", "3", "--cpu-baseline", "off", "--end-to-end", "off",
                        "--global-probe", "off", "--with-gain", "off"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_with_two_ranks_rehearsed_on_one_gpu_equals_one_rank(gpu):
    import_module(gpu.__name__ + ".pipeline").release_device_memory()  # (two more processes are about to share this GPU)
    one = _bench(1, {})
    two = _bench(2, {"APS_BENCH_REHEARSE": "1"})
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2 and two["scaling"] == "strong"
    for key in ("pairs_verified", "pairs_matched", "features_per_view", "panorama", "input_mpix"):
        assert one["config"][key] == two["config"][key], (key, one["config"][key], two["config"][key])
    assert one["pipeline"]["on"] and two["pipeline"]["on"]
    assert two["value"] > 0 and two["roofline"] is not None and two["steps"] == 3


def test_plain_run_reports_the_headline_only_and_dumps_the_same_outputs_twice(gpu, tmp_path):
    """A plain run (no --full) prints the contract fields for exactly --steps timed steps and none of the extra legs;
    --dump-outputs writes float32 / float64 arrays under 64 MB, and a second run with the same arguments writes the same ones."""
    import numpy as np

    import_module(gpu.__name__ + ".pipeline").release_device_memory()
    dumps = []
    for k in range(2):
        out_dir = tmp_path / ("run%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--grid", "3x3", "--size", "1280x720", "--bands", "3", "--dump-outputs", str(out_dir)],
                           capture_output=True, text=True, cwd=ROOT, timeout=900)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == 3 and len(line["ms_per_step_series"]) == 3 and line["value"] > 0 and line["ms_per_step"] > 0
        for key in ("roofline", "cpu_baseline", "value_end_to_end", "value_with_gain", "pipeline", "kernels", "sift_standalone"):
            assert key not in line, key
        files = sorted(os.listdir(out_dir))
        assert "panorama_sample.npy" in files and "n_features.npy" in files and "pairs.npy" in files, files
        arrays = {f: np.load(out_dir / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64_000_000
        assert len(arrays["pairs.npy"]) > 0 and arrays["panorama_shape.npy"][:2].min() > 0
        dumps.append(arrays)
    assert sorted(dumps[0]) == sorted(dumps[1])
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name], equal_nan=True), name
