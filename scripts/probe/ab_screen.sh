#!/bin/bash
# A/B of the screening kernel's two MFMA shapes on the bench workload (same box, back to back).  Output under $OUT (default out/).
set -e
OUT=${OUT:-out}
mkdir -p "$OUT"
python -m pytest tests/test_match_gpu.py tests/test_global_gpu.py tests/test_golden.py -m gpu -x -q > "$OUT/t_match.txt" 2>&1 || { tail -30 "$OUT/t_match.txt"; exit 1; }
tail -1 "$OUT/t_match.txt"
for shape in 16 32 16 32; do
  APS_SCREEN_SHAPE=$shape python bench.py --full --steps 4 --warmup 2 --cpu-baseline off --end-to-end off --global-probe off > "$OUT/b$shape.json" 2> "$OUT/b$shape.err"
  python - <<PY
import json
d=json.load(open("$OUT/b$shape.json"))
print("shape $shape", d["value"], d["ms_per_step"], "matching", d["stages_ms_per_step"]["matching"], {k:v["ms_per_step"] for k,v in d["kernels"].items() if k.startswith("match")}, d["config"]["int8_screen_survivor_share"])
PY
done
