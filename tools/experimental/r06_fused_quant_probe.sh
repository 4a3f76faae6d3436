#!/usr/bin/env bash
# round 6: quantiser inside the mid-M GEMM launch: tests, then decode_step (initialised handles vs not) from a short bench run
set -u
cd "$(dirname "$0")/../.."
OUT="${1:?usage: tools/experimental/r06_fused_quant_probe.sh OUT_DIR}"
mkdir -p "$OUT"
timeout 900 python -m pytest tests/test_gpu_fused_quant.py -x -q 2>&1 | tail -15
timeout 900 python bench.py --tokens 65536 --steps 1 --warmup 1 --full --no-cpu-baseline --no-small-m --no-sweeps 2>"$OUT/r06_fq_bench.err" | tail -1 > "$OUT/r06_fq_bench.json"
python - "$OUT/r06_fq_bench.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
for k, v in d["decode_step"].items():
    if isinstance(v, dict):
        print(k, round(v["us_per_step"]), "us", "| not initialised:", round(v.get("handles_not_initialised", {}).get("us_per_step", 0)), "|", v.get("kernels"))
PY
