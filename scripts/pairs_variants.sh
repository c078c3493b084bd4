#!/bin/bash
# usage (GPU box): scripts/pairs_variants.sh "<hipcc flags>" ...  -- rebuilds per flag set, prints the pair-kernel time of bench.py
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}; export OUT; mkdir -p "$OUT"
cd $R
for v in "$@"; do
  python3 - <<PY
from epipolarconsistency_amd import build
build.build_library(force=True, extra_flags="$v".split())
PY
  echo "== $v"
  python3 bench.py --full --steps 300 --warmup 100 --no-cpu-baseline 2>$OUT/pv_err.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('kernel_ms', d['roofline']['kernel_ms'], 'evals/s', d['value'], 'value', d['last_value'])"
done
python3 -m epipolarconsistency_amd.build --force > /dev/null
