#!/bin/bash
# Tuning visit for the sweep crossing: geometry / crossing tests, then bench.py.
# Usage: bash scripts/gpu_cross.sh <tag>
set -u
TAG=${1:-cross}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/gpurun_out/$TAG
mkdir -p $OUT
cd $R
( timeout 600 python -m pytest tests/test_geometry.py tests/test_full_size.py -m gpu -x -q 2>&1 | tail -15 ) > $OUT/pytest.log
( timeout 300 python bench.py --no-cpu-baseline --steps 20 --warmup 3 2>&1 | tail -1 | python -c '
import sys, json
l = sys.stdin.read().strip()
try:
    d = json.loads(l)
    print("value %.1f M  ms/step %.3f  breakdown %s  frac64 %.3f" % (d["value"] / 1e6, d["ms_per_step"], d["step_breakdown_ms"], d["roofline_fp64_valu"]["frac"]))
except Exception as e:
    print("FAILED", l[-2000:])
' ) >> $OUT/bench.log
( timeout 300 python bench.py --no-cpu-baseline --steps 20 --warmup 3 --xi-out 2>&1 | tail -1 | cut -c1-400 ) > $OUT/bench_xi.log
cat $OUT/pytest.log $OUT/bench.log $OUT/bench_xi.log
