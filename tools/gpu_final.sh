#!/bin/bash
# Round-end evidence: GPU tests, the full bench line (with CPU baseline), rocprofv3 kernel
# stats of the bench, PMC HBM traffic of the K matvec.  Each GPU step has its own limit.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
OUT=${OUT:-bench_out}   # where the result files go
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || { tail -30 "$OUT/pytest_gpu.log"; exit 1; }
tail -1 "$OUT/pytest_gpu.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { tail -20 "$OUT/smoke.log"; exit 1; }
tail -1 "$OUT/smoke.log"
timeout -k 10 400 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || { tail -20 "$OUT/bench.err"; exit 1; }
tail -1 "$OUT/bench.json"
bash tools/profile.sh ${TAG:-final} || exit 1
bash tools/pmc_kop.sh > "$OUT/pmc_kop.log" 2>&1 || { tail -20 "$OUT/pmc_kop.log"; exit 1; }
grep traffic_bytes_per_op gpurun_out/pmc_kop/pmc_kop_C2.json
