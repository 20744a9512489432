#!/bin/bash
# quick check: bench (per-pass times) + the parity / CG / large-grid GPU tests
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}   # where the result files go
mkdir -p "$OUT"
timeout -k 10 200 python bench.py --full --no-cpu-baseline > "$OUT/bench_q.json" 2> "$OUT/bench_q.err" || { tail -20 "$OUT/bench_q.err"; exit 1; }
python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["OUT"], "bench_q.json")).read().strip().splitlines()[-1])
r = d["roofline"]
print("value", round(d["value"]), "ms/step", round(d["ms_per_step"], 4), "frac", round(r["frac"], 3),
      "ev_ms", round(r["event_op_ms"], 4), "pcg_ms", round(d["pcg_wall_clock_ms"], 2), "passes", [(p["ms"], p["gbs"]) for p in r["passes"]])
PY
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread ${PYTEST_ARGS:-} > "$OUT/pytest_q.log" 2>&1 || { tail -40 "$OUT/pytest_q.log"; exit 1; }
tail -1 "$OUT/pytest_q.log"
