"""bench.py end to end on the GPU (short runs): one JSON line with the driver's contract fields.
A plain run carries the headline figure alone and, with --dump-outputs, writes the last timed
step's K matvec (checked against the fp64 oracle); with --full the line also holds the roofline
block of the batched K matvec (frac below 1, PMC traffic from the committed summary), the per-pass
HIP-event times and the compute_kn wall-clock -- so a change that breaks the driver's bench line
fails here first."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "roofline")


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_bench_line_contract():
    d = _bench("--full", "--steps", "3", "--warmup", "1", "--pcg-reps", "1", "--settle-s", "0",
               "--no-cpu-baseline", "--no-legs")
    for k in CONTRACT + ("pcg_wall_clock_ms",):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
    r = d["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] < 1 and r["peak"] == 8000.0
    assert abs(r["achieved"] - r["bytes_per_launch"] / (d["ms_per_step"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert r["traffic"] is not None and r["traffic"] > r["bytes_per_launch"]
    assert len(r["passes"]) == 3 and all(ps["ms"] > 0 for ps in r["passes"])
    assert d["config"]["workload"].startswith("C2")


def test_bench_plain_run_and_dump(tmp_path):
    """A plain run: the contract fields with ms_per_step = the timed steps' own clock, nothing of
    what --full measures, and --dump-outputs = the K matvec of the benchmark's own inputs (odd
    sizes, whole output; fp32 bound of __graft_entry__.smoke's K matvec check)."""
    m, B = 250, 3
    d = _bench("--steps", "4", "--warmup", "2", "--m", str(m), "--rhs", str(B), "--dump-outputs", str(tmp_path))
    for k in CONTRACT:
        assert k in d, k
    assert d["steps"] == 4 and d["warmup"] == 2 and d["dtype"] == "f32" and d["unit"] == "RHS-matvecs/s"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("pcg_wall_clock_ms", "pcg", "cpu_baseline", "strong", "elbo_step", "strong_c4"):
        assert k not in d, k
    assert "passes" not in d["roofline"] and "event_op_ms" not in d["roofline"]
    assert sorted(os.listdir(tmp_path)) == ["kmatvec.npy"]
    y = np.load(tmp_path / "kmatvec.npy")
    assert y.dtype == np.float32 and y.shape == (B, m * m)

    import torch
    sys.path.insert(0, ROOT)
    import bench
    from oracle import ziggy_oracle as zo
    _, _, Knm = bench.make_problem(m, B, torch.device("cuda:0"), seed=1234)
    g = [np.linspace(-1, 1, m) for _ in range(2)]
    T = zo.ToeplitzOracle(zo.toeplitz_column(g, lambda a, b: zo.kernel_eval("sqexp", a, b, (1., .01)), 1e-3), (m, m))
    ref = T.matmul_K(Knm.double().cpu().numpy())
    err = float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))
    print(f"bench dump vs fp64 oracle: max rel.err = {err:.3e}")
    assert err < 1e-5, err
