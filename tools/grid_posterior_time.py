"""grid_posterior() against per-point prediction (GPU box): the whole inducing-grid posterior (mean and
sd, two operator applications) and the first call's lazy set-up of HGP_OP_RSQ's spectrum, next to
predict(fused=True) on B points at maxiter_cg = 50 as the comparison point; fp32, synthetic
variational parameters, on a BASELINE config's grid.

    timeout -k 10 900 python tools/grid_posterior_time.py --cases C2,C5 > profiles/grid_posterior_time.jsonl

Per case one JSON line: rsq_setup_ms (first grid_posterior after the spectrum set-up minus a warm
one: the table build), grid_posterior_ms and predict_ms (HIP events around the call, after warm-up
calls; median, min and max of `reps`), rsq_table_bytes (hgp_plan_mem tables after minus before) and
the grid sizes.  A case that does not fit the card is recorded as {"oom": true}, not forced."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_configs import BOX, CONFIGS  # noqa: E402


def timed(fn, warmup, reps):
    """HIP-event times of fn() in ms (one event pair per call, the device idle before each)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "reps": reps}


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return float(a.elapsed_time(b))


def run_case(name, B, maxiter, warmup, reps):
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    from hipgp_amd import plan as hp
    dev = torch.device("cuda", 0)
    dims, (kind, nu), params, jitter, _, _, _, _ = CONFIGS[name]
    d = len(dims)
    dt = torch.float32
    k = zk.SqExp(dtype=dt) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dt)
    grids = [torch.linspace(lo, hi, m, dtype=dt) for (lo, hi), m in zip(BOX[d], dims)]
    mod = hg.MeanFieldToeplitzGP(k, grids, num_obs=B, sig2_init=params[0], ell_init=params[1], noise2_init=.01,
                                 learn_kernel=False, dtype=dt, jitter_val=jitter).cuda_params(0)
    g = torch.Generator(device="cpu").manual_seed(42)
    with torch.no_grad():
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g).to(dev))
    lo = torch.tensor([b[0] for b in BOX[d]])
    hi = torch.tensor([b[1] for b in BOX[d]])
    x = (lo + (hi - lo) * torch.rand(B, d, generator=g)).to(dev)
    out = {"config": name, "dims": list(dims), "M": mod.M, "Mprime": mod.Mprime, "dtype": "float32",
           "predict_B": B, "maxiter_cg": maxiter}
    try:
        with torch.no_grad():
            T = mod.toeplitz()
            T.set_batch_shape((1,))
            mod.grid_posterior(Kmm=T)                           # builds the table; workspaces, streams
            T2 = mod.toeplitz()                                 # a fresh spectrum set-up: no table yet
            t0 = T2._plan.mem()["tables"]
            first = once(lambda: mod.grid_posterior(Kmm=T2))
            out["rsq_table_bytes"] = T2._plan.mem()["tables"] - t0
            out["L_R"] = list(T2._plan.L_R[:d])
            gp = timed(lambda: mod.grid_posterior(Kmm=T2), warmup, reps)
            out["grid_posterior_ms"] = gp
            out["first_call_ms"] = first
            out["rsq_setup_ms"] = first - gp["median"]
            out["sample_grid_4_ms"] = timed(lambda: mod.sample_grid(4, Kmm=T2), warmup, reps)
            out["predict_ms"] = timed(lambda: mod.predict(x, maxiter_cg=maxiter, Kmm=T2, fused=True), warmup, reps)
            out["voxels_per_predict_batch"] = B
            del T, T2
    except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
        if "out of memory" not in str(e).lower() and "HGP" not in str(e) and "hipMalloc" not in str(e):
            raise
        out["oom"] = True
        out["error"] = str(e)[:200]
    print(json.dumps(out), flush=True)
    hp.release_pool()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C2,C5", help="BASELINE configs, comma separated")
    ap.add_argument("--B", type=int, default=100, help="points of the predict(fused=True) comparison")
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    for c in a.cases.split(","):
        run_case(c, a.B, a.maxiter, a.warmup, a.reps)


if __name__ == "__main__":
    main()
