"""predict fused against materialised (GPU box): time, the PCG / R^T-and-statistics split and the
memory of each mode, fp32, maxiter_cg = 50, on synthetic data of a BASELINE config's grid.

    timeout -k 10 900 python tools/predict_time.py --cases C2:100,C5:25,C5:100 > profiles/predict_time_fused_vs_materialised.jsonl

Per case and mode one JSON line: predict_s (the whole call, median of 3), pcg_s (inv_matmul alone),
tail_s (fused: rt_stats; materialised: R^T + the three torch reductions), torch_peak_bytes (peak
above the level before the call) and plan_scratch_bytes (hgp_plan_mem of the model's pooled plan).
A mode that does not fit the card is recorded as {"oom": true}, not forced."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_configs import BOX, CONFIGS  # noqa: E402


def med(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def run_case(name, B, maxiter, reps):
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
    lo = torch.tensor([b[0] for b in BOX[d]])
    hi = torch.tensor([b[1] for b in BOX[d]])
    x = (lo + (hi - lo) * torch.rand(B, d, generator=g)).to(dev)
    for fused in (True, False):
        out = {"config": name, "B": B, "maxiter_cg": maxiter, "mode": "fused" if fused else "materialised",
               "Mprime": mod.Mprime, "kn_bytes": B * mod.Mprime * 4}
        try:
            with torch.no_grad():
                out["predict_s"] = med(lambda: mod.predict(x, maxiter_cg=maxiter, fused=fused), reps)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                mod.predict(x, maxiter_cg=maxiter, fused=fused)
                torch.cuda.synchronize()
                out["torch_peak_bytes"] = torch.cuda.max_memory_allocated() - base
                out["plan_scratch_bytes"] = hp.pool_scratch_bytes(0)
                Knm, _ = mod._make_grams(x)
                T = mod.toeplitz()
                out["pcg_s"] = med(lambda: T.inv_matmul(Knm, do_precond=True, maxiter=maxiter, tol=1e-8), reps)
                d0 = T.inv_matmul(Knm, do_precond=True, maxiter=maxiter, tol=1e-8)
                qm, qS = mod.standard_variational_params()
                if fused:
                    out["tail_s"] = med(lambda: T.rt_stats(d0, qm, qS), reps)
                else:
                    def tail():
                        kn = T._matmul_by_RT(d0)
                        return kn.matmul(qm), torch.sum(kn * kn, dim=-1), mod.compute_knSkn(kn, qS)
                    out["tail_s"] = med(tail, reps)
                del T, d0, Knm
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
    ap.add_argument("--cases", default="C2:100,C5:25,C5:100", help="config:B, comma separated")
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for c in a.cases.split(","):
        name, B = c.split(":")
        run_case(name, int(B), a.maxiter, a.reps)


if __name__ == "__main__":
    main()
