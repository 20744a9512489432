"""One mean-field natural-gradient step (elbo_and_grad) fused against materialised (GPU box): time,
the PCG / R^T-and-statistics split and the memory of each mode, fp32, on synthetic data of a
BASELINE config's grid.

    timeout -k 10 900 python tools/fit_time.py --cases C2:100,C5:25,C5:100 > profiles/fit_time_fused_vs_materialised.jsonl

Per case and mode one JSON line: step_s (the whole elbo_and_grad call, median of 3), pcg_s
(inv_matmul alone), tail_s (fused: rt_fit_stats + the (B, M) column sum + the single-RHS R^T of the
linear dm route; materialised: R^T + batch_stats, i.e. hgp_meanfield_stats), torch_peak_bytes (peak
above the level before the call) and plan_scratch_bytes (hgp_plan_mem of the model's pooled plan).
The materialised mode is elbo_and_grad(fused=False), the unchanged default path.  A mode that does
not fit the card is recorded as {"oom": true}, not forced."""
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
    y = torch.randn(B, 1, generator=g).to(dev)
    for fused in (True, False):
        out = {"config": name, "B": B, "maxiter_cg": maxiter, "mode": "fused" if fused else "materialised",
               "Mprime": mod.Mprime, "kn_bytes": B * mod.Mprime * 4}
        try:
            with torch.no_grad():
                out["step_s"] = med(lambda: mod.elbo_and_grad(x, y, maxiter_cg=maxiter, fused=fused), reps)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                mod.elbo_and_grad(x, y, maxiter_cg=maxiter, fused=fused)
                torch.cuda.synchronize()
                out["torch_peak_bytes"] = torch.cuda.max_memory_allocated() - base
                out["plan_scratch_bytes"] = hp.pool_scratch_bytes(0)
                Knm, kd = mod._make_grams(x)
                T = mod.toeplitz()
                out["pcg_s"] = med(lambda: T.inv_matmul(Knm, do_precond=True, maxiter=maxiter, tol=1e-8), reps)
                d0 = T.inv_matmul(Knm, do_precond=True, maxiter=maxiter, tol=1e-8)
                del Knm
                if fused:
                    class _Solved:      # fit_stats on the solved d0: the step without its PCG
                        column = T.column
                        rt_fit_stats = staticmethod(T.rt_fit_stats)
                        _matmul_by_RT = staticmethod(T._matmul_by_RT)
                        inv_matmul = staticmethod(lambda b, **kw: b)
                    out["tail_s"] = med(lambda: mod.fit_stats(d0, y, kd, None, maxiter_cg=maxiter, Kmm=_Solved), reps)
                else:
                    out["tail_s"] = med(lambda: mod.batch_stats(T._matmul_by_RT(d0), y, kd), reps)
                del T, d0
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
    ap.add_argument("--maxiter", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for c in a.cases.split(","):
        name, B = c.split(":")
        run_case(name, int(B), a.maxiter, a.reps)


if __name__ == "__main__":
    main()
