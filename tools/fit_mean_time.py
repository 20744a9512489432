"""The optimal variational mean from one matrix-free solve (`fit_mean`: hgp_kuf_grid_rmatvec with
hgp_kuf_grid_matvec and the K matvec) on a GPU box, fp32, point observations, on synthetic data of a
BASELINE config's grid.

    timeout -k 10 900 python tools/fit_mean_time.py --configs C2,C5 > profiles/fit_mean_time.jsonl

One JSON line per measurement, every time the median of `--reps` warm repetitions between two
device events (milliseconds):
  rproduct nc=1 / nc=8     kuf_grid_rmatvec alone at each N, with kernel evaluations per second
                           (N * M / time); the forward product's figures are in
                           profiles/predict_mean_time.jsonl
  product nw=1             kuf_grid_matvec at N = --fit-n, for the split of an iteration
  K, Cinv                  one single-RHS K matvec / C^-1 apply
  fit_mean                 the solve at N = --fit-n: the iterations at which |r|/|b| first fell under
                           1e-4 and 1e-6 (null where it did not within --maxiter iterations or
                           --budget seconds), the wall time per iteration and its split into K,
                           Kuf., Kuf^T. and the rest (C^-1, the dots and updates, one host read)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_configs import BOX, CONFIGS  # noqa: E402


def med_ms(fn, reps):
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
    return float(np.median(ts))


class _Budget(Exception):
    pass


def run_config(name, sizes, reps, fit_n, maxiter, budget):
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    from hipgp_amd import kuf
    from hipgp_amd import plan as hp
    dev = torch.device("cuda", 0)
    dims, (kind, nu), params, jitter, _, _, _, _ = CONFIGS[name]
    d = len(dims)
    dt = torch.float32
    k = zk.SqExp(dtype=dt) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dt)
    grids = [torch.linspace(lo, hi, m, dtype=dt) for (lo, hi), m in zip(BOX[d], dims)]
    mod = hg.MeanFieldToeplitzGP(k, grids, num_obs=fit_n, sig2_init=params[0], ell_init=params[1], noise2_init=.01,
                                 learn_kernel=False, dtype=dt, jitter_val=jitter).cuda_params(0)
    g = torch.Generator(device="cpu").manual_seed(42)
    lo = torch.tensor([b[0] for b in BOX[d]])
    hi = torch.tensor([b[1] for b in BOX[d]])
    M = mod.M
    base = {"config": name, "M": M, "dtype": "fp32", "reps": reps}

    def emit(**kw):
        print(json.dumps(dict(base, **kw)), flush=True)

    with torch.no_grad():
        kp = mod.get_kernel_params()
        for N in sizes:
            x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
            C8 = torch.randn(8, N, generator=g).to(dev)
            r = max(2, reps if N < 10 ** 6 else reps // 2)
            for nc in (1, 8):
                ms = med_ms(lambda: kuf.kuf_grid_rmatvec(k, mod.xgrids, x, kp, C8[:nc]), r)
                emit(what=f"rproduct nc={nc}", N=N, ms=ms, kernel_evals_per_s=N * M / (ms * 1e-3), reps=r)
            del x, C8
        # fit_mean at fit_n observations of a smooth function plus noise
        N = fit_n
        x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
        span = (hi - lo).to(dev)
        y = torch.sin(6.28 * (x / span).sum(dim=1, keepdim=True)) + .1 * torch.randn(N, 1, generator=g).to(dev)
        T = mod.toeplitz()
        T.set_batch_shape((1,))
        p = torch.randn(1, M, generator=g).to(dev)
        c = torch.randn(1, N, generator=g).to(dev)
        ms_k = med_ms(lambda: T._matmul_by_K(p), reps)
        ms_cinv = med_ms(lambda: T._matmul_by_Cinv(p), reps)
        ms_fwd = med_ms(lambda: kuf.kuf_grid_matvec(k, mod.xgrids, x, kp, p), reps)
        ms_rev = med_ms(lambda: kuf.kuf_grid_rmatvec(k, mod.xgrids, x, kp, c), reps)
        emit(what="K", ms=ms_k)
        emit(what="Cinv", ms=ms_cinv)
        emit(what="product nw=1", N=N, ms=ms_fwd, kernel_evals_per_s=N * M / (ms_fwd * 1e-3))
        first = {1e-4: None, 1e-6: None}
        t0 = time.perf_counter()

        def cb(it, rr):
            for tol in first:
                if first[tol] is None and rr < tol:
                    first[tol] = it
            if time.perf_counter() - t0 > budget:
                raise _Budget()

        last = {}

        def cb2(it, rr):
            last["it"], last["rr"] = it, rr
            cb(it, rr)

        stopped = "tol"
        try:
            fit = mod.fit_mean(x, y, maxiter=maxiter, tol=1e-6, Kmm=T, update=False, callback=cb2)
            iters, relres = fit.iters, fit.relres
            if relres >= 1e-6:
                stopped = "maxiter"
        except _Budget:
            iters, relres, stopped = last["it"], last["rr"], "budget"
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        per = wall / max(iters, 1)
        emit(what="fit_mean", N=N, iters=iters, relres=relres, stopped=stopped, wall_ms=wall, ms_per_iter=per,
             ms_K=ms_k, ms_Kuf=ms_fwd, ms_KufT=ms_rev, ms_rest=per - ms_k - ms_fwd - ms_rev, maxiter=maxiter, budget_s=budget,
             **{"iters_to_1e-4": first[1e-4], "iters_to_1e-6": first[1e-6]})
    hp.release_pool()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C5")
    ap.add_argument("--sizes", default="100,10000,1000000")
    ap.add_argument("--fit-n", type=int, default=10000)
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--budget", type=float, default=150., help="seconds of fit_mean per config")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for c in a.configs.split(","):
        run_config(c, [int(s) for s in a.sizes.split(",")], a.reps, a.fit_n, a.maxiter, a.budget)


if __name__ == "__main__":
    main()
