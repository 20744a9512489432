"""The windowed Kuf products (hgp_kuf_grid_matvec_win / hgp_kuf_grid_rmatvec_win, `kuf.WindowPlan`) against
their dense twins in the same session on one GPU box, fp32, point observations uniform in the grid's box,
tolerance 2^-24.

    timeout -k 10 900 python tools/kuf_win_time.py > profiles/kuf_win_time.jsonl

One JSON line per measurement.  Every timing lists ALL its warm repetitions between two device events
(`runs_ms`, in order) next to their median (`ms`); nothing is dropped.
  C2 (1024^2, SqExp(1, 0.01)): both products, windowed and dense, nw = nc = 1, at N = 10^4 and 10^6; the
      plan's sort into bins once per N; one `fit_mean` iteration at N = 10^4 (wall time between the
      callbacks of the first and the last of --iters iterations, windowed and dense; three such runs
      each); `predict_mean` at 10^6 points with the weights given
      (the product, the copy to the host and nothing else).
  C4 (4096^2, Matern-3/2(0.1, 0.1)): both products at N = 10^4, where the radius covers most of the
      grid: the unfavourable case."""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_configs import BOX, CONFIGS  # noqa: E402

TOL = 2.0 ** -24


def runs_ms(fn, reps):
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
    return ts


def run_config(name, sizes, reps, fit_n, iters, predict_n):
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
    with contextlib.redirect_stdout(sys.stderr):          # the model announces itself: keep stdout JSON lines only
        mod = hg.MeanFieldToeplitzGP(k, grids, num_obs=max(fit_n, 1), sig2_init=params[0], ell_init=params[1],
                                     noise2_init=.01, learn_kernel=False, dtype=dt, jitter_val=jitter).cuda_params(0)
    g = torch.Generator(device="cpu").manual_seed(42)
    lo = torch.tensor([b[0] for b in BOX[d]])
    hi = torch.tensor([b[1] for b in BOX[d]])
    M = mod.M
    with torch.no_grad():
        kp = mod.get_kernel_params()
        rho = kuf.support_radius(k, kp, TOL)
        steps = [rho / float(gr[1] - gr[0]) for gr in grids]
        base = {"config": name, "M": M, "dtype": "fp32", "tol": TOL, "rho": rho, "rho_steps": steps}

        def emit(ts=None, **kw):
            if ts is not None:
                kw.update(ms=float(np.median(ts)), runs_ms=ts)
            print(json.dumps(dict(base, **kw)), flush=True)

        for N in sizes:
            x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
            W = torch.randn(1, M, generator=g).to(dev)
            C = torch.randn(1, N, generator=g).to(dev)
            r = max(2, reps if N < 10 ** 6 else reps // 2)
            t0 = time.perf_counter()
            plan = kuf.WindowPlan(k, mod.xgrids, x, kp, TOL)
            plan.bins()
            torch.cuda.synchronize()
            emit(what="plan + bins (once per x), wall", N=N, ms=(time.perf_counter() - t0) * 1e3)
            pairs = N * float(np.prod([min(2 * s + 1, m) for s, m in zip(steps, dims)]))
            win = runs_ms(lambda: kuf.kuf_grid_matvec_win(plan, W), r)
            emit(win, what="product windowed nw=1", N=N, window_pairs_at_most=pairs)
            dense = runs_ms(lambda: kuf.kuf_grid_matvec(k, mod.xgrids, x, kp, W), r)
            emit(dense, what="product dense nw=1", N=N, kernel_evals=N * M)
            emit(what="product dense / windowed (medians)", N=N, ratio=float(np.median(dense) / np.median(win)))
            win = runs_ms(lambda: kuf.kuf_grid_rmatvec_win(plan, C), r)
            emit(win, what="rproduct windowed nc=1", N=N, window_pairs_at_most=pairs)
            dense = runs_ms(lambda: kuf.kuf_grid_rmatvec(k, mod.xgrids, x, kp, C), r)
            emit(dense, what="rproduct dense nc=1", N=N, kernel_evals=N * M)
            emit(what="rproduct dense / windowed (medians)", N=N, ratio=float(np.median(dense) / np.median(win)))
            del x, W, C, plan
        if fit_n > 0:
            N = fit_n
            x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
            span = (hi - lo).to(dev)
            y = torch.sin(6.28 * (x / span).sum(dim=1, keepdim=True)) + .1 * torch.randn(N, 1, generator=g).to(dev)
            T = mod.toeplitz()
            for tol, label in ((TOL, "windowed"), (None, "dense")):
                mod.kuf_support_tol = tol
                mod.fit_mean(x, y, maxiter=2, tol=0., Kmm=T, update=False)                  # warm
                walls = []
                for _ in range(3):
                    stamps = []
                    mod.fit_mean(x, y, maxiter=iters, tol=0., Kmm=T, update=False,
                                 callback=lambda it, rr: stamps.append(time.perf_counter()))
                    walls.append((stamps[-1] - stamps[0]) * 1e3 / (len(stamps) - 1))
                emit(walls, what=f"fit_mean ms per iteration, {label} (wall between the callbacks of iterations 1 "
                                 f"and {iters}; each iteration ends in a host read)", N=N, iters=iters)
            mod.kuf_support_tol = None
        if predict_n > 0:
            N = predict_n
            x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
            alpha = torch.randn(1, M, generator=g).to(dev)
            for tol, label in ((TOL, "windowed"), (None, "dense")):
                mod.kuf_support_tol = tol
                emit(runs_ms(lambda: mod.predict_mean(x, weights=alpha), max(2, reps // 2)),
                     what=f"predict_mean, weights given, {label} (the plan is rebuilt per call)", N=N)
            mod.kuf_support_tol = None
    hp.release_pool()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    run_config("C2", [10 ** 4, 10 ** 6], a.reps, 10 ** 4, a.iters, 10 ** 6)
    run_config("C4", [10 ** 4], a.reps, 0, a.iters, 0)


if __name__ == "__main__":
    main()
