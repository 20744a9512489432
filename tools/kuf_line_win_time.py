"""The windowed line-integral Kuf products (hgp_kuf_semi_*_win, `kuf.LineWindowPlan`) against their dense twins
in the same process on one GPU, fp32, lines from the origin to ends uniform in the grid's box, tolerance 2^-24.

    timeout -k 10 900 python tools/kuf_line_win_time.py > profiles/kuf_line_win_time.jsonl

One JSON line per measurement.  Every timing lists ALL its warm repetitions between two device events
(`runs_ms`, in order) next to their median (`ms`); nothing is dropped.
  C2 (1024^2, SqExp(1, 0.01), "analytic"): both products, windowed and dense, nw = nc = 1, at 10^2, 10^3 and
      10^4 lines; one `fit_mean` iteration at 10^4 lines (wall time between the callbacks of the first and the
      last of --iters iterations); `predict_line_samples` (4 draws) at 10^3 lines; the culling share of the
      transposed product at 10^4 and 10^5 lines.
  C5 (256^2 x 128, the kernel and parameters of tools/fit_mean_time.py, "mc-biased" with 10 nodes): both
      products at 10^2, 10^3 and 10^4 lines, one `fit_mean` iteration at 10^4, `predict_line_samples` at 10^3.
Per config also rho in grid steps, and on a subsample of lines the in-window pairs (read from the kernels by
one-hot coefficients) next to the pairs of the exact Chebyshev tube (torch, fp64).
The culling share is the transposed product on the same lines with the grid moved 100 units away: every tile
still tests every line's bounding box, none survives, nothing is evaluated."""
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


def tube_pairs(x, grids, rho):
    """Pairs within Chebyshev distance rho of the segments, fp64, one line at a time."""
    mesh = torch.stack([a.reshape(-1) for a in torch.meshgrid(*[g.double() for g in grids], indexing="ij")], dim=-1)
    n = 0
    for xv in x.double():
        e0, e1 = (mesh - rho) / xv, (mesh + rho) / xv
        lo, hi = torch.minimum(e0, e1).amax(dim=-1).clamp(min=0.), torch.maximum(e0, e1).amin(dim=-1).clamp(max=1.)
        n += int((lo <= hi).sum())
    return n


def run_config(name, est, sizes, reps, fit_n, iters, samples_n, cull_sizes, sub):
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
    npts = 10
    u = torch.tensor([0.5], dtype=dt, device=dev)
    route = dict(semi_integrated_estimator=est, semi_integrated_samps=npts, mc_offset=u)
    with torch.no_grad():
        kp = mod.get_kernel_params()
        rho = kuf.support_radius(k, kp, TOL)
        steps = [rho / float(gr[1] - gr[0]) for gr in grids]
        base = {"config": name, "estimator": est, "M": M, "dtype": "fp32", "tol": TOL, "rho": rho, "rho_steps": steps,
                "grid_steps": [m - 1 for m in dims]}

        def emit(ts=None, **kw):
            if ts is not None:
                kw.update(ms=float(np.median(ts)), runs_ms=ts)
            print(json.dumps(dict(base, **kw)), flush=True)

        def products(plan, x):
            if est == "analytic":
                return (lambda W: kuf.kuf_semi_sqexp_matvec_win(plan, W), lambda C: kuf.kuf_semi_sqexp_rmatvec_win(plan, C),
                        lambda W: kuf.kuf_semi_sqexp_matvec(k, mod.xgrids, x, kp, W),
                        lambda C: kuf.kuf_semi_sqexp_rmatvec(k, mod.xgrids, x, kp, C))
            return (lambda W: kuf.kuf_semi_mc_matvec_win(plan, W, npts, u=u),
                    lambda C: kuf.kuf_semi_mc_rmatvec_win(plan, C, npts, u=u),
                    lambda W: kuf.kuf_semi_mc_matvec(k, mod.xgrids, x, kp, npts, u=u, W=W),
                    lambda C: kuf.kuf_semi_mc_rmatvec(k, mod.xgrids, x, kp, npts, u=u, C=C))

        # the window's size on a subsample: what the kernels realise, and the exact tube
        xs = (lo + (hi - lo) * torch.rand(sub, d, generator=g)).to(dev)
        # the same window under a kernel 100 units long: no in-window value underflows, so the non-zeros are the window
        plan = kuf.LineWindowPlan(k, mod.xgrids, xs, (float(kp[0]), 100.), TOL, rho=rho)
        rows = kuf.kuf_semi_mc_rmatvec_win(plan, torch.eye(sub, dtype=dt, device=dev), 2, u=u)
        emit(what="pairs on a subsample of lines", lines=sub, window_pairs=int((rows != 0).sum()),
             tube_pairs=tube_pairs(xs, mod.xgrids, rho), all_pairs=sub * M,
             pieces=[int(plan.pieces.min()), int(plan.pieces.max())])
        del rows, plan, xs
        for N in sizes:
            x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
            W = torch.randn(1, M, generator=g).to(dev)
            C = torch.randn(1, N, generator=g).to(dev)
            r = max(2, reps if N < 10 ** 4 else reps // 2)
            t0 = time.perf_counter()
            plan = kuf.LineWindowPlan(k, mod.xgrids, x, kp, TOL)
            torch.cuda.synchronize()
            emit(what="plan (once per x), wall", N=N, ms=(time.perf_counter() - t0) * 1e3)
            mvw, rmvw, mv, rmv = products(plan, x)
            win = runs_ms(lambda: mvw(W), r)
            emit(win, what="product windowed nw=1", N=N)
            dense = runs_ms(lambda: mv(W), r)
            emit(dense, what="product dense nw=1", N=N, elements=N * M)
            emit(what="product dense / windowed (medians)", N=N, ratio=float(np.median(dense) / np.median(win)))
            win = runs_ms(lambda: rmvw(C), r)
            emit(win, what="rproduct windowed nc=1", N=N)
            dense = runs_ms(lambda: rmv(C), r)
            emit(dense, what="rproduct dense nc=1", N=N, elements=N * M)
            emit(what="rproduct dense / windowed (medians)", N=N, ratio=float(np.median(dense) / np.median(win)))
            del x, W, C, plan
        for N in cull_sizes:
            x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
            C = torch.randn(1, N, generator=g).to(dev)
            plan = kuf.LineWindowPlan(k, mod.xgrids, x, kp, TOL)
            away = kuf.LineWindowPlan(k, [gr + 100. for gr in mod.xgrids], x, kp, TOL)
            away.pieces = plan.pieces
            rmvw = products(plan, x)[1]
            rcull = products(away, x)[1]
            full = runs_ms(lambda: rmvw(C), max(2, reps // 2))
            cull = runs_ms(lambda: rcull(C), max(2, reps // 2))
            emit(full, what="rproduct windowed nc=1 (for the culling share)", N=N)
            emit(cull, what="rproduct windowed nc=1, grid moved away: the bounding-box tests alone", N=N,
                 share_of_full=float(np.median(cull) / np.median(full)))
            del x, C, plan, away
        if fit_n > 0:
            N = fit_n
            x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
            y = torch.sin(6.28 * x.sum(dim=1, keepdim=True)) + .1 * torch.randn(N, 1, generator=g).to(dev)
            T = mod.toeplitz()
            for tol, label in ((TOL, "windowed"), (None, "dense")):
                mod.kuf_line_support_tol = tol
                mod.fit_mean(x, y, maxiter=2, tol=0., Kmm=T, update=False, integrated_obs=True, **route)   # warm
                walls = []
                for _ in range(2):
                    stamps = []
                    mod.fit_mean(x, y, maxiter=iters, tol=0., Kmm=T, update=False, integrated_obs=True,
                                 callback=lambda it, rr: stamps.append(time.perf_counter()), **route)
                    walls.append((stamps[-1] - stamps[0]) * 1e3 / (len(stamps) - 1))
                emit(walls, what=f"fit_mean ms per iteration, {label} (wall between the callbacks of iterations 1 "
                                 f"and {iters}; each iteration ends in a host read)", N=N, iters=iters)
            mod.kuf_line_support_tol = None
        if samples_n > 0:
            N = samples_n
            x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
            for tol, label in ((TOL, "windowed"), (None, "dense")):
                mod.kuf_line_support_tol = tol
                emit(runs_ms(lambda: mod.predict_line_samples(x, 4, nfeat=1024, **route), max(2, reps // 2)),
                     what=f"predict_line_samples, 4 draws, {label} (the plan is rebuilt per call)", N=N)
            mod.kuf_line_support_tol = None
    hp.release_pool()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--configs", default="C2,C5")
    a = ap.parse_args()
    if "C2" in a.configs:
        run_config("C2", "analytic", [10 ** 2, 10 ** 3, 10 ** 4], a.reps, 10 ** 4, a.iters, 10 ** 3, [10 ** 4, 10 ** 5], 8)
    if "C5" in a.configs:
        run_config("C5", "mc-biased", [10 ** 2, 10 ** 3, 10 ** 4], a.reps, 10 ** 4, a.iters, 10 ** 3, [10 ** 4], 4)


if __name__ == "__main__":
    main()
