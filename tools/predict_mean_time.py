"""The posterior mean from one solve (mean_weights + predict_mean, hgp_kuf_grid_matvec) against the
ways the same numbers were reached before it (GPU box), fp32, point observations, on synthetic
data of a BASELINE config's grid.

    timeout -k 10 900 python tools/predict_mean_time.py --configs C2,C5 > profiles/predict_mean_time.jsonl

One JSON line per measurement, every time the median of `--reps` warm repetitions between two
device events (milliseconds):
  mean_weights             R qm and the single-RHS solve (maxiter_cg = 50)
  predict_mean             the whole call at N = 100 (solve + product)
  product nw=1 / nw=8      kuf_grid_matvec alone at each N, with kernel evaluations per second
                           (N * M / time) and the nsplit the library would choose
  predict_fused            `predict(fused=True)` at N = 100: one right-hand side per point
  chunked_kuf_grid         kuf_grid(piece) @ alpha over pieces whose Knm stays under 256 MiB, N = 10^4
and the largest difference between the new and the old means where both were computed."""
import argparse
import json
import os
import sys

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


def run_config(name, sizes, reps, maxiter):
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
    mod = hg.MeanFieldToeplitzGP(k, grids, num_obs=100, sig2_init=params[0], ell_init=params[1], noise2_init=.01,
                                 learn_kernel=False, dtype=dt, jitter_val=jitter).cuda_params(0)
    g = torch.Generator(device="cpu").manual_seed(42)
    lo = torch.tensor([b[0] for b in BOX[d]])
    hi = torch.tensor([b[1] for b in BOX[d]])
    M = mod.M
    base = {"config": name, "M": M, "dtype": "fp32", "maxiter_cg": maxiter, "reps": reps}

    def emit(**kw):
        print(json.dumps(dict(base, **kw)), flush=True)

    with torch.no_grad():
        kp = mod.get_kernel_params()
        emit(what="mean_weights", ms=med_ms(lambda: mod.mean_weights(maxiter_cg=maxiter), reps))
        alpha = mod.mean_weights(maxiter_cg=maxiter)
        W8 = torch.cat([alpha] + [alpha * (1 + .1 * i) for i in range(1, 8)], dim=0).contiguous()
        for N in sizes:
            x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
            r = max(2, reps if N < 10 ** 6 else reps // 2)
            mu = None
            for nw, W in ((1, alpha), (8, W8)):
                ms = med_ms(lambda: kuf.kuf_grid_matvec(k, mod.xgrids, x, kp, W), r)
                emit(what=f"product nw={nw}", N=N, ms=ms, kernel_evals_per_s=N * M / (ms * 1e-3), reps=r)
            mu = kuf.kuf_grid_matvec(k, mod.xgrids, x, kp, alpha)
            if N == 100:
                emit(what="predict_mean", N=N, ms=med_ms(lambda: mod.predict_mean(x, maxiter_cg=maxiter), reps))
                emit(what="predict_fused", N=N,
                     ms=med_ms(lambda: mod.predict(x, maxiter_cg=maxiter, fused=True), max(2, reps // 2)))
                old = mod.predict(x, maxiter_cg=maxiter, fused=True)[0].reshape(-1)
                new = mod.predict_mean(x, maxiter_cg=maxiter).reshape(-1)
                emit(what="predict_mean vs predict_fused", N=N,
                     max_abs_diff=float((new - old).abs().max()), max_abs=float(old.abs().max()))
            if N == 10 ** 4:
                piece = max(1, (256 << 20) // (M * 4))

                def chunked():
                    return torch.cat([kuf.kuf_grid(k, mod.xgrids, x[a:a + piece], kp) @ alpha.t()
                                      for a in range(0, N, piece)])
                emit(what="chunked_kuf_grid", N=N, piece=piece, ms=med_ms(chunked, max(2, reps // 2)))
                emit(what="product vs chunked_kuf_grid", N=N, max_abs_diff=float((mu - chunked()).abs().max()),
                     max_abs=float(mu.abs().max()))
            del x
    hp.release_pool()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C5")
    ap.add_argument("--sizes", default="100,10000,1000000")
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for c in a.configs.split(","):
        run_config(c, [int(s) for s in a.sizes.split(",")], a.reps, a.maxiter)


if __name__ == "__main__":
    main()
