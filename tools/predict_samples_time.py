"""Joint draws of f at arbitrary points by pathwise conditioning (predict_samples, hgp_rff_matvec)
and the fused Fourier-feature product alone (GPU box), fp32, point observations, on a BASELINE
config's grid.

    timeout -k 10 900 python tools/predict_samples_time.py --configs C2 > profiles/predict_samples_time.jsonl

One JSON line per measurement, every time the median of `--reps` warm repetitions between two
device events (milliseconds):
  rff nw=1 / nw=8          rff_matvec alone at each N explicit points, with cosines per second
                           (N * F / time)
  rff mesh nw=8            rff_matvec on the whole inducing mesh, transposed and accumulated in place
                           (the right-hand side of predict_samples), cosines per second (M * F / time)
  predict_samples n=8      the whole call at N = 10^4 (R v, the mesh product, the solve of 8
                           right-hand sides at maxiter_cg, the Kuf product, the feature product),
                           the copy to the host included
  predict_draws n=8        the projected draws at the same points, for the cost of the prior half
Run tools/predict_mean_time.py in the same session for `predict(fused=True)` at N = 100, the only
other route to a correct sd (one solve per point)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_configs import BOX, CONFIGS  # noqa: E402
from tools.predict_mean_time import med_ms  # noqa: E402


def run_config(name, sizes, reps, maxiter, nfeat):
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    from hipgp_amd import plan as hp
    from hipgp_amd import rff
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
    base = {"config": name, "M": M, "dtype": "fp32", "nfeat": nfeat, "maxiter_cg": maxiter, "reps": reps}

    def emit(**kw):
        print(json.dumps(dict(base, **kw)), flush=True)

    with torch.no_grad():
        omega, phase = rff.spectral_features(k, mod.get_kernel_params(), d, nfeat, generator=g, device=dev)
        W8 = torch.randn(8, nfeat, generator=g, dtype=dt).to(dev)
        scale = float(np.sqrt(2 * params[0] / nfeat))
        for N in sizes:
            x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
            r = max(2, reps if N < 10 ** 6 else reps // 2)
            for nw in (1, 8):
                ms = med_ms(lambda: rff.rff_matvec(omega, phase, W8[:nw], x=x, scale=scale), r)
                emit(what=f"rff nw={nw}", N=N, ms=ms, cosines_per_s=N * nfeat / (ms * 1e-3), reps=r)
            if N == 10 ** 4:
                ms = med_ms(lambda: mod.predict_samples(x, 8, nfeat=nfeat, maxiter_cg=maxiter), max(2, reps // 2))
                emit(what="predict_samples n=8", N=N, ms=ms)
                emit(what="predict_draws n=8", N=N,
                     ms=med_ms(lambda: mod.predict_draws(x, 8, maxiter_cg=maxiter), max(2, reps // 2)))
            del x
        b = torch.zeros(8, M, dtype=dt, device=dev)
        ms = med_ms(lambda: rff.rff_matvec(omega, phase, W8, xgrids=mod.xgrids, scale=-scale, transposed=True, out=b,
                                           beta=1.0), max(2, reps // 2))
        emit(what="rff mesh nw=8", N=M, ms=ms, cosines_per_s=M * nfeat / (ms * 1e-3))
    hp.release_pool()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2")
    ap.add_argument("--sizes", default="10000,1000000")
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--nfeat", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for c in a.configs.split(","):
        run_config(c, [int(s) for s in a.sizes.split(",")], a.reps, a.maxiter, a.nfeat)


if __name__ == "__main__":
    main()
