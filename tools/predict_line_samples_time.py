"""Joint draws of line integrals by pathwise conditioning (predict_line_samples, hgp_rff_line_matvec)
and the fused line feature product alone beside the point product (GPU box), fp32.

    python tools/predict_line_samples_time.py          # writes profiles/predict_line_samples_time.jsonl

Without --step this process never touches the GPU: it runs each step below as a child under a
`timeout` of its own and stops at the first non-zero status; the children append their JSON lines
to --out.  One line per measurement, every time the median of `--reps` warm repetitions between two
device events (milliseconds):
  step product   at C2's kernel (SqExp(1, 0.01) on [-1, 1]^2), F = 4096, N = 10^4 and 10^6 lines / points:
    rff line nw=1 / nw=8     rff_line_matvec alone, features per second (N * F / time)
    rff point nw=1 / nw=8    rff_matvec at the same points in the same process, and the ratio line / point
  step c2        C2 = 1024^2, SqExp, analytic estimator:
    predict_line_samples n=8 the whole call at 10^4 lines (R v, the mesh product, the solve of 8 right-hand
                             sides at maxiter_cg, the semi-integrated Kuf product, the line feature
                             product), the copy to the host included; with xpoint = 10^4 points too
    predict_draws n=8        the projected draws of the same lines, for the cost of the prior half
    predict fused            `predict(integrated_obs=True, fused=True)` at 100 lines: the only other
                             route to a correct sd, one solve per line
  step c5        C5's geometry 256 x 256 x 128, Matern 5/2, "mc-biased" with 10 nodes:
    predict_line_samples n=8 at 10^3 lines; predict_draws n=8 beside it"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_configs import BOX, CONFIGS  # noqa: E402
from tools.predict_mean_time import med_ms  # noqa: E402

STEPS = (("product", 300), ("c2", 420), ("c5", 420))      # (name, seconds allowed)


def _model(name):
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    dims, (kind, nu), params, jitter, _, _, _, _ = CONFIGS[name]
    d = len(dims)
    dt = torch.float32
    k = zk.SqExp(dtype=dt) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dt)
    grids = [torch.linspace(lo, hi, m, dtype=dt) for (lo, hi), m in zip(BOX[d], dims)]
    mod = hg.MeanFieldToeplitzGP(k, grids, num_obs=100, sig2_init=params[0], ell_init=params[1], noise2_init=.01,
                                 learn_kernel=False, dtype=dt, jitter_val=jitter).cuda_params(0)
    lo = torch.tensor([b[0] for b in BOX[d]])
    hi = torch.tensor([b[1] for b in BOX[d]])
    return mod, k, params, lo, hi


def _emitter(out, **base):
    def emit(**kw):
        with open(out, "a") as f:
            f.write(json.dumps(dict(base, **kw)) + "\n")
        print(json.dumps(dict(base, **kw)), flush=True)
    return emit


def step_product(a):
    import ziggy.kernels as zk
    from hipgp_amd import rff
    dev = torch.device("cuda", 0)
    dt = torch.float32
    _, _, params, _, _, _, _, _ = CONFIGS["C2"]
    g = torch.Generator(device="cpu").manual_seed(42)
    emit = _emitter(a.out, step="product", kernel="SqExp(1, 0.01)", dtype="fp32", nfeat=a.nfeat)
    with torch.no_grad():
        omega, phase = rff.spectral_features(zk.SqExp(dtype=dt), params, 2, a.nfeat, generator=g, device=dev)
        W8 = torch.randn(8, a.nfeat, generator=g, dtype=dt).to(dev)
        scale = float(np.sqrt(2 * params[0] / a.nfeat))
        for N in (10 ** 4, 10 ** 6):
            x = (torch.rand(N, 2, generator=g) * 2 - 1).to(dev)
            r = max(2, a.reps if N < 10 ** 6 else a.reps // 2)
            for nw in (1, 8):
                line = med_ms(lambda: rff.rff_line_matvec(omega, phase, W8[:nw], x, scale=scale), r)
                point = med_ms(lambda: rff.rff_matvec(omega, phase, W8[:nw], x=x, scale=scale), r)
                emit(what=f"rff line nw={nw}", N=N, ms=line, features_per_s=N * a.nfeat / (line * 1e-3), reps=r)
                emit(what=f"rff point nw={nw}", N=N, ms=point, features_per_s=N * a.nfeat / (point * 1e-3), reps=r,
                     line_over_point=line / point)
            del x


def step_model(a, name):
    from hipgp_amd import plan as hp
    dev = torch.device("cuda", 0)
    mod, k, params, lo, hi = _model(name)
    d = len(lo)
    g = torch.Generator(device="cpu").manual_seed(42)
    c2 = name == "C2"
    N = 10 ** 4 if c2 else 10 ** 3
    route = dict(semi_integrated_estimator="analytic") if c2 else dict(semi_integrated_estimator="mc-biased",
                                                                       semi_integrated_samps=10)
    emit = _emitter(a.out, step=name.lower(), config=name, M=mod.M, dtype="fp32", nfeat=a.nfeat, maxiter_cg=a.maxiter,
                    estimator=route["semi_integrated_estimator"])
    r = max(2, a.reps // 2)
    with torch.no_grad():
        x = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
        xp = (lo + (hi - lo) * torch.rand(N, d, generator=g)).to(dev)
        call = lambda **kw: mod.predict_line_samples(x, 8, nfeat=a.nfeat, maxiter_cg=a.maxiter, **route, **kw)
        emit(what="predict_line_samples n=8", N=N, ms=med_ms(call, r), reps=r)
        emit(what="predict_line_samples n=8 with xpoint", N=N, Np=N, ms=med_ms(lambda: call(xpoint=xp), r), reps=r)
        emit(what="predict_draws n=8", N=N, reps=r,
             ms=med_ms(lambda: mod.predict_draws(x, 8, maxiter_cg=a.maxiter, integrated_obs=True, **route), r))
        if c2:
            emit(what="predict fused", N=100, reps=r,
                 ms=med_ms(lambda: mod.predict(x[:100], integrated_obs=True, maxiter_cg=a.maxiter, fused=True), r))
    hp.release_pool()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_line_samples_time.jsonl"))
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--nfeat", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.step == "product":
        return step_product(a)
    if a.step is not None:
        return step_model(a, a.step.upper())
    open(a.out, "w").close()
    for step, seconds in STEPS:
        rc = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step,
                             "--out", a.out, "--maxiter", str(a.maxiter), "--nfeat", str(a.nfeat), "--reps",
                             str(a.reps)]).returncode
        if rc != 0:
            print(f"step {step} ended with status {rc}: stopping", file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
