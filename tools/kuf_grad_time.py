"""Kernel hyper-parameter learning with the fused Kuf backward (the model's `kuf_grad` knob) on and
off (GPU box): time and memory of `_make_grams` forward + backward and of one learn_kernel step,
fp32, mean-field family, on synthetic data of a BASELINE config's grid.

    python tools/kuf_grad_time.py --out profiles/kuf_grad_time.jsonl

Cases: C2 (1024^2, B = 32, SqExp, point observations) and C5 (256^2 x 128, B = 25, its Matern 5/2,
line-integral observations by the mc-biased estimator with 10 samples).  Per case and knob one JSON
line:
  grams_s / grams_peak_bytes   Knm, Knn = _make_grams(...); Knm.backward(G) with a fixed random G
  step_s / step_peak_bytes     elbo_and_grad(...).backward(): the whole learn_kernel step
times are host clocks around a device synchronise after one warm-up call, median of --reps (>= 3)
calls; peaks are torch.cuda.max_memory_allocated above the level before the call (G, x and the
model excluded).  The knob-off route is the unchanged default path (the torch kernel's broadcast
under autograd).  A route that does not fit the card is recorded as {"oom": true} and not tried
again.  Every (case, knob) runs in a child process of its own under a time limit; after a child
that was killed or crashed nothing more is started."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"C2": dict(B=32, integrated=False), "C5": dict(B=25, integrated=True, npts=10)}


def med(fn, reps):
    import numpy as np
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def peak_of(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def is_oom(e):
    import torch
    s = str(e).lower()
    return isinstance(e, torch.cuda.OutOfMemoryError) or "out of memory" in s or "hipmalloc" in s


def run_child(name, knob, maxiter, reps):
    import torch
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    from tools.bench_configs import BOX, CONFIGS
    case = CASES[name]
    B = case["B"]
    dev = torch.device("cuda", 0)
    dims, (kind, nu), params, jitter, _, _, _, _ = CONFIGS[name]
    d, dt = len(dims), torch.float32
    k = zk.SqExp(dtype=dt) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dt)
    grids = [torch.linspace(lo, hi, m, dtype=dt) for (lo, hi), m in zip(BOX[d], dims)]
    mod = hg.MeanFieldToeplitzGP(k, grids, num_obs=B, sig2_init=params[0], ell_init=params[1], noise2_init=.01,
                                 learn_kernel=True, learn_noise=False, dtype=dt, jitter_val=jitter).cuda_params(0)
    mod.kuf_grad = knob == "on"
    g = torch.Generator(device="cpu").manual_seed(42)
    lo = torch.tensor([b[0] for b in BOX[d]])
    hi = torch.tensor([b[1] for b in BOX[d]])
    x = (lo + (hi - lo) * torch.rand(B, d, generator=g)).to(dev)
    y = torch.randn(B, 1, generator=g).to(dev)
    gram_kw = {}
    if case["integrated"]:
        gram_kw = dict(integrated_obs=True, semi_integrated_estimator="mc-biased",
                       semi_integrated_samps=case["npts"])
        mod.kernel.diag_interp            # the doubly-integrated table (host quadrature), outside the timing
    G = torch.randn(B, mod.M, generator=g).to(dev)
    out = {"config": name, "B": B, "kuf_grad": knob, "maxiter_cg": maxiter, "reps": reps, "M": mod.M,
           "knm_bytes": B * mod.M * 4, "observations": "line-integral mc-biased" if case["integrated"] else "point"}

    def grams():
        mod.zero_grad(set_to_none=False)
        Knm, _ = mod._make_grams(x, **gram_kw)
        Knm.backward(G)

    def step():
        mod.zero_grad(set_to_none=False)
        mod.elbo_and_grad(x, y, maxiter_cg=maxiter, **gram_kw).backward()

    for key, fn in (("grams", grams), ("step", step)):
        try:
            out[key + "_s"] = med(fn, reps)
            out[key + "_peak_bytes"] = peak_of(fn)
        except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
            if not is_oom(e):
                raise
            out["oom"] = True
            out["oom_in"] = key
            out["error"] = str(e)[:200]
            break                              # recorded, not retried
    out["log_ell_grad"] = float(mod.log_ell.grad) if mod.log_ell.grad is not None else None
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C2,C5")
    ap.add_argument("--maxiter", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=280, help="time limit of one (case, knob) child, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kuf_grad_time.jsonl"))
    ap.add_argument("--child", nargs=2, metavar=("CASE", "KNOB"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.reps >= 3
    if a.child:
        run_child(a.child[0], a.child[1], a.maxiter, a.reps)
        return 0
    lines = []
    for name in a.cases.split(","):
        for knob in ("off", "on"):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", name,
                   knob, "--maxiter", str(a.maxiter), "--reps", str(a.reps)]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                print(f"{name} kuf_grad={knob}: child ended with status {p.returncode}; stopping", file=sys.stderr)
                with open(a.out, "w") as f:
                    f.write("".join(ln + "\n" for ln in lines))
                return 1
            print(res[-1], flush=True)
            lines.append(res[-1])
    with open(a.out, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
