"""One block-family natural-gradient step (BlockToeplitzGP.elbo_and_grad) streamed against
materialised (GPU box): time, the PCG / R^T-and-statistics split and the memory of each mode, fp32,
on synthetic data of a BASELINE config's grid.

    timeout -k 10 1100 python tools/block_fit_time.py > profiles/block_fit_time.jsonl

A case is config:B:blocks[:pieces], e.g. C2:100:11x11:0/8/32/100 (pieces: kn_piece_rhs values, 0 =
the library's default rule min(B, max(32 Mi / M', bs))).  The block sides must divide the expanded
grid n = 2m - 2: C2's n = 2046 = 2 * 3 * 11 * 31 has no 10 x 10 tiling, so its cases take 11 x 11
(121 points per block), the nearest shape that tiles it; C5's n = (510, 510, 254) takes 5 x 5 x 2.

Per case, mode and piece one JSON line: step_s (the whole elbo_and_grad call, median of `reps`, with
step_min_s / step_max_s as the run-to-run spread), pcg_s (inv_matmul alone), tail_s (streamed:
rt_block_stats + the (B, M) column sum + the single-RHS R^T of the linear dm route; materialised:
R^T + batch_stats, i.e. hgp_block_stats + hgp_meanfield_stats), torch_peak_bytes (peak above the
level before the call) and plan_scratch_bytes (hgp_plan_mem of the model's pooled plan).  The
materialised mode is elbo_and_grad(streamed=False), the unchanged default path.  A mode that does
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


def times(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def med(fn, reps=3):
    return float(np.median(times(fn, reps)))


def run_case(name, B, blocks, pieces, maxiter, reps):
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    from hipgp_amd import plan as hp
    dev = torch.device("cuda", 0)
    dims, (kind, nu), params, jitter, _, _, _, _ = CONFIGS[name]
    d = len(dims)
    dt = torch.float32
    k = zk.SqExp(dtype=dt) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dt)
    grids = [torch.linspace(lo, hi, m, dtype=dt) for (lo, hi), m in zip(BOX[d], dims)]
    mod = hg.BlockToeplitzGP(k, grids, num_obs=B, block_sizes=list(blocks), sig2_init=params[0], ell_init=params[1],
                             noise2_init=.01, learn_kernel=False, dtype=dt, jitter_val=jitter).cuda_params(0)
    g = torch.Generator(device="cpu").manual_seed(42)
    lo = torch.tensor([b[0] for b in BOX[d]])
    hi = torch.tensor([b[1] for b in BOX[d]])
    x = (lo + (hi - lo) * torch.rand(B, d, generator=g)).to(dev)
    y = torch.randn(B, 1, generator=g).to(dev)
    for mode, piece in [("streamed", p) for p in pieces] + [("materialised", None)]:
        streamed = mode == "streamed"
        mod.kn_piece_rhs = piece or 0
        out = {"config": name, "B": B, "blocks": list(blocks), "bs": mod.block_size, "maxiter_cg": maxiter, "mode": mode,
               "kn_piece_rhs": piece, "Mprime": mod.Mprime, "kn_bytes": B * mod.Mprime * 4,
               "gram_bytes": mod.Mprime * mod.block_size * 4}
        try:
            with torch.no_grad():
                ts = times(lambda: mod.elbo_and_grad(x, y, maxiter_cg=maxiter, streamed=streamed), reps)
                out["step_s"], out["step_min_s"], out["step_max_s"] = float(np.median(ts)), min(ts), max(ts)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                mod.elbo_and_grad(x, y, maxiter_cg=maxiter, streamed=streamed)
                torch.cuda.synchronize()
                out["torch_peak_bytes"] = torch.cuda.max_memory_allocated() - base
                out["plan_scratch_bytes"] = hp.pool_scratch_bytes(0)
                Knm, kd = mod._make_grams(x)
                T = mod.toeplitz()
                out["pcg_s"] = med(lambda: T.inv_matmul(Knm, do_precond=True, maxiter=maxiter, tol=1e-8), reps)
                d0 = T.inv_matmul(Knm, do_precond=True, maxiter=maxiter, tol=1e-8)
                del Knm
                if streamed:
                    class _Solved:      # streamed_fit_stats on the solved d0: the step without its PCG
                        column = T.column
                        rt_block_stats = staticmethod(T.rt_block_stats)
                        _matmul_by_RT = staticmethod(T._matmul_by_RT)
                        inv_matmul = staticmethod(lambda b, **kw: b)
                    out["tail_s"] = med(lambda: mod.streamed_fit_stats(d0, y, kd, None, maxiter_cg=maxiter,
                                                                       Kmm=_Solved), reps)
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
    ap.add_argument("--cases", default="C2:100:11x11:0/8/32/100,C2:200:11x11:0/8/32/100,C5:25:5x5x2:0",
                    help="config:B:blocks[:pieces], comma separated; blocks AxB[xC], pieces p/q/...")
    ap.add_argument("--maxiter", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for c in a.cases.split(","):
        f = c.split(":")
        pieces = [int(p) for p in f[3].split("/")] if len(f) > 3 else [0]
        run_case(f[0], int(f[1]), tuple(int(b) for b in f[2].split("x")), pieces, a.maxiter, a.reps)


if __name__ == "__main__":
    main()
