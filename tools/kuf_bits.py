"""The bits of every entry point of the Kuf / RFF product family for a fixed seed: one SHA-256 per output,
written as one JSON object.  Run it against two builds of the library on the same device and compare the
files; a change that is meant to leave the arithmetic alone must leave them identical.

    timeout -k 10 300 python tools/kuf_bits.py --out bits_new.json
    HGP_LIB=/path/to/other/libhipgp.so timeout -k 10 300 python tools/kuf_bits.py --out bits_old.json
    cmp bits_old.json bits_new.json

Entries: the forwards (grid, semi-mc, semi-sqexp), the dense matvec / rmatvec in their three modes, the
windowed point products, the windowed line products in both modes, both RFF products; the (sig2, ell)
gradients of the three forwards, through the `_ad` functions with a fixed upstream G; with one length scale per
axis (a list `ell`, `SqExp(ard=True)`) the forward, the dense and the windowed point products and the gradient.
Shapes are small and
chosen so that every path of the launchers runs: grids (5,), (3, 70), (2, 3, 70) (the last axis crosses a
64-lane tile with a tail); 3 and 257 observations (past one 256-observation run or chunk); 1, 3 and 9 weight
or coefficient rows (groups of 1, 4 and 8 + 1); nsplit 1 and 2 where the entry takes it; fp32 and fp64; SqExp
and Matern-3/2; npts = 7 with the offset draw fixed.  The windowed line matvec chooses its split from the
device's CU count, so both runs must see the same device."""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRIDS = [(5,), (3, 70), (2, 3, 70)]
NOBS = [3, 257]
ROWS = [1, 3, 9]
NSPLIT = [1, 2]
NPTS = 7
NFEAT = 300            # five 64-feature units: two slices of whole units exist
ELL, SIG2, TOL = 0.15, 1.3, 1e-3
ELLS = [0.15, 0.4, 0.07]   # one per axis: the first len(grid) of them


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import ziggy.kernels as zk
    from hipgp_amd import kuf, rff
    dev = torch.device("cuda", 0)
    res = {}

    def put(key, t):
        assert t is not None and key not in res, key
        res[key] = sha(t)

    def put_grad(key, fwd, ell, G):
        """the (sig2, ell) gradient of fwd((sig2, ell)) for the upstream G: what the hgp_kuf_*_grad entry wrote"""
        s2 = torch.tensor(SIG2, dtype=ell.dtype, device=ell.device, requires_grad=True)
        ell.requires_grad_(True)
        K = fwd((s2, ell))
        assert K is not None and K.requires_grad, key
        K.backward(G)
        put(f"{key} grad", torch.cat([s2.grad.reshape(1), ell.grad.reshape(-1)]))

    for dt in (torch.float32, torch.float64):
        for dims in GRIDS:
            d = len(dims)
            grids = [torch.linspace(-1., 1., m, dtype=dt, device=dev) for m in dims]
            M = 1
            for m in dims:
                M *= m
            for N in NOBS:
                g = torch.Generator(device="cpu").manual_seed(1000 * d + N)
                x = (2.2 * torch.rand(N, d, generator=g, dtype=torch.float64) - 1.1).to(dt).to(dev)
                u = torch.tensor([0.37], dtype=dt, device=dev)
                Wall = torch.randn(max(ROWS), M, generator=g, dtype=torch.float64).to(dt).to(dev)
                Call = torch.randn(max(ROWS), N, generator=g, dtype=torch.float64).to(dt).to(dev)
                om = torch.randn(NFEAT, d, generator=g, dtype=torch.float64).to(dev) * 20.
                ph = torch.rand(NFEAT, generator=g, dtype=torch.float64).to(dev) * 6.28
                Fall = torch.randn(max(ROWS), NFEAT, generator=g, dtype=torch.float64).to(dt).to(dev)
                Gup = torch.randn(N, M, generator=g, dtype=torch.float64).to(dt).to(dev)
                base = f"{'f32' if dt == torch.float32 else 'f64'} grid={dims} N={N}"
                for kname, k in (("sqexp", zk.SqExp(dtype=dt)), ("matern32", zk.Matern(nu=1.5, dtype=dt))):
                    sq = kname == "sqexp"
                    kp = (torch.tensor(SIG2, dtype=dt), torch.tensor(ELL, dtype=dt))
                    b = f"{base} {kname}"
                    put(f"{b} kuf_grid", kuf.kuf_grid(k, grids, x, kp))
                    put(f"{b} kuf_semi_mc", kuf.kuf_semi_mc(k, grids, x, kp, NPTS, u=u))
                    if sq:
                        put(f"{b} kuf_semi_sqexp", kuf.kuf_semi_sqexp(k, grids, x, kp))
                    plan = kuf.WindowPlan(k, grids, x, kp, TOL)
                    lplan = kuf.LineWindowPlan(k, grids, x, kp, TOL)
                    for r in ROWS:
                        W, C = Wall[:r], Call[:r]
                        for ns in NSPLIT:
                            t = f"{b} rows={r} nsplit={ns}"
                            put(f"{t} grid_matvec", kuf.kuf_grid_matvec(k, grids, x, kp, W, nsplit=ns))
                            put(f"{t} grid_rmatvec", kuf.kuf_grid_rmatvec(k, grids, x, kp, C, nsplit=ns))
                            put(f"{t} semi_mc_matvec",
                                kuf.kuf_semi_mc_matvec(k, grids, x, kp, NPTS, u=u, W=W, nsplit=ns))
                            put(f"{t} semi_mc_rmatvec",
                                kuf.kuf_semi_mc_rmatvec(k, grids, x, kp, NPTS, u=u, C=C, nsplit=ns))
                            if sq:
                                put(f"{t} semi_sqexp_matvec",
                                    kuf.kuf_semi_sqexp_matvec(k, grids, x, kp, W, nsplit=ns))
                                put(f"{t} semi_sqexp_rmatvec",
                                    kuf.kuf_semi_sqexp_rmatvec(k, grids, x, kp, C, nsplit=ns))
                        t = f"{b} rows={r}"
                        put(f"{t} grid_matvec_win", kuf.kuf_grid_matvec_win(plan, W))
                        put(f"{t} grid_rmatvec_win", kuf.kuf_grid_rmatvec_win(plan, C))
                        put(f"{t} semi_mc_matvec_win", kuf.kuf_semi_mc_matvec_win(lplan, W, NPTS, u=u))
                        put(f"{t} semi_mc_rmatvec_win", kuf.kuf_semi_mc_rmatvec_win(lplan, C, NPTS, u=u))
                        if sq:
                            put(f"{t} semi_sqexp_matvec_win", kuf.kuf_semi_sqexp_matvec_win(lplan, W))
                            put(f"{t} semi_sqexp_rmatvec_win", kuf.kuf_semi_sqexp_rmatvec_win(lplan, C))
                    ads = [("kuf_grid_ad", lambda p: kuf.kuf_grid_ad(k, grids, x, p)),
                           ("kuf_semi_mc_ad", lambda p: kuf.kuf_semi_mc_ad(k, grids, x, p, NPTS, u=u))]
                    if sq:
                        ads.append(("kuf_semi_sqexp_ad", lambda p: kuf.kuf_semi_sqexp_ad(k, grids, x, p)))
                    for name, fn in ads:
                        put_grad(f"{b} {name}", fn, torch.tensor(ELL, dtype=dt, device=dev), Gup)
                k = zk.SqExp(dtype=dt, ard=True)
                b, ell = f"{base} sqexp ard", ELLS[:d]
                kp = (torch.tensor(SIG2, dtype=dt), ell)
                put(f"{b} kuf_grid", kuf.kuf_grid(k, grids, x, kp))
                put_grad(f"{b} kuf_grid_ad", lambda p: kuf.kuf_grid_ad(k, grids, x, p),
                         torch.tensor(ell, dtype=dt, device=dev), Gup)
                plan = kuf.WindowPlan(k, grids, x, kp, TOL)
                for r in ROWS:
                    for ns in NSPLIT:
                        t = f"{b} rows={r} nsplit={ns}"
                        put(f"{t} grid_matvec", kuf.kuf_grid_matvec(k, grids, x, kp, Wall[:r], nsplit=ns))
                        put(f"{t} grid_rmatvec", kuf.kuf_grid_rmatvec(k, grids, x, kp, Call[:r], nsplit=ns))
                    put(f"{b} rows={r} grid_matvec_win", kuf.kuf_grid_matvec_win(plan, Wall[:r]))
                    put(f"{b} rows={r} grid_rmatvec_win", kuf.kuf_grid_rmatvec_win(plan, Call[:r]))
                for r in ROWS:
                    for ns in NSPLIT:
                        for tr in (False, True):
                            t = f"{base} rows={r} nsplit={ns} transposed={tr}"
                            put(f"{t} rff_matvec x", rff.rff_matvec(om, ph, Fall[:r], x=x, scale=.7, transposed=tr,
                                                                    nsplit=ns))
                            put(f"{t} rff_line_matvec", rff.rff_line_matvec(om, ph, Fall[:r], x, scale=.7,
                                                                            transposed=tr, nsplit=ns))
                            if N == NOBS[0]:
                                put(f"{t} rff_matvec mesh", rff.rff_matvec(om, ph, Fall[:r], xgrids=grids, scale=.7,
                                                                           transposed=tr, nsplit=ns))
    torch.cuda.synchronize()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print(json.dumps({"entries": len(res), "lib": os.environ.get("HGP_LIB", "default"),
                      "digest": hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest()}))


if __name__ == "__main__":
    main()
