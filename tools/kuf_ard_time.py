"""The point-observation Kuf entries with one length scale per axis (hgp_kuf_grid*_ard) against the scalar
entries of this tree and of a library built from the parent commit, in the same session on one GPU box:
C2 (1024^2 on [-1, 1]^2, SqExp(1, 0.01)), fp32, points uniform in the grid's box.

    make -C hipgp_amd/csrc VARIANT=parent      # in a checkout of the parent commit -> libhipgp_parent.so
    timeout -k 10 900 python tools/kuf_ard_time.py --parent-lib PATH/libhipgp_parent.so > profiles/kuf_ard_time.jsonl

One JSON line per (entry, N, rows, variant).  The variants of a measurement ALTERNATE inside every
repetition (parent scalar, tree scalar, tree _ard with ell replicated, tree _ard with ell = (0.01, 0.02)),
each call between two device events after one warm call of each; every repetition is listed (`runs_ms`,
in order) next to the median (`ms`); nothing is dropped.
  dense products   hgp_kuf_grid_matvec / _rmatvec, N = 10^4 and 10^6, 1 and 8 rows
  windowed pair    hgp_kuf_grid_matvec_win / _rmatvec_win at t = 2^-24, the same N and rows
  backward         hgp_kuf_grid_grad, N = 200 (the upstream gradient is (N, M) fp32: 0.8 GB)
Without --parent-lib the parent variant is left out."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOL = 2.0 ** -24
SIG2, ELL, ELL_ARD = 1.0, 0.01, (0.01, 0.02)
DIMS = (1024, 1024)


def bind(path):
    """the scalar entries of another build of the library, with the tree's own signatures"""
    from hipgp_amd import _lib
    tree = _lib.lib()
    L = ctypes.CDLL(path)
    for name in ("hgp_kuf_grid_matvec", "hgp_kuf_grid_rmatvec", "hgp_kuf_grid_matvec_win", "hgp_kuf_grid_rmatvec_win",
                 "hgp_kuf_grid_grad", "hgp_last_error"):
        fn, ref = getattr(L, name), getattr(tree, name)
        fn.restype, fn.argtypes = ref.restype, ref.argtypes
    return L


def alternate(fns, reps):
    """{variant: [ms, ...]}: one warm call of each, then reps rounds that run every variant once, in order"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 4, 10 ** 6])
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--grad-n", type=int, default=200)
    a = ap.parse_args()
    from hipgp_amd import _lib, kuf
    import ziggy.kernels as zk
    dev = torch.device("cuda", 0)
    dt = torch.float32
    tree = _lib.lib()
    parent = bind(a.parent_lib) if a.parent_lib else None
    k = zk.SqExp(dtype=dt, ard=True)
    grids = [torch.linspace(-1, 1, m, dtype=dt, device=dev) for m in DIMS]
    M = DIMS[0] * DIMS[1]
    m, ptrs = kuf._grid_ptrs(grids)
    code, st = _lib.dtype_code(dt), _lib.stream_ptr(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    g = torch.Generator(device="cpu").manual_seed(42)
    rep2, ard2 = kuf._dvec([ELL, ELL]), kuf._dvec(list(ELL_ARD))
    rho = kuf.support_radius(k, (SIG2, ELL), TOL)
    rho_ard = kuf.support_radius(k, (SIG2, list(ELL_ARD)), TOL)
    rrep2, rard2 = kuf._dvec([rho, rho]), kuf._dvec(rho_ard)
    base = {"config": "C2", "dims": list(DIMS), "dtype": "fp32", "tol": TOL, "ell": ELL, "ell_ard": list(ELL_ARD),
            "rho": rho, "rho_ard": rho_ard, "device": torch.cuda.get_device_name(0)}

    def emit(entry, N, rows, runs):
        for variant, ts in runs.items():
            print(json.dumps(dict(base, entry=entry, N=N, rows=rows, variant=variant, ms=float(np.median(ts)),
                                  runs_ms=[round(t, 4) for t in ts])), flush=True)

    def variants(scalar, ard):
        """scalar(L) and ard(ell, rho) -> the four calls of one measurement, checked"""
        fns = {}
        if parent is not None:
            fns["parent_scalar"] = lambda: _lib.check(scalar(parent))
        fns["tree_scalar"] = lambda: _lib.check(scalar(tree))
        fns["tree_ard_replicated"] = lambda: _lib.check(ard(rep2, rrep2))
        fns["tree_ard_0.01_0.02"] = lambda: _lib.check(ard(ard2, rard2))
        return fns

    for N in a.sizes:
        x = (torch.rand(N, 2, generator=g, dtype=dt) * 2 - 1).to(dev).contiguous()
        order, start = kuf.WindowPlan(k, grids, x, (SIG2, ELL), TOL).bins()
        head = (code, _lib.KERN_SQEXP, 2, m, ptrs, vp(x), N, SIG2)
        reps = a.reps if N <= 10 ** 5 else max(3, a.reps // 2)
        for nr in a.rows:
            W = torch.randn(nr, M, generator=g, dtype=dt).to(dev).contiguous()
            C = torch.randn(nr, N, generator=g, dtype=dt).to(dev).contiguous()
            omv = torch.empty(N, nr, dtype=dt, device=dev)
            ormv = torch.empty(nr, M, dtype=dt, device=dev)
            emit("matvec", N, nr, alternate(variants(
                lambda L: L.hgp_kuf_grid_matvec(*head, ELL, vp(W), nr, 0, vp(omv), st),
                lambda e, r: tree.hgp_kuf_grid_matvec_ard(*head, e, vp(W), nr, 0, vp(omv), st)), reps))
            emit("rmatvec", N, nr, alternate(variants(
                lambda L: L.hgp_kuf_grid_rmatvec(*head, ELL, vp(C), nr, 0, vp(ormv), st),
                lambda e, r: tree.hgp_kuf_grid_rmatvec_ard(*head, e, vp(C), nr, 0, vp(ormv), st)), reps))
            emit("matvec_win", N, nr, alternate(variants(
                lambda L: L.hgp_kuf_grid_matvec_win(*head, ELL, rho, vp(W), nr, vp(omv), st),
                lambda e, r: tree.hgp_kuf_grid_matvec_win_ard(*head, e, r, vp(W), nr, vp(omv), st)), a.reps))
            emit("rmatvec_win", N, nr, alternate(variants(
                lambda L: L.hgp_kuf_grid_rmatvec_win(*head, ELL, rho, vp(C), nr, vp(order), vp(start), vp(ormv), st),
                lambda e, r: tree.hgp_kuf_grid_rmatvec_win_ard(*head, e, r, vp(C), nr, vp(order), vp(start), vp(ormv),
                                                               st)), a.reps))
            del W, C, omv, ormv
    N = a.grad_n
    x = (torch.rand(N, 2, generator=g, dtype=dt) * 2 - 1).to(dev).contiguous()
    G = torch.randn(N, M, generator=g, dtype=dt).to(dev).contiguous()
    grad = torch.empty(4, dtype=dt, device=dev)
    head = (code, _lib.KERN_SQEXP, 2, m, ptrs, vp(x), N, SIG2)
    emit("grad", N, 1, alternate(variants(
        lambda L: L.hgp_kuf_grid_grad(*head, ELL, vp(G), vp(grad), st),
        lambda e, r: tree.hgp_kuf_grid_grad_ard(*head, e, vp(G), vp(grad), st)), a.reps))


if __name__ == "__main__":
    main()
