"""The windowed Kuf products (hgp_kuf_grid_matvec_win / hgp_kuf_grid_rmatvec_win / hgp_kuf_win_bins behind
`kuf.WindowPlan`, `kuf.kuf_grid_matvec_win`, `kuf.kuf_grid_rmatvec_win`) without a GPU: the truncation
rule `kuf.support_radius` against the fp64 kernel formulas, the ABI and its argument checks (all made
before any HIP call), the tile / bin geometry, the wrappers and the model knobs declining or refusing
where they must, and the register budget of the new kernels."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from test_kernel_resources_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN_SYMS = ("hgp_kuf_grid_matvec_win", "hgp_kuf_grid_rmatvec_win", "hgp_kuf_win_bins")
E_ARG = -1
F32, SQEXP, GNEITING = 0, 0, 4
KERNELS = [("sqexp", None), ("matern", 0.5), ("matern", 1.5), ("matern", 2.5)]
TOLS = (1e-3, 2.0 ** -24, 1e-12)
PARAMS = ((1.0, 0.01), (2.5, 0.3))
kid = lambda k: f"{k[0]}{k[1] or ''}"


def _kern(kind, nu, dtype=torch.float64):
    import hipgp_amd.ziggy.kernels as zk
    if kind == "gneiting":
        return zk.Gneiting(dtype=dtype)
    return zk.SqExp(dtype=dtype) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dtype)


def _k64(kind, nu, r, sig2, ell):
    """k(r) in fp64 by the formulas of the device's kern_eval (hgp_kuf_eval.hpp)."""
    if kind == "sqexp":
        dv = r / ell
        return sig2 * math.exp(-(dv * dv) / 2)
    if nu == 0.5:
        return sig2 * math.exp(-r / ell)
    if nu == 1.5:
        dp = 1.7320508075688772935 * r / ell
        return sig2 * ((1 + dp) * math.exp(-dp))
    dp = 2.2360679774997896964 * r / ell
    return sig2 * ((1 + dp + (5. / 3.) * (r * r) / (ell * ell)) * math.exp(-dp))


@pytest.mark.parametrize("params", PARAMS, ids=lambda p: f"s{p[0]}l{p[1]}")
@pytest.mark.parametrize("tol", TOLS, ids=lambda t: f"{t:.1e}")
@pytest.mark.parametrize("kern", KERNELS, ids=kid)
def test_support_radius_is_the_smallest_distance_under_the_tolerance(kern, tol, params):
    from hipgp_amd import kuf
    sig2, ell = params
    rho = kuf.support_radius(_kern(*kern), params, tol)
    assert isinstance(rho, float) and rho > 0
    at, inside = _k64(*kern, rho, sig2, ell), _k64(*kern, 0.999 * rho, sig2, ell)
    print(f"{kid(kern)} tol={tol:.3e} sig2={sig2} ell={ell}: rho = {rho:.17g} = {rho / ell:.4f} ell, "
          f"k(rho)/sig2 = {at / sig2:.6e}, k(0.999 rho)/sig2 = {inside / sig2:.6e}")
    assert at <= tol * sig2
    assert inside > tol * sig2
    if kern[0] == "sqexp":
        closed = ell * math.sqrt(2 * math.log(1 / tol))
        assert abs(rho - closed) <= 1e-15 * closed
    # tensors for the parameters are read as their values
    assert kuf.support_radius(_kern(*kern), (torch.tensor(sig2), torch.tensor([ell], dtype=torch.float64)), tol) == rho


def test_support_radius_declines_what_the_fused_kernels_decline():
    from hipgp_amd import kuf
    k = _kern("sqexp", None)
    assert kuf.support_radius(_kern("gneiting", None), (1.0, 0.3), 1e-6) is None
    assert kuf.support_radius(k, (1.0, torch.tensor([0.2, 0.3])), 1e-6) is None
    assert kuf.support_radius(_kern("matern", 1.5), (1.0, torch.tensor([0.2, 0.3])), 1e-6) is None
    for bad in (0.0, 1.0, -1e-3, 1.5, float("nan"), None):
        assert kuf.support_radius(k, (1.0, 0.3), bad) is None, bad
        assert kuf.support_radius(_kern("matern", 2.5), (1.0, 0.3), bad) is None, bad
    assert kuf.support_radius(object(), (1.0, 0.3), 1e-6) is None


def test_header_declares_and_library_exports_the_window_entries():
    from hipgp_amd import _lib
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    L = _lib.lib()
    for s in WIN_SYMS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", src), f"include/hipgp.h does not declare {s}"
        assert hasattr(L, s), f"libhipgp.so does not export {s}"
        assert s in _lib.EXPORTS
        assert getattr(L, s).argtypes is not None, f"{s} is not bound"


class _Args:
    """A well-formed argument set (host addresses standing in for device ones: every call below
    must return before anything is launched), with one field replaced per case."""

    def __init__(self):
        self.buf = (ctypes.c_float * 64)()
        self.idx = (ctypes.c_int64 * 64)()
        p = ctypes.cast(self.buf, ctypes.c_void_p)
        q = ctypes.cast(self.idx, ctypes.c_void_p)
        self.m = (ctypes.c_int64 * 2)(4, 4)
        self.grids = (ctypes.c_void_p * 2)(p.value, p.value)
        self.kw = dict(dtype=F32, kind=SQEXP, ndim=2, x=p, nobs=2, rho=0.5, w=p, nw=2, out=p, m=self.m,
                       grids=self.grids, order=q, bin_start=q)

    def call(self, L, name, **over):
        a = dict(self.kw, **over)
        if name == "hgp_kuf_grid_matvec_win":
            return L.hgp_kuf_grid_matvec_win(a["dtype"], a["kind"], a["ndim"], a["m"], a["grids"], a["x"], a["nobs"],
                                             1.0, 0.5, a["rho"], a["w"], a["nw"], a["out"], None)
        return L.hgp_kuf_grid_rmatvec_win(a["dtype"], a["kind"], a["ndim"], a["m"], a["grids"], a["x"], a["nobs"],
                                          1.0, 0.5, a["rho"], a["w"], a["nw"], a["order"], a["bin_start"], a["out"],
                                          None)


BAD = [("null_x", dict(x=None)), ("null_w", dict(w=None)), ("null_out", dict(out=None)), ("null_m", dict(m=None)),
       ("null_grids", dict(grids=None)), ("bad_dtype", dict(dtype=7)), ("bad_kind", dict(kind=9)),
       ("negative_kind", dict(kind=-1)), ("gneiting", dict(kind=GNEITING)), ("ndim0", dict(ndim=0)),
       ("ndim4", dict(ndim=4)), ("negative_nobs", dict(nobs=-1)), ("negative_nw", dict(nw=-1)),
       ("negative_rho", dict(rho=-1e-3)), ("nan_rho", dict(rho=float("nan"))), ("inf_rho", dict(rho=float("inf"))),
       ("grid_size0", dict(m=(ctypes.c_int64 * 2)(4, 0))),
       ("null_grid", dict(grids=(ctypes.c_void_p * 2)(None, None))),
       ("null_order", dict(order=None)), ("null_bin_start", dict(bin_start=None))]
BAD_CALLS = [(n, t, o) for n in WIN_SYMS[:2] for t, o in BAD
             if not (t in ("null_order", "null_bin_start") and n == "hgp_kuf_grid_matvec_win")]


@pytest.mark.parametrize("name,tag,over", BAD_CALLS, ids=[f"{c[0]}-{c[1]}" for c in BAD_CALLS])
def test_window_entries_refuse_bad_arguments_before_any_hip_call(name, tag, over):
    from hipgp_amd import _lib
    L = _lib.lib()
    a = _Args()
    for i in range(64):
        a.buf[i] = 3.0
    rc = a.call(L, name, **over)
    assert rc == E_ARG, (name, tag, rc)
    assert len(L.hgp_last_error()) > 0
    assert all(v == 3.0 for v in a.buf)


@pytest.mark.parametrize("name,over", [("hgp_kuf_grid_matvec_win", dict(nobs=0)), ("hgp_kuf_grid_matvec_win", dict(nw=0)),
                                       ("hgp_kuf_grid_matvec_win", dict(nobs=0, x=None, out=None)),
                                       ("hgp_kuf_grid_matvec_win", dict(nw=0, w=None)),
                                       ("hgp_kuf_grid_rmatvec_win", dict(nw=0)),
                                       ("hgp_kuf_grid_rmatvec_win", dict(nw=0, w=None, out=None, order=None))],
                         ids=["mv_nobs0", "mv_nw0", "mv_nobs0_null", "mv_nw0_null", "rmv_nc0", "rmv_nc0_null"])
def test_empty_window_products_return_zero_before_any_launch(name, over):
    from hipgp_amd import _lib
    a = _Args()
    for i in range(64):
        a.buf[i] = 3.0
    assert a.call(_lib.lib(), name, **over) == 0
    assert all(v == 3.0 for v in a.buf), "an empty product wrote something"


@pytest.mark.parametrize("ndim", [1, 2, 3])
@pytest.mark.parametrize("m", [1, 7, 64, 65, 1024])
def test_win_bins_cover_the_grid(m, ndim):
    """Every cell 0 .. m (the number of nodes <= x) has a bin, tiles cover the nodes, and the Python
    wrapper reports what the C entry reports."""
    from hipgp_amd import _lib, kuf
    dims = [m, 5, 9][:ndim]
    tile, nbins = kuf.win_bins(dims)
    assert len(tile) == ndim and len(nbins) == ndim
    threads = 1
    for a in range(ndim):
        assert tile[a] >= 1 and nbins[a] >= 1
        assert nbins[a] == dims[a] // tile[a] + 1
        assert (nbins[a] - 1) * tile[a] <= dims[a] < nbins[a] * tile[a], "the bins do not cover the cells 0 .. m"
        assert -(-dims[a] // tile[a]) * tile[a] >= dims[a]
        threads *= tile[a]
    assert threads == 256, "a tile is one block of 256 mesh points"
    # m on every axis position
    for perm in ([m] + [3] * (ndim - 1), [3] * (ndim - 1) + [m]):
        t2, n2 = kuf.win_bins(perm)
        assert t2 == tile and n2 == [v // t + 1 for v, t in zip(perm, t2)]
    L = _lib.lib()
    t3, n3 = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    mm = (ctypes.c_int64 * ndim)(*dims)
    assert L.hgp_kuf_win_bins(ndim, mm, t3, n3) == 0
    assert list(t3)[:ndim] == tile and list(n3)[:ndim] == nbins
    assert list(t3)[ndim:] == [1] * (3 - ndim) and list(n3)[ndim:] == [1] * (3 - ndim)


def test_win_bins_refuses_bad_arguments():
    from hipgp_amd import _lib
    L = _lib.lib()
    t, n = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    m = (ctypes.c_int64 * 2)(4, 4)
    assert L.hgp_kuf_win_bins(0, m, t, n) == E_ARG
    assert L.hgp_kuf_win_bins(4, m, t, n) == E_ARG
    assert L.hgp_kuf_win_bins(2, None, t, n) == E_ARG
    assert L.hgp_kuf_win_bins(2, m, None, n) == E_ARG
    assert L.hgp_kuf_win_bins(2, m, t, None) == E_ARG
    assert L.hgp_kuf_win_bins(2, (ctypes.c_int64 * 2)(4, 0), t, n) == E_ARG


def test_window_plan_declines_cpu_tensors_and_unsupported_kernels():
    from hipgp_amd import kuf
    k = _kern("sqexp", None, torch.float32)
    grids = [torch.linspace(-1, 1, 8)] * 2
    x = torch.full((3, 2), 0.4)
    assert kuf.WindowPlan.make(k, grids, x, (1.0, 0.3), 1e-6) is None            # a CPU tensor
    with pytest.raises(ValueError, match="windowed Kuf products do not apply"):
        kuf.WindowPlan(k, grids, x, (1.0, 0.3), 1e-6)
    assert list(inspect.signature(kuf.WindowPlan.__init__).parameters)[:6] == ["self", "kernel", "xgrids", "x",
                                                                               "params", "tol"]
    assert list(inspect.signature(kuf.kuf_grid_matvec_win).parameters) == ["plan", "W"]
    assert list(inspect.signature(kuf.kuf_grid_rmatvec_win).parameters) == ["plan", "C"]
    assert list(inspect.signature(kuf.support_radius).parameters) == ["kernel", "params", "tol"]


def test_model_knobs_default_off_and_refuse_line_integrals(monkeypatch):
    import hipgp_amd.ziggy.hipgp as hg
    from test_kuf_matvec_cpu import SolvingKmm, _model, _oracle, _points
    monkeypatch.delenv("HGP_KUF_SUPPORT_TOL", raising=False)
    mod = _model()
    assert mod.kuf_support_tol is None and mod._kuf_support_tol() is None and mod._win is None
    assert inspect.signature(hg.ToeplitzInducingGP.predict_samples).parameters["support_tol"].default is None
    assert mod._kuf_support_tol(1e-6) == 1e-6
    monkeypatch.setenv("HGP_KUF_SUPPORT_TOL", "1e-5")
    assert mod._kuf_support_tol() == 1e-5
    mod.kuf_support_tol = 1e-7                    # the attribute goes before the environment
    assert mod._kuf_support_tol() == 1e-7
    assert mod._kuf_support_tol(1e-3) == 1e-3     # and the argument before both
    for bad in (0.0, 1.0, -1.0):
        with pytest.raises(ValueError, match="support tolerance"):
            mod._kuf_support_tol(bad)
    monkeypatch.delenv("HGP_KUF_SUPPORT_TOL")
    Kmm = SolvingKmm(_oracle())
    x = _points()
    y = torch.zeros(x.shape[0], 1, dtype=torch.float64)
    for call in (lambda: mod.predict_mean(x, integrated_obs=True, Kmm=Kmm),
                 lambda: mod.predict_draws(x, 2, integrated_obs=True, Kmm=Kmm),
                 lambda: mod.fit_mean(x, y, integrated_obs=True, Kmm=Kmm)):
        with pytest.raises(NotImplementedError, match="tube"):
            call()
    assert mod._win is None
    # point observations on the CPU: the plan declines, the dense route answers as with the knob unset
    mu_t = mod.predict_mean(x, Kmm=Kmm)
    mod.kuf_support_tol = None
    assert torch.equal(mu_t, mod.predict_mean(x, Kmm=Kmm))


def test_window_kernels_do_not_spill():
    ks = [k for k in _kernels() if re.search(r"hgp::k_kuf_win_\w+<", k[0])]
    mv = [k for k in ks if "k_kuf_win_mv<" in k[0]]
    rmv = [k for k in ks if "k_kuf_win_rmv<" in k[0]]
    assert len(mv) == 2 * 4 * 3 and len(rmv) == 2 * 4 * 3 * 3, (len(mv), len(rmv))
    bad = [f"{n} (spill {s}, scratch {p}, vgpr {v})" for n, s, p, v in ks if s or p]
    assert not bad, "windowed Kuf product kernels spilling to scratch:\n" + "\n".join(bad)
