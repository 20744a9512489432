"""The transposed fused Kuf products (hgp_kuf_grid_rmatvec / hgp_kuf_semi_mc_rmatvec /
hgp_kuf_semi_sqexp_rmatvec) and `ToeplitzInducingGP.fit_mean` on top of them without a GPU: the ABI and
its argument checks (all made before any HIP call), the wrappers declining CPU tensors, the register
budget of the new fp32 kernels, and the host logic of `fit_mean` on a stand-in Kmm made of the fp64
oracle's operators, where both products take the chunked fallback, against the dense `batch_solve`
formula (I + sum iv kn kn^T)^-1 sum iv y kn."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from grid_posterior_cases import OracleKmm, dense_R, max_rel
from test_kernel_resources_cpu import _kernels
from test_kuf_matvec_cpu import _model, _oracle, _points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RMV_SYMS = ("hgp_kuf_grid_rmatvec", "hgp_kuf_semi_mc_rmatvec", "hgp_kuf_semi_sqexp_rmatvec")
E_ARG = -1
F32, SQEXP, GNEITING = 0, 0, 4
NOBS = 40


def test_header_declares_and_library_exports_the_rmatvec_entries():
    from hipgp_amd import _lib
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    L = _lib.lib()
    for s in RMV_SYMS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", src), f"include/hipgp.h does not declare {s}"
        assert hasattr(L, s), f"libhipgp.so does not export {s}"
        assert s in _lib.EXPORTS


class _Args:
    """A well-formed argument set (host addresses standing in for device ones: every call below
    must return before anything is launched), with one field replaced per case."""

    def __init__(self):
        self.buf = (ctypes.c_float * 64)()
        p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.m = (ctypes.c_int64 * 2)(4, 4)
        self.grids = (ctypes.c_void_p * 2)(p.value, p.value)
        self.kw = dict(dtype=F32, kind=SQEXP, ndim=2, x=p, nobs=2, npts=3, u=p, c=p, nc=2, nsplit=0, out=p,
                       m=self.m, grids=self.grids)

    def call(self, L, name, **over):
        a = dict(self.kw, **over)
        if name == "hgp_kuf_grid_rmatvec":
            return L.hgp_kuf_grid_rmatvec(a["dtype"], a["kind"], a["ndim"], a["m"], a["grids"], a["x"], a["nobs"],
                                          1.0, 0.5, a["c"], a["nc"], a["nsplit"], a["out"], None)
        if name == "hgp_kuf_semi_mc_rmatvec":
            return L.hgp_kuf_semi_mc_rmatvec(a["dtype"], a["kind"], 1.0, a["ndim"], a["m"], a["grids"], a["x"],
                                             a["nobs"], 1.0, 0.5, a["npts"], a["u"], a["c"], a["nc"], a["nsplit"],
                                             a["out"], None)
        return L.hgp_kuf_semi_sqexp_rmatvec(a["dtype"], a["ndim"], a["m"], a["grids"], a["x"], a["nobs"], 1.0, 0.5,
                                            a["c"], a["nc"], a["nsplit"], a["out"], None)


BAD = [("null_x", dict(x=None)), ("null_c", dict(c=None)), ("null_out", dict(out=None)), ("null_m", dict(m=None)),
       ("null_grids", dict(grids=None)), ("null_u", dict(u=None)), ("bad_dtype", dict(dtype=7)),
       ("bad_kind", dict(kind=9)), ("negative_kind", dict(kind=-1)), ("ndim0", dict(ndim=0)), ("ndim4", dict(ndim=4)),
       ("negative_nobs", dict(nobs=-1)), ("negative_nc", dict(nc=-1)), ("negative_nsplit", dict(nsplit=-1)),
       ("grid_size0", dict(m=(ctypes.c_int64 * 2)(4, 0))), ("nobs0_null_out", dict(nobs=0, out=None)),
       ("npts0", dict(npts=0)), ("npts1025", dict(npts=1025))]

# (the semi-sqexp entry has no kind; only the semi-mc entry has npts and u)
BAD_CALLS = [(n, t, o) for n in RMV_SYMS for t, o in BAD
             if not (t in ("bad_kind", "negative_kind") and n == "hgp_kuf_semi_sqexp_rmatvec")
             and not (t in ("npts0", "npts1025", "null_u") and n != "hgp_kuf_semi_mc_rmatvec")]


@pytest.mark.parametrize("name,tag,over", BAD_CALLS, ids=[f"{c[0]}-{c[1]}" for c in BAD_CALLS])
def test_rmatvec_entries_refuse_bad_arguments(name, tag, over):
    from hipgp_amd import _lib
    L = _lib.lib()
    rc = _Args().call(L, name, **over)
    assert rc == E_ARG, (name, tag, rc)
    assert len(L.hgp_last_error()) > 0


@pytest.mark.parametrize("name", RMV_SYMS)
@pytest.mark.parametrize("over", [dict(nc=0), dict(nc=0, c=None, out=None), dict(nc=0, nobs=0, x=None)],
                         ids=["nc0", "nc0_null", "nc0_nobs0"])
def test_no_coefficient_rows_write_nothing_before_any_launch(name, over):
    from hipgp_amd import _lib
    a = _Args()
    for i in range(64):
        a.buf[i] = 3.0
    assert a.call(_lib.lib(), name, **over) == 0
    assert all(v == 3.0 for v in a.buf), "a product of no rows wrote something"


def test_grid_rmatvec_refuses_gneiting_as_the_forward_does():
    """Gneiting is a semi-mc kernel only: the point product answers it exactly as hgp_kuf_grid."""
    from hipgp_amd import _lib
    L = _lib.lib()
    a = _Args()
    p = a.kw["x"]
    fwd = L.hgp_kuf_grid(F32, GNEITING, 2, a.m, a.grids, p, 2, 1.0, 0.5, p, None)
    assert fwd == E_ARG
    assert a.call(L, "hgp_kuf_grid_rmatvec", kind=GNEITING) == fwd
    assert b"kind" in L.hgp_last_error()


def test_wrappers_decline_cpu_tensors_and_unsupported_kernels():
    import hipgp_amd.ziggy.hipgp as hg
    import hipgp_amd.ziggy.kernels as zk
    from hipgp_amd import kuf
    k = zk.SqExp(dtype=torch.float32)
    grids = [torch.linspace(-1, 1, 8)] * 2
    x = torch.full((3, 2), 0.4)
    C = torch.ones(2, 3)
    assert kuf.kuf_grid_rmatvec(k, grids, x, (1.0, 0.3), C) is None
    assert kuf.kuf_semi_mc_rmatvec(k, grids, x, (1.0, 0.3), 4, C=C) is None
    assert kuf.kuf_semi_sqexp_rmatvec(k, grids, x, (1.0, 0.3), C) is None
    assert kuf.kuf_semi_sqexp_rmatvec(zk.Matern(nu=1.5, dtype=torch.float32), grids, x, (1.0, 0.3), C) is None
    assert kuf.kuf_grid_rmatvec(zk.Gneiting(dtype=torch.float32), grids, x, (1.0, 0.3), C) is None
    par = lambda f: inspect.signature(f).parameters
    assert list(par(kuf.kuf_grid_rmatvec)) == ["kernel", "xgrids", "x", "params", "C", "nsplit"]
    assert list(par(kuf.kuf_semi_mc_rmatvec)) == ["kernel", "xgrids", "x", "params", "npts", "u", "C", "nsplit"]
    assert list(par(kuf.kuf_semi_sqexp_rmatvec)) == ["kernel", "xgrids", "x", "params", "C", "nsplit"]
    for f in (kuf.kuf_grid_rmatvec, kuf.kuf_semi_mc_rmatvec, kuf.kuf_semi_sqexp_rmatvec):
        assert par(f)["nsplit"].default == 0
    assert par(kuf.kuf_semi_mc_rmatvec)["u"].default is None and par(kuf.kuf_semi_mc_rmatvec)["C"].default is None
    T = hg.ToeplitzInducingGP
    sig = par(T.fit_mean)
    assert list(sig) == ["self", "xobs", "yobs", "noise_std", "integrated_obs", "semi_integrated_estimator",
                         "semi_integrated_samps", "maxiter", "tol", "Kmm", "mc_offset", "batch_size", "update",
                         "callback"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, False, "analytic", 10, 1000, 1e-6, None, None, None,
                                                       True, None]
    assert list(par(T._kuf_rproduct)) == ["self", "x", "C", "integrated_obs", "estimator", "samps", "mc_offset",
                                          "batch_size"]
    assert hg.MeanFit._fields == ("weights", "qm", "iters", "relres")
    for cls in (hg.MeanFieldToeplitzGP, hg.BlockToeplitzGP):
        assert cls.fit_mean is T.fit_mean


def test_new_fp32_rmatvec_kernels_do_not_spill():
    ks = [k for k in _kernels() if re.search(r"hgp::k_kuf_\w*rmv\w*<float", k[0])]
    point = [k for k in ks if "k_kuf_grid_rmv<float" in k[0]]
    semi = [k for k in ks if "k_kuf_semi_rmv<float" in k[0]]
    assert len(point) >= 4 and len(semi) >= 2 and any("k_kuf_rmv_finish<float" in k[0] for k in ks), [k[0] for k in ks]
    bad = [f"{n} (spill {s}, scratch {p}, vgpr {v})" for n, s, p, v in ks if s or p]
    assert not bad, "fp32 transposed Kuf product kernels spilling to scratch:\n" + "\n".join(bad)


# ---- host logic on the oracle stand-in ---------------------------------------------------------
class FitKmm(OracleKmm):
    """`OracleKmm` with the operators `fit_mean` calls (K, C^-1, R^T from the fp64 oracle) and the dense K
    for the reference.  It has no solve: a method that tried one would fail."""

    def __init__(self, O):
        super().__init__(O)
        self.K = O.matmul_K(np.eye(O.M, dtype=O.dtype)).T.copy()

    def _matmul_by_K(self, v):
        self.calls.append(("K", tuple(v.shape)))
        return torch.from_numpy(self.O.matmul_K(v.detach().numpy()))

    def _matmul_by_Cinv(self, v):
        self.calls.append(("Cinv", tuple(v.shape)))
        return torch.from_numpy(self.O.matmul_Cinv(v.detach().numpy()))

    def _matmul_by_RT(self, v):
        self.calls.append(("RT", tuple(v.shape)))
        return torch.from_numpy(self.O.matmul_RT(v.detach().numpy()))


def _data(per_obs_noise):
    g = torch.Generator().manual_seed(31)
    x = torch.rand(NOBS, 2, generator=g, dtype=torch.float64) * 2.4 - 1.2      # some outside the grid's hull
    y = torch.randn(NOBS, 1, generator=g, dtype=torch.float64)
    sd = (torch.rand(NOBS, 1, generator=g, dtype=torch.float64) * .4 + .1) if per_obs_noise else None
    return x, y, sd


def _dense_mstar(mod, Kmm, x, y, sd):
    """(m*, Knm, beta*) of the dense `batch_solve` formula with kn = R^T K^-1 Knm^T from dense algebra."""
    R = dense_R(Kmm.O)
    Knm = mod.kernel(x, mod.xinduce, mod.get_kernel_params()).detach().numpy()
    kn = (R.T @ np.linalg.solve(Kmm.K, Knm.T)).T
    iv = (1 / sd.numpy().reshape(-1) ** 2) if sd is not None else np.full(NOBS, float(torch.exp(-mod.log_noise2)))
    yv = y.numpy().reshape(-1)
    mstar = np.linalg.solve(np.eye(kn.shape[1]) + (iv[:, None] * kn).T @ kn, kn.T @ (iv * yv))
    return mstar, Knm


def _params(mod):
    return {k: v.detach().clone() for k, v in mod.named_parameters()}


@pytest.mark.parametrize("batch_size", [None, 7], ids=["one_piece", "pieces_with_tail"])
@pytest.mark.parametrize("per_obs_noise", [True, False], ids=["noise_per_obs", "noise_shared"])
@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_fit_mean_matches_the_dense_batch_solve_formula(family, per_obs_noise, batch_size):
    mod, Kmm = _model(family), FitKmm(_oracle())
    x, y, sd = _data(per_obs_noise)
    mstar, Knm = _dense_mstar(mod, Kmm, x, y, sd)
    before = _params(mod)
    seen = []
    fit = mod.fit_mean(x, y, noise_std=sd, tol=1e-10, Kmm=Kmm, batch_size=batch_size, update=False,
                       callback=lambda it, rr: seen.append((it, rr)))
    gap = max_rel(fit.qm.numpy().reshape(-1), mstar)
    print(f"fit_mean vs dense m*: {family} per_obs={per_obs_noise} batch={batch_size} gap {gap:.2e} "
          f"iters {fit.iters} relres {fit.relres:.2e}")
    assert gap < 1e-7
    assert tuple(fit.weights.shape) == (1, Kmm.O.M) and tuple(fit.qm.shape) == (Kmm.O.Mp, 1)
    assert not fit.weights.requires_grad and not fit.qm.requires_grad
    assert fit.relres < 1e-10 and 0 < fit.iters < 1000
    assert [s[0] for s in seen] == list(range(1, fit.iters + 1)) and seen[-1][1] == fit.relres
    # one K and one C^-1 per iteration (no C^-1 after the last), one R^T at the end, nothing else
    kinds = [c[0] for c in Kmm.calls]
    assert kinds.count("K") == fit.iters and kinds.count("Cinv") == fit.iters and kinds.count("RT") == 1
    assert set(kinds) == {"K", "Cinv", "RT"}
    # update=False: every parameter bit-identical
    after = _params(mod)
    assert all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("parameterization", ["expectation-family", "standard"])
@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_fit_mean_update_writes_the_mean_and_leaves_the_covariance(family, parameterization):
    import hipgp_amd.ziggy.hipgp as hg
    import hipgp_amd.ziggy.kernels as zk
    if parameterization == "standard":
        dt = torch.float64
        grids = [torch.linspace(-1, 1, m, dtype=dt) for m in (8, 6)]
        kw = dict(num_obs=NOBS, sig2_init=1., ell_init=.3, noise2_init=.05, learn_kernel=False, dtype=dt,
                  parameterization="standard")
        torch.manual_seed(5)
        mod = (hg.BlockToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, block_sizes=[2, 2], **kw) if family == "block"
               else hg.MeanFieldToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, **kw))
        cov = "global_S"
    else:
        mod, cov = _model(family), "global_theta2"
    Kmm = FitKmm(_oracle())
    x, y, sd = _data(True)
    before = _params(mod)
    fit = mod.fit_mean(x, y, noise_std=sd, tol=1e-10, Kmm=Kmm)
    after = _params(mod)
    assert torch.equal(before[cov], after[cov]), "fit_mean changed the variational covariance"
    for k in ("log_ell", "log_sig2", "log_noise2"):
        assert torch.equal(before[k], after[k])
    qm_now, qS_now = mod.standard_variational_params()
    assert max_rel(qm_now.detach().numpy(), fit.qm.numpy()) < 1e-11
    if parameterization == "standard":
        assert torch.equal(mod.global_m.data, fit.qm)
    mstar, _ = _dense_mstar(mod, Kmm, x, y, sd)
    assert max_rel(qm_now.detach().numpy().reshape(-1), mstar) < 1e-7


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_predict_mean_takes_the_fitted_weights_without_a_solve(family):
    mod, Kmm = _model(family), FitKmm(_oracle())
    x, y, sd = _data(False)
    fit = mod.fit_mean(x, y, tol=1e-10, Kmm=Kmm)
    xt = _points()
    Knm_t = mod.kernel(xt, mod.xinduce, mod.get_kernel_params()).detach().numpy()
    ncalls = len(Kmm.calls)
    mu = mod.predict_mean(xt, weights=fit.weights, Kmm=Kmm)
    assert len(Kmm.calls) == ncalls, "predict_mean called an operator although weights were given"
    assert max_rel(mu.numpy()[:, 0], Knm_t @ fit.weights.numpy()[0]) < 1e-12
    # beta is K^-1 R qm: the weights `mean_weights` would solve for
    R = dense_R(Kmm.O)
    alpha = np.linalg.solve(Kmm.K, R @ fit.qm.numpy().reshape(-1))
    assert max_rel(fit.weights.numpy()[0], alpha) < 1e-7


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_fit_mean_refuses_cholesky_whitening(family):
    mod = _model(family, whitened_type="cholesky")
    Kmm = FitKmm(_oracle())
    x, y, sd = _data(True)
    with pytest.raises(NotImplementedError, match="fit_mean need whitened_type='ziggy'"):
        mod.fit_mean(x, y, noise_std=sd, Kmm=Kmm)
    with pytest.raises(NotImplementedError, match="cholesky whitening has no circulant R"):
        mod.fit_mean(x, y, Kmm=Kmm)
    assert Kmm.calls == []
