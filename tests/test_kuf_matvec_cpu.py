"""The fused Kuf products (hgp_kuf_grid_matvec / hgp_kuf_semi_mc_matvec / hgp_kuf_semi_sqexp_matvec) and
the model methods on top of them (mean_weights / predict_mean / predict_draws) without a GPU: the ABI
and its argument checks (all made before any HIP call), the wrappers declining CPU tensors, the
register budget of the new fp32 kernels, and the host logic of the model methods on a stand-in Kmm
made of the fp64 oracle's operators with a dense solve, where the product takes the chunked
fallback, against dense Knm @ solve(K, R v)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from grid_posterior_cases import OracleKmm, dense_R, max_rel
from oracle import ziggy_oracle as zo
from test_kernel_resources_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MV_SYMS = ("hgp_kuf_grid_matvec", "hgp_kuf_semi_mc_matvec", "hgp_kuf_semi_sqexp_matvec")
E_ARG = -1
F32, SQEXP, GNEITING = 0, 0, 4
DIMS = (8, 6)


def test_header_declares_and_library_exports_the_matvec_entries():
    from hipgp_amd import _lib
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    L = _lib.lib()
    for s in MV_SYMS:
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
        self.kw = dict(dtype=F32, kind=SQEXP, ndim=2, x=p, nobs=2, npts=3, u=p, w=p, nw=2, nsplit=0, out=p,
                       m=self.m, grids=self.grids)

    def call(self, L, name, **over):
        a = dict(self.kw, **over)
        if name == "hgp_kuf_grid_matvec":
            return L.hgp_kuf_grid_matvec(a["dtype"], a["kind"], a["ndim"], a["m"], a["grids"], a["x"], a["nobs"],
                                         1.0, 0.5, a["w"], a["nw"], a["nsplit"], a["out"], None)
        if name == "hgp_kuf_semi_mc_matvec":
            return L.hgp_kuf_semi_mc_matvec(a["dtype"], a["kind"], 1.0, a["ndim"], a["m"], a["grids"], a["x"],
                                            a["nobs"], 1.0, 0.5, a["npts"], a["u"], a["w"], a["nw"], a["nsplit"],
                                            a["out"], None)
        return L.hgp_kuf_semi_sqexp_matvec(a["dtype"], a["ndim"], a["m"], a["grids"], a["x"], a["nobs"], 1.0, 0.5,
                                           a["w"], a["nw"], a["nsplit"], a["out"], None)


BAD = [("null_x", dict(x=None)), ("null_w", dict(w=None)), ("null_out", dict(out=None)), ("null_m", dict(m=None)),
       ("null_grids", dict(grids=None)), ("null_u", dict(u=None)), ("bad_dtype", dict(dtype=7)),
       ("bad_kind", dict(kind=9)), ("negative_kind", dict(kind=-1)), ("ndim0", dict(ndim=0)), ("ndim4", dict(ndim=4)),
       ("negative_nobs", dict(nobs=-1)), ("negative_nw", dict(nw=-1)), ("negative_nsplit", dict(nsplit=-1)),
       ("npts0", dict(npts=0)), ("npts1025", dict(npts=1025))]

# (the semi-sqexp entry has no kind; only the semi-mc entry has npts and u)
BAD_CALLS = [(n, t, o) for n in MV_SYMS for t, o in BAD
             if not (t in ("bad_kind", "negative_kind") and n == "hgp_kuf_semi_sqexp_matvec")
             and not (t in ("npts0", "npts1025", "null_u") and n != "hgp_kuf_semi_mc_matvec")]


@pytest.mark.parametrize("name,tag,over", BAD_CALLS, ids=[f"{c[0]}-{c[1]}" for c in BAD_CALLS])
def test_matvec_entries_refuse_bad_arguments(name, tag, over):
    from hipgp_amd import _lib
    L = _lib.lib()
    rc = _Args().call(L, name, **over)
    assert rc == E_ARG, (name, tag, rc)
    assert len(L.hgp_last_error()) > 0


@pytest.mark.parametrize("name", MV_SYMS)
@pytest.mark.parametrize("over", [dict(nobs=0), dict(nw=0), dict(nobs=0, x=None, out=None), dict(nw=0, w=None)],
                         ids=["nobs0", "nw0", "nobs0_null", "nw0_null"])
def test_empty_products_return_zero_before_any_launch(name, over):
    from hipgp_amd import _lib
    a = _Args()
    for i in range(64):
        a.buf[i] = 3.0
    assert a.call(_lib.lib(), name, **over) == 0
    assert all(v == 3.0 for v in a.buf), "an empty product wrote something"


def test_grid_matvec_refuses_gneiting_as_the_forward_does():
    """Gneiting is a semi-mc kernel only: the point product answers it exactly as hgp_kuf_grid."""
    from hipgp_amd import _lib
    L = _lib.lib()
    a = _Args()
    p = a.kw["x"]
    fwd = L.hgp_kuf_grid(F32, GNEITING, 2, a.m, a.grids, p, 2, 1.0, 0.5, p, None)
    assert fwd == E_ARG
    assert a.call(L, "hgp_kuf_grid_matvec", kind=GNEITING) == fwd
    assert b"kind" in L.hgp_last_error()


def test_wrappers_decline_cpu_tensors_and_unsupported_kernels():
    import hipgp_amd.ziggy.kernels as zk
    from hipgp_amd import kuf
    k = zk.SqExp(dtype=torch.float32)
    grids = [torch.linspace(-1, 1, 8)] * 2
    x = torch.full((3, 2), 0.4)
    W = torch.ones(2, 64)
    assert kuf.kuf_grid_matvec(k, grids, x, (1.0, 0.3), W) is None
    assert kuf.kuf_semi_mc_matvec(k, grids, x, (1.0, 0.3), 4, W=W) is None
    assert kuf.kuf_semi_sqexp_matvec(k, grids, x, (1.0, 0.3), W) is None
    assert list(inspect.signature(kuf.kuf_grid_matvec).parameters) == ["kernel", "xgrids", "x", "params", "W", "nsplit"]
    assert inspect.signature(kuf.kuf_grid_matvec).parameters["nsplit"].default == 0
    assert list(inspect.signature(kuf.kuf_semi_mc_matvec).parameters)[:6] == ["kernel", "xgrids", "x", "params",
                                                                              "npts", "u"]


def test_new_fp32_matvec_kernels_do_not_spill():
    ks = [k for k in _kernels() if re.search(r"hgp::k_kuf_\w*mv\w*<float", k[0])]
    point = [k for k in ks if "k_kuf_grid_mv<float" in k[0]]
    semi = [k for k in ks if "k_kuf_semi_mv<float" in k[0]]
    assert len(point) >= 4 and len(semi) >= 2 and any("k_kuf_mv_finish<float" in k[0] for k in ks), [k[0] for k in ks]
    bad = [f"{n} (spill {s}, scratch {p}, vgpr {v})" for n, s, p, v in ks if s or p]
    assert not bad, "fp32 Kuf product kernels spilling to scratch:\n" + "\n".join(bad)


def test_model_methods_exist_with_their_signatures():
    import hipgp_amd.ziggy.hipgp as hg
    T = hg.ToeplitzInducingGP
    assert list(inspect.signature(T.mean_weights).parameters) == ["self", "v", "maxiter_cg", "tol", "Kmm"]
    sig = inspect.signature(T.mean_weights).parameters
    assert (sig["v"].default, sig["maxiter_cg"].default, sig["tol"].default, sig["Kmm"].default) == (None, 50, 1e-8, None)
    assert list(inspect.signature(T.predict_mean).parameters) == [
        "self", "x", "integrated_obs", "semi_integrated_estimator", "semi_integrated_samps", "maxiter_cg", "Kmm",
        "weights", "batch_size", "mc_offset"]
    assert list(inspect.signature(T.predict_draws).parameters) == [
        "self", "x", "n", "eps", "generator", "integrated_obs", "semi_integrated_estimator", "semi_integrated_samps",
        "maxiter_cg", "Kmm", "batch_size", "mc_offset"]
    for cls in (hg.MeanFieldToeplitzGP, hg.BlockToeplitzGP):
        assert cls.predict_mean is T.predict_mean and cls.predict_draws is T.predict_draws
        assert cls.variational_draws is not T.variational_draws
    doc = T.predict_draws.__doc__
    assert "projected process" in doc.lower() and "K_xu K^-1 u" in doc and "ktilde" in doc


# ---- host logic on the oracle stand-in ---------------------------------------------------------
class SolvingKmm(OracleKmm):
    """`OracleKmm` with the solve the new methods need: dense K from the oracle's own K operator,
    solved directly (a converged solve, whatever maxiter says)."""

    def __init__(self, O):
        super().__init__(O)
        self.K = O.matmul_K(np.eye(O.M, dtype=O.dtype)).T.copy()

    def inv_matmul(self, b, do_precond=True, maxiter=20, tol=1e-8):
        self.calls.append(("solve", tuple(b.shape)))
        return torch.from_numpy(np.linalg.solve(self.K, b.detach().numpy().T).T.copy())


def _oracle():
    grids = [np.linspace(-1, 1, m) for m in DIMS]
    col = zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("matern", x, y, (1., .3), nu=1.5), 1e-3)
    return zo.ToeplitzOracle(col, DIMS)


def _model(family="mean-field", whitened_type="ziggy"):
    import hipgp_amd.ziggy.hipgp as hg
    import hipgp_amd.ziggy.kernels as zk
    dt = torch.float64
    grids = [torch.linspace(-1, 1, m, dtype=dt) for m in DIMS]
    torch.manual_seed(5)
    kw = dict(num_obs=40, sig2_init=1., ell_init=.3, noise2_init=.05, learn_kernel=False, dtype=dt,
              whitened_type=whitened_type)
    g = torch.Generator().manual_seed(11)
    if family == "block":
        mod = hg.BlockToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, block_sizes=[2, 2], **kw)
        with torch.no_grad():       # random theta1, theta2 = -(A A^T + I) / 2 per block
            mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=dt))
            if whitened_type == "ziggy":
                A = torch.randn(mod.num_blocks, mod.block_size, mod.block_size, generator=g, dtype=dt)
                mod.global_theta2.copy_(-.5 * (A.matmul(A.transpose(1, 2)) + torch.eye(mod.block_size, dtype=dt)))
        return mod
    mod = hg.MeanFieldToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, **kw)
    with torch.no_grad():
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=dt))
        mod.global_theta2.copy_(-(torch.rand(mod.Mprime, 1, generator=g, dtype=dt) * 4 + .5))
    return mod


def _points(n=13):
    g = torch.Generator().manual_seed(21)
    return torch.rand(n, 2, generator=g, dtype=torch.float64) * 2.4 - 1.2      # some outside the grid's hull


def _dense_S_half(mod):
    """S^{1/2} (M', M') dense in grid order: diag sqrt(qS), or the block Cholesky factors scattered."""
    _, qS = mod.standard_variational_params()
    if mod.name == "mean-field":
        return np.diag(np.sqrt(qS.detach().numpy().reshape(-1)))
    L = torch.linalg.cholesky(qS.detach()).numpy()
    out = np.zeros((mod.Mprime, mod.Mprime))
    idx = mod.block_idx.numpy()
    for b in range(mod.num_blocks):
        out[np.ix_(idx[b], idx[b])] = L[b]
    return out


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_mean_weights_and_predict_mean_match_dense(family):
    mod, O = _model(family), _oracle()
    Kmm = SolvingKmm(O)
    R = dense_R(O)
    qm = mod.standard_variational_params()[0].detach().numpy().reshape(-1)
    x = _points()
    Knm = mod.kernel(x, mod.xinduce, mod.get_kernel_params()).detach().numpy()
    alpha_ref = np.linalg.solve(Kmm.K, R @ qm)
    alpha = mod.mean_weights(Kmm=Kmm)
    assert tuple(alpha.shape) == (1, O.M) and not alpha.requires_grad
    assert Kmm.calls == [("R", (1, O.Mp)), ("solve", (1, O.M))]
    assert max_rel(alpha.numpy()[0], alpha_ref) < 1e-9
    mu = mod.predict_mean(x, Kmm=Kmm)
    assert tuple(mu.shape) == (13, 1) and mu.device.type == "cpu" and not mu.requires_grad
    assert max_rel(mu.numpy()[:, 0], Knm @ alpha_ref) < 1e-9
    # the weights kept from the earlier call, and the fallback in pieces with a tail
    ncalls = len(Kmm.calls)
    assert torch.equal(mod.predict_mean(x, weights=alpha), mu)
    assert len(Kmm.calls) == ncalls, "predict_mean solved again although weights were given"
    assert max_rel(mod.predict_mean(x, weights=alpha, batch_size=5).numpy()[:, 0], Knm @ alpha_ref) < 1e-9
    assert tuple(mod.predict_mean(x[:0], weights=alpha).shape) == (0, 1)
    # several right-hand sides through mean_weights
    V = torch.randn(3, O.Mp, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    A = mod.mean_weights(V, Kmm=Kmm)
    assert max_rel(A.numpy(), np.linalg.solve(Kmm.K, R @ V.numpy().T).T) < 1e-9
    with pytest.raises(ValueError):
        mod.mean_weights(V[:, :-1], Kmm=Kmm)


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_predict_draws_match_dense(family):
    mod, O = _model(family), _oracle()
    Kmm = SolvingKmm(O)
    R = dense_R(O)
    qm = mod.standard_variational_params()[0].detach().numpy().reshape(-1)
    x = _points()
    Knm = mod.kernel(x, mod.xinduce, mod.get_kernel_params()).detach().numpy()
    eps = torch.randn(4, O.Mp, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    keep = eps.clone()
    V = qm[None, :] + eps.numpy() @ _dense_S_half(mod).T
    assert max_rel(mod.variational_draws(4, eps=eps).numpy(), V) < 1e-12
    ref = (Knm @ np.linalg.solve(Kmm.K, R @ V.T)).T
    d = mod.predict_draws(x, 4, eps=eps, Kmm=Kmm)
    assert tuple(d.shape) == (4, 13) and d.device.type == "cpu" and not d.requires_grad
    assert torch.equal(eps, keep), "predict_draws changed the caller's eps"
    assert max_rel(d.numpy(), ref) < 1e-9
    assert Kmm.calls == [("R", (4, O.Mp)), ("solve", (4, O.M))]
    with pytest.raises(ValueError):
        mod.predict_draws(x, 3, eps=eps, Kmm=Kmm)
    # zero eps: every draw is the mean
    d0 = mod.predict_draws(x, 2, eps=torch.zeros(2, O.Mp, dtype=torch.float64), Kmm=Kmm)
    mu = mod.predict_mean(x, Kmm=Kmm)
    assert max_rel(d0.numpy(), np.stack([mu.numpy()[:, 0]] * 2)) < 1e-12
    # from a generator: reproducible, and equal to the draws of the same eps
    a = mod.predict_draws(x, 2, generator=torch.Generator().manual_seed(9), Kmm=Kmm)
    b = mod.predict_draws(x, 2, generator=torch.Generator().manual_seed(9), Kmm=Kmm)
    e9 = torch.randn((2, O.Mp), generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    assert torch.equal(a, b) and torch.equal(a, mod.predict_draws(x, 2, eps=e9, Kmm=Kmm))


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_cholesky_whitening_refuses(family):
    mod = _model(family, whitened_type="cholesky")
    Kmm = SolvingKmm(_oracle())
    x = _points()
    for call in (lambda: mod.mean_weights(Kmm=Kmm), lambda: mod.predict_mean(x, Kmm=Kmm),
                 lambda: mod.predict_draws(x, 2, Kmm=Kmm)):
        with pytest.raises(NotImplementedError, match="cholesky whitening has no circulant R"):
            call()
    assert Kmm.calls == []
