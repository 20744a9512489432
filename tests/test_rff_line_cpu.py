"""The fused line-integral feature product (hgp_rff_line_matvec), `hipgp_amd.rff.rff_line_matvec` and
the joint draws of line integrals `predict_line_samples` without a GPU: the ABI and its argument
checks (all made before any HIP call), the register budget of the fp32 kernels, the closed form
against a quadrature that does not know it, the integrated features against the semi-integrated
kernels, and the model method on the fp64 oracle stand-in (where the products take their torch
routes) against a dense NumPy restatement and, statistically, against
`predict(integrated_obs=True)`."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from grid_posterior_cases import dense_R, max_rel
from oracle import ziggy_oracle as zo
from rff_line_cases import (SPECIAL_T, quad_line_features, special_features, special_row, with_specials)
from test_kernel_resources_cpu import _kernels
from test_kuf_matvec_cpu import SolvingKmm, _dense_S_half, _model, _oracle, _points
from test_rff_cpu import BAD, FullKmm, _kernel_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
F32 = 0
LINE_ARGS = ("dtype", "ndim", "x", "nobs", "omega", "phase", "nfeat", "w", "nw", "scale", "transposed", "beta",
             "nsplit", "out")


def test_header_declares_and_library_exports_the_entry():
    from hipgp_amd import _lib
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    assert re.search(r"\bint\s+hgp_rff_line_matvec\s*\(", src), "include/hipgp.h does not declare hgp_rff_line_matvec"
    assert hasattr(_lib.lib(), "hgp_rff_line_matvec"), "libhipgp.so does not export hgp_rff_line_matvec"
    assert "hgp_rff_line_matvec" in _lib.EXPORTS


class _Args:
    """A well-formed argument set (host addresses standing in for device ones: every call below must
    return before anything is launched), with fields replaced per case."""

    def __init__(self):
        self.buf = (ctypes.c_float * 64)()
        p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.kw = dict(dtype=F32, ndim=2, x=p, nobs=2, omega=p, phase=p, nfeat=3, w=p, nw=2, scale=1.0, transposed=0,
                       beta=0.0, nsplit=0, out=p)

    def call(self, L, **over):
        a = dict(self.kw, **over)
        return L.hgp_rff_line_matvec(*[a[k] for k in LINE_ARGS], None)


# the cases of test_rff_cpu's list that apply to explicit points: those that replace no mesh argument
# ("neither_x_nor_grids" is x = NULL here)
BAD_LINE = [(tag, over) for tag, over in BAD if set(over) <= set(LINE_ARGS)]


def test_the_bad_cases_are_those_of_the_point_entry():
    assert [t for t, _ in BAD_LINE] == ["null_omega", "null_phase", "null_w", "null_out", "bad_dtype", "ndim0", "ndim4",
                                        "negative_nobs", "negative_nfeat", "negative_nw", "negative_nsplit",
                                        "nfeat0_with_points", "neither_x_nor_grids"]


@pytest.mark.parametrize("tag,over", BAD_LINE, ids=[c[0] for c in BAD_LINE])
def test_entry_refuses_bad_arguments_before_any_hip_call(tag, over):
    from hipgp_amd import _lib
    L = _lib.lib()
    a = _Args()
    for i in range(64):
        a.buf[i] = 3.0
    assert a.call(L, **over) == E_ARG, tag
    assert len(L.hgp_last_error()) > 0
    assert all(v == 3.0 for v in a.buf)


@pytest.mark.parametrize("over", [dict(nobs=0), dict(nw=0), dict(nobs=0, omega=None, w=None, out=None, nfeat=0),
                                  dict(nw=0, w=None, out=None)], ids=["nobs0", "nw0", "nobs0_null", "nw0_null"])
def test_empty_products_return_zero_before_any_launch(over):
    from hipgp_amd import _lib
    a = _Args()
    for i in range(64):
        a.buf[i] = 3.0
    assert a.call(_lib.lib(), **over) == 0
    assert all(v == 3.0 for v in a.buf), "an empty product wrote something"


def test_fp32_line_kernels_do_not_spill():
    ks = [k for k in _kernels() if "hgp::k_rff_line_mv<float" in k[0]]
    assert len(ks) == 3, ks
    bad = [f"{n} (spill {s}, scratch {p}, vgpr {v})" for n, s, p, v in ks if s or p]
    assert not bad, "fp32 line feature kernels spilling to scratch:\n" + "\n".join(bad)
    assert all(v <= 64 for _, _, _, v in ks), ks          # 8 waves per SIMD, as the point kernels


def test_wrapper_declines_cpu_tensors_and_signatures():
    import hipgp_amd.ziggy.hipgp as hg
    from hipgp_amd import rff
    om, ph, W = torch.ones(5, 2, dtype=torch.float64), torch.zeros(5, dtype=torch.float64), torch.ones(2, 5)
    assert rff.rff_line_matvec(om, ph, W, torch.zeros(3, 2)) is None
    assert list(inspect.signature(rff.rff_line_matvec).parameters) == ["omega", "phase", "W", "x", "scale",
                                                                      "transposed", "out", "beta", "nsplit"]
    T = hg.ToeplitzInducingGP
    assert inspect.signature(T._rff_product).parameters["line"].default is False
    sig = inspect.signature(T.predict_line_samples).parameters
    assert list(sig) == ["self", "x", "n", "xpoint", "nfeat", "eps", "features", "prior_w", "nugget_eps", "generator",
                         "maxiter_cg", "Kmm", "semi_integrated_estimator", "semi_integrated_samps", "mc_offset",
                         "batch_size"]
    assert (sig["xpoint"].default, sig["nfeat"].default, sig["maxiter_cg"].default,
            sig["semi_integrated_estimator"].default, sig["semi_integrated_samps"].default) == (None, 4096, 50,
                                                                                              "analytic", 10)
    for cls in (hg.MeanFieldToeplitzGP, hg.BlockToeplitzGP):
        assert cls.predict_line_samples is T.predict_line_samples
    doc = T.predict_line_samples.__doc__
    assert "mc-biased" in doc and "K^-1" in doc and "exceeds" in doc


# ---- the closed form ---------------------------------------------------------------------------
@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_closed_form_matches_a_quadrature(ndim):
    """The torch route in fp64 against composite Gauss-Legendre quadrature of
    |x| int_0^1 cos(a omega . x + b) da (128 panels of 48 nodes: `quad_line_features` says why that is
    enough for the largest |omega . x| here, asserted below 1000 revolutions), at random rows and
    features and at the special ones: x = 0, omega . x = 0 exactly, |t| = 1e-9, 1e-3, 0.2499, 0.2501
    with both signs and about 500 revolutions.  Element by element, over the largest element."""
    from hipgp_amd import rff
    g = torch.Generator().manual_seed(40 + ndim)
    dt = torch.float64
    x, omega = with_specials(torch.rand(9, ndim, generator=g, dtype=dt) * 1.6 - .8,
                             torch.randn(20, ndim, generator=g, dtype=dt) / .3, ndim)
    phase = torch.rand(20, generator=g, dtype=dt) * 2 * np.pi
    xs = special_row(ndim)
    assert torch.equal(x[-2], xs) and not x[-1].any()
    t = (special_features(ndim) @ xs / (2 * np.pi)).numpy()
    assert t[0] == 0 and np.allclose(t[1:], SPECIAL_T, rtol=1e-12, atol=0), t
    assert float((x @ omega.t()).abs().max()) < 1000 * 2 * np.pi
    got = rff.line_features(omega, phase, x)
    ref = quad_line_features(omega, phase, x)
    err = max_rel(got.numpy(), ref)
    print(f"{ndim}-D: closed form vs quadrature {err:.2e} of max |L|; at the special row: "
          + " ".join(f"{abs(a - b):.1e}" for a, b in zip(got[-2, -8:].numpy(), ref[-2, -8:])))
    assert err <= 1e-12
    assert not got[-1].any(), "the row x = 0 is not exactly 0"
    # omega . x = 0 exactly: sinc is exactly 1
    assert got[-2, -8] == torch.linalg.vector_norm(xs) * torch.cos(phase[-8])


def test_rff_product_line_mode_is_the_closed_form_in_pieces():
    """`_rff_product(line=True)` on CPU tensors: scale * L W^T, both layouts, accumulated."""
    from hipgp_amd import rff
    mod = _model()
    g = torch.Generator().manual_seed(3)
    dt = torch.float64
    x, omega = with_specials(_points(), torch.randn(29, 2, generator=g, dtype=dt) / .3, 2)
    phase = torch.rand(29, generator=g, dtype=dt) * 2 * np.pi
    W = torch.randn(3, 29, generator=g, dtype=dt)
    ref = .7 * quad_line_features(omega, phase, x) @ W.numpy().T
    a = mod._rff_product(x, omega, phase, W, .7, line=True)
    assert tuple(a.shape) == (13, 3) and max_rel(a.numpy(), ref) <= 1e-12
    start = torch.randn(3, 13, generator=g, dtype=dt)
    b = mod._rff_product(x, omega, phase, W, .7, transposed=True, out=start.clone(), beta=1.0, line=True)
    assert max_rel(b.numpy(), start.numpy() + ref.T) <= 1e-12
    point = .7 * torch.cos(x @ omega.t() + phase) @ W.t()                           # the default is the point product
    assert max_rel(mod._rff_product(x, omega, phase, W, .7).numpy(), point.numpy()) <= 1e-14
    with pytest.raises(TypeError):
        mod._rff_product(None, omega, phase, W, .7, line=True)
    assert rff.line_features(omega, phase, x[:0]).shape == (0, 29)


# ---- the integrated features against the semi-integrated kernels ----------------------------------
@pytest.mark.parametrize("name", ["sqexp", "matern12", "matern32", "matern52"])
def test_integrated_features_reproduce_the_semi_integrated_kernel(name):
    """(2 sig2 / F) sum_f L_f(x) cos(w_f . u + b_f) is a mean of F terms bounded by 2 sig2 |x| with
    expectation k_semi(u, x): 10 sig2 |x| / sqrt(F) is five standard deviations of that mean at the
    most (`test_spectral_features_reproduce_the_kernel`'s bound times |x|).  SqExp: against the
    analytic `k_semi`; Matern: against a 200-node Gauss-Legendre quadrature of the point kernel."""
    from hipgp_amd import rff
    kernel = dict(_kernel_cases())[name]
    sig2, ell, F = 1.7, 0.3, 2 ** 14
    g = torch.Generator().manual_seed(4321)
    dt = torch.float64
    omega, phase = rff.spectral_features(kernel, (sig2, ell), 2, F, generator=g)
    x = torch.rand(50, 2, generator=g, dtype=dt) * 2 - 1                          # the lines
    u = x * torch.rand(50, 1, generator=g, dtype=dt) + (torch.rand(50, 2, generator=g, dtype=dt) - .5) \
        * torch.linspace(0, 2, 50, dtype=dt)[:, None]                            # points on, near and far from them
    L = rff.line_features(omega, phase, x)
    approx = (2 * sig2 / F) * torch.sum(L * torch.cos(u @ omega.t() + phase), dim=1)
    if name == "sqexp":
        exact = torch.stack([kernel.k_semi(u[i:i + 1], x[i:i + 1], (sig2, ell))[0, 0] for i in range(50)])
    else:
        s, w = np.polynomial.legendre.leggauss(200)
        a, w = torch.tensor((s + 1) / 2), torch.tensor(w / 2)
        exact = torch.stack([torch.linalg.vector_norm(x[i]) * (kernel(u[i:i + 1], a[:, None] * x[i], (sig2, ell))[0] @ w)
                             for i in range(50)])
    bound = 10 * sig2 * torch.linalg.vector_norm(x, dim=1) / np.sqrt(F)
    err = (approx - exact).abs()
    print(f"{name}: max |features - k_semi| / bound = {float((err / bound).max()):.3f} "
          f"(max error {float(err.max()):.4f})")
    assert bool((err < bound).all())


# ---- predict_line_samples on the oracle stand-in ------------------------------------------------------
NPTS_MC, U_MC = 7, 0.3


def _dense_line_samples(mod, Kmm, R, x, xpoint, eps, omega, phase, W, xi):
    """The steps in NumPy, the prior's line integral by quadrature and the cross-covariance as the
    biased MC estimator with NPTS_MC nodes at offset U_MC: (n, N) lines and (n, Np) points."""
    params = mod.get_kernel_params()
    F = omega.shape[0]
    s = np.sqrt(2 * float(params[0]) / F)
    qm = mod.standard_variational_params()[0].detach().numpy().reshape(-1)
    U = mod.xinduce.numpy()
    prior = lambda p: s * np.cos(p @ omega.T + phase[None, :]) @ W.T                 # (points, n)
    V = qm[None, :] + eps @ _dense_S_half(mod).T
    u = R @ V.T                                                                      # (M, n)
    alpha = np.linalg.solve(Kmm.K, u - prior(U) - np.sqrt(mod.jitter_val) * xi.T)
    nodes = (np.arange(NPTS_MC) + U_MC) / NPTS_MC
    Ksemi = sum(mod.kernel(a * x, mod.xinduce, params).detach().numpy() for a in nodes) / NPTS_MC
    Ksemi = Ksemi * np.linalg.norm(x.numpy(), axis=1)[:, None]
    lines = s * quad_line_features(omega, phase, x.numpy()) @ W.T + Ksemi @ alpha
    Knm = mod.kernel(xpoint, mod.xinduce, params).detach().numpy()
    return lines.T, (prior(xpoint.numpy()) + Knm @ alpha).T


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_predict_line_samples_match_the_dense_restatement(family, monkeypatch):
    """On CPU tensors `_kuf_product` goes through `_make_grams`, which also makes the doubly-integrated
    diagonal (not used here) by a table interpolation that runs on the device only: the project's torch
    statement of the same formula stands in for it."""
    from hipgp_amd import kuf, rff
    monkeypatch.setattr(kuf, "knn_doubly_diag", kuf.knn_doubly_diag_ad)
    mod, O = _model(family), _oracle()
    Kmm = SolvingKmm(O)
    R = dense_R(O)
    n, F = 3, 37
    g = torch.Generator().manual_seed(8)
    dt = torch.float64
    eps = torch.randn(n, O.Mp, generator=g, dtype=dt)
    omega, phase = rff.spectral_features(mod.kernel, mod.get_kernel_params(), 2, F, generator=g)
    x = _points()
    x[-1] = 0
    xpoint = _points(5) * .9
    W = torch.randn(n, F, generator=g, dtype=dt)
    xi = torch.randn(n, O.M, generator=g, dtype=dt)
    u = torch.tensor([U_MC], dtype=dt)
    keep = [t.clone() for t in (eps, omega, phase, W, xi, x, xpoint, u)]
    ref_l, ref_p = _dense_line_samples(mod, Kmm, R, x, xpoint, eps.numpy(), omega.numpy(), phase.numpy(), W.numpy(),
                                       xi.numpy())
    kw = dict(eps=eps, features=(omega, phase), prior_w=W, nugget_eps=xi, Kmm=Kmm,
              semi_integrated_estimator="mc-biased", semi_integrated_samps=NPTS_MC, mc_offset=u)
    d = mod.predict_line_samples(x, n, **kw)
    assert tuple(d.shape) == (n, 13) and d.device.type == "cpu" and not d.requires_grad
    assert Kmm.calls == [("R", (n, O.Mp)), ("solve", (n, O.M))]
    err = max_rel(d.numpy(), ref_l)
    print(f"{family}: predict_line_samples vs dense restatement {err:.2e}")
    assert err <= 1e-12
    assert not d[:, -1].any(), "the line to x = 0 is not exactly 0"
    # with points: a pair from ONE solve, the lines unchanged, the points those of predict_samples
    Kmm.calls.clear()
    dl, dp = mod.predict_line_samples(x, n, xpoint=xpoint, **kw)
    assert Kmm.calls == [("R", (n, O.Mp)), ("solve", (n, O.M))]
    assert torch.equal(dl, d) and tuple(dp.shape) == (n, 5) and dp.device.type == "cpu"
    assert all(torch.equal(a, b) for a, b in zip(keep, (eps, omega, phase, W, xi, x, xpoint, u))), "an input changed"
    ps = mod.predict_samples(xpoint, n, eps=eps, features=(omega, phase), prior_w=W, nugget_eps=xi, Kmm=Kmm)
    errp, errs = max_rel(dp.numpy(), ref_p), max_rel(dp.numpy(), ps.numpy())
    print(f"{family}: point rows vs dense restatement {errp:.2e}, vs predict_samples {errs:.2e}")
    assert errp <= 1e-12 and errs <= 1e-14
    # the pieces of the fallback with a tail; a generator gives the same draws twice; shapes are checked
    assert max_rel(mod.predict_line_samples(x, n, batch_size=5, **kw).numpy(), ref_l) <= 1e-12
    ga = dict(nfeat=16, Kmm=Kmm, semi_integrated_estimator="mc-biased", mc_offset=u)
    a = mod.predict_line_samples(x, 2, xpoint=xpoint, generator=torch.Generator().manual_seed(3), **ga)
    b = mod.predict_line_samples(x, 2, xpoint=xpoint, generator=torch.Generator().manual_seed(3), **ga)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and tuple(a[0].shape) == (2, 13)
    assert torch.equal(a[1], mod.predict_samples(xpoint, 2, nfeat=16, generator=torch.Generator().manual_seed(3),
                                                 Kmm=Kmm))
    for bad in (dict(prior_w=W[:, :-1]), dict(nugget_eps=xi[:, :-1]), dict(eps=eps[:, :-1]),
                dict(features=(omega[:, :1], phase))):
        with pytest.raises(ValueError):
            mod.predict_line_samples(x, n, **dict(kw, **bad))


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_cholesky_whitening_refuses_and_predict_samples_still_refuses_lines(family):
    Kmm = SolvingKmm(_oracle())
    x = _points()
    with pytest.raises(NotImplementedError, match="cholesky whitening has no circulant R"):
        _model(family, whitened_type="cholesky").predict_line_samples(x, 2, nfeat=8, Kmm=Kmm)
    with pytest.raises(NotImplementedError, match="integrated_obs"):
        _model(family).predict_samples(x, 2, nfeat=8, Kmm=Kmm, integrated_obs=True)
    assert Kmm.calls == []


def _doubly_integrated_sqexp(d):
    """int_0^1 int_0^1 exp(-(a - a')^2 d^2 / 2) da da' d^2 = 2 d^2 int_0^1 (1 - s) exp(-s^2 d^2 / 2) ds for
    d = |x| / ell, by 400-node Gauss-Legendre quadrature (the integrand's width is 1 / d >= 1 / 30)."""
    s, w = np.polynomial.legendre.leggauss(400)
    s, w = (s + 1) / 2, w / 2
    return np.array([2 * di * di * np.sum(w * (1 - s) * np.exp(-.5 * (s * di) ** 2)) for di in d])


def test_line_samples_have_predicts_mean_and_variance_where_predict_draws_do_not(monkeypatch):
    """12 x 10 grid on [0, 1]^2, SqExp(1, 0.05), jitter 1e-3, F = 4096, 20 000 draws, analytic
    estimator, at the lines to the seven points of the point test: the residual ktilde is at least
    half of `predict(integrated_obs=True)`'s variance there.  The draws' variance over `predict`'s lies
    in [0.8, 1.25] and their mean within 0.05 sd of `predict`'s, while the projected draws of
    `predict_draws(integrated_obs=True)` have less than 0.6 of the variance.

    `predict`'s Knn_diag is the interpolated doubly-integrated table (N = 50, dmax = 5, linear beyond):
    it is asserted within 2 % of a quadrature of the doubly-integrated kernel at these lines, so that a
    table error cannot pass for, or hide, a sampler error.  The table's interpolation runs on the
    device only; here the project's torch statement of the same formula (`knn_doubly_diag_ad`)
    stands in for it inside `predict`."""
    import hipgp_amd.ziggy.hipgp as hg
    import hipgp_amd.ziggy.kernels as zk
    from hipgp_amd import kuf
    monkeypatch.setattr(kuf, "knn_doubly_diag", kuf.knn_doubly_diag_ad)
    dt = torch.float64
    dims, ell, jit, F, n = (12, 10), .05, 1e-3, 4096, 20000
    grids = [np.linspace(0, 1, m) for m in dims]
    O = zo.ToeplitzOracle(zo.toeplitz_column(grids, lambda a, b: zo.kernel_eval("sqexp", a, b, (1., ell)), jit), dims)
    Kmm = FullKmm(O)
    torch.manual_seed(2)
    kernel = zk.SqExp(dtype=dt)
    mod = hg.MeanFieldToeplitzGP(kernel, [torch.tensor(g) for g in grids], num_obs=50, sig2_init=1.,
                                 ell_init=ell, noise2_init=.05, learn_kernel=False, dtype=dt, jitter_val=jit)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=dt))
        mod.global_theta2.copy_(-(torch.rand(mod.Mprime, 1, generator=g, dtype=dt) * 4 + 1))     # S in [0.1, 0.5]
    h0, h1 = 1 / 11, 1 / 9
    x = torch.tensor([[2.5 * h0, 3.5 * h1], [6.5 * h0, 0.5 * h1], [9.5 * h0, 7.5 * h1], [4.5 * h0, 5 * h1],
                      [7 * h0, 2.5 * h1], [-.06, .45], [1.07, 1.06]], dtype=dt)
    params = mod.get_kernel_params()
    table = kernel.k_doubly_diag(x, params).detach().numpy()
    quad = ell * ell * _doubly_integrated_sqexp(np.linalg.norm(x.numpy(), axis=1) / ell)
    print("doubly-integrated table / quadrature:", np.round(table / quad, 4))
    assert np.all(np.abs(table / quad - 1) < .02), table / quad
    mu, sd = mod.predict(x, integrated_obs=True, maxiter_cg=50, Kmm=Kmm)
    mu, var = mu.numpy().reshape(-1), sd.numpy().reshape(-1) ** 2
    proj_var = mod.predict_draws(x, n, generator=g, integrated_obs=True, Kmm=Kmm).numpy().var(axis=0)
    Knm = kernel.k_semi(mod.xinduce, x, params).numpy().T
    kn = O.matmul_RT(np.linalg.solve(Kmm.K, Knm.T).T).reshape(len(x), -1)
    ktilde = table - np.sum(kn * kn, axis=1)
    print("ktilde / predict variance:", np.round(ktilde / var, 3))
    assert np.all(ktilde >= .5 * var), ktilde / var
    draws = mod.predict_line_samples(x, n, nfeat=F, generator=g, Kmm=Kmm).numpy()
    ratio = draws.var(axis=0) / var
    shift = (draws.mean(axis=0) - mu) / np.sqrt(var)
    pratio = proj_var / var
    print("variance ratio:", np.round(ratio, 3), "mean shift / sd:", np.round(shift, 4), "projected:", np.round(pratio, 3))
    assert np.all((ratio >= .8) & (ratio <= 1.25)), ratio
    assert np.all(np.abs(shift) < .05), shift
    assert np.all(pratio < .6), pratio
