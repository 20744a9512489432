"""`ToeplitzInducingGP.fit_mean` on the device: the optimal variational mean of all observations from one
matrix-free solve of (K + Kuf^T diag(iv) Kuf) beta = Kuf^T (iv o y), qm = R^T beta, through the fused
products hgp_kuf_*_matvec / hgp_kuf_*_rmatvec, against the dense `batch_solve` (kn per observation and
an M' x M' solve) on the 20 x 20 grid that method names, M' = 1444, 300 point observations.

Both sides truncate PCG solves (`batch_solve` one per observation at maxiter_cg = 200, `fit_mean` one at
tol = 1e-10), so the fp64 bounds are 10 x the gaps measured against `batch_solve` / `predict` /
the dense formula (the *_MEASURED figures below); the fp32 bound is the 4 x rule against the same
dense route in fp32 (fit_mean asked for tol = 1e-7, which its fp64 residual sweeps make
reachable).  Each test prints its figures before it asserts."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (20, 20)
NOBS = 300
CG = 200                              # maxiter_cg of the dense routes: their PCGs reach the break test
GAP_BATCH_SOLVE_F64_MEASURED = 9.0e-9  # worst max|qm - qm_batch_solve| / max|qm_batch_solve|, both families
GAP_PREDICT_F64_MEASURED = 1.7e-9      # worst max|predict_mean(weights) - predict mean| / max|predict mean|
GAP_LINE_F64_MEASURED = 3.3e-9         # worst gap to the dense formula of the line-integral routes


def _kern(kind, nu, dt):
    import ziggy.kernels as zk
    return zk.SqExp(dtype=dt) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dt)


def _model(family, dt, dims=DIMS, kern=("matern", 1.5), nobs=NOBS):
    import ziggy.hipgp as hg
    grids = [torch.linspace(-1, 1, m, dtype=dt) for m in dims]
    torch.manual_seed(5)
    kw = dict(num_obs=nobs, sig2_init=1., ell_init=.3, noise2_init=.05, learn_kernel=False, dtype=dt)
    g = torch.Generator().manual_seed(11)
    if family == "block":
        mod = hg.BlockToeplitzGP(_kern(*kern, dt), grids, block_sizes=[2] * len(dims), **kw)
        with torch.no_grad():
            A = torch.randn(mod.num_blocks, mod.block_size, mod.block_size, generator=g, dtype=dt) * .5
            mod.global_theta2.copy_(-.5 * (A.matmul(A.transpose(1, 2)) + torch.eye(mod.block_size, dtype=dt)))
    else:
        mod = hg.MeanFieldToeplitzGP(_kern(*kern, dt), grids, **kw)
        with torch.no_grad():
            mod.global_theta2.copy_(-(torch.rand(mod.Mprime, 1, generator=g, dtype=dt) * 4 + .5))
    with torch.no_grad():
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=dt))
    return mod.cuda_params(0)


def _data(dt, d=2, nobs=NOBS, line=False):
    """x in [-1.1, 1.1]^d (some outside the grid's hull; |x| >= 0.25 for line integrals), y a smooth
    function plus noise, per-observation noise sd in [0.1, 0.5]."""
    g = torch.Generator(device="cpu").manual_seed(41)
    x = torch.rand(nobs, d, generator=g, dtype=torch.float64) * 2.2 - 1.1
    if line:
        nrm = x.norm(dim=1, keepdim=True)
        x = torch.where(nrm < 0.25, x * (0.25 / nrm), x)
    sd = torch.rand(nobs, 1, generator=g, dtype=torch.float64) * .4 + .1
    y = torch.sin(3 * x[:, :1]) * torch.cos(2 * x[:, 1:2]) + sd * torch.randn(nobs, 1, generator=g, dtype=torch.float64)
    return x.to(dt).to(DEV), y.to(dt).to(DEV), sd.to(dt).to(DEV)


def _gap(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def _qm(mod):
    with torch.no_grad():
        return mod.standard_variational_params()[0].detach().clone()


@functools.lru_cache(maxsize=None)
def _solved(family, tag):
    """(qm of fit_mean, qm of batch_solve on a copy, the MeanFit): computed once per family and dtype."""
    dt = torch.float64 if tag == "f64" else torch.float32
    mod = _model(family, dt)
    x, y, sd = _data(dt)
    dense = copy.deepcopy(mod)
    dense.batch_solve(x, y, noise_std=sd, maxiter_cg=CG)
    if tag == "f64":
        fit = mod.fit_mean(x, y, noise_std=sd, tol=1e-10, maxiter=2000)
    else:
        fit = mod.fit_mean(x, y, noise_std=sd, tol=1e-7)      # reachable through the fp64 residual sweeps
    print(f"\nfit_mean {family} {tag}: {fit.iters} iterations, relres {fit.relres:.2e}")
    return _qm(mod), _qm(dense), fit


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_fit_mean_matches_batch_solve_fp64(family):
    qm, qm_dense, fit = _solved(family, "f64")
    g = _gap(qm, qm_dense)
    print(f"fit_mean vs batch_solve {family} fp64: relative gap {g:.3e} after {fit.iters} iterations "
          f"(measured worst {GAP_BATCH_SOLVE_F64_MEASURED:.1e}, limit 10 x)")
    assert fit.relres < 1e-10 and fit.iters < 2000
    assert tuple(fit.weights.shape) == (1, 400) and tuple(fit.qm.shape) == (1444, 1)
    assert fit.weights.device.type == "cuda" and not fit.weights.requires_grad
    assert _gap(qm, fit.qm) < 1e-11                      # update=True wrote the returned mean
    assert g <= 10 * GAP_BATCH_SOLVE_F64_MEASURED


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_fit_mean_fp32_within_four_times_batch_solve_fp32(family):
    """The 4 x rule against the dense route in the same precision.  Measured on one MI355X: fit_mean fp32
    against fit_mean fp64 7.0e-6 at tol = 1e-7 (374 iterations in two sweeps; 5.7e-5 at the default
    tol = 1e-6), batch_solve fp32 against batch_solve fp64 1.9e-5.  The fp32 recurrence alone stops at
    7.4e-4: the fp64 residual between sweeps is what carries it."""
    qm64, dense64, _ = _solved(family, "f64")
    qm32, dense32, fit = _solved(family, "f32")
    g, ref = _gap(qm32, qm64), _gap(dense32, dense64)
    print(f"fit_mean fp32 vs fp64 {family}: {g:.3e}; batch_solve fp32 vs fp64: {ref:.3e}; {fit.iters} iterations, "
          f"relres {fit.relres:.2e}")
    assert g <= 4 * ref


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_fit_mean_leaves_the_covariance_and_update_false_leaves_everything(family):
    dt = torch.float64
    mod = _model(family, dt)
    x, y, sd = _data(dt)
    before = {k: v.detach().clone() for k, v in mod.named_parameters()}
    fit = mod.fit_mean(x, y, noise_std=sd, tol=1e-6, update=False)
    assert all(torch.equal(before[k], v) for k, v in mod.named_parameters())
    mod.fit_mean(x, y, noise_std=sd, tol=1e-6)
    assert torch.equal(before["global_theta2"], mod.global_theta2)
    assert not torch.equal(before["global_theta1"], mod.global_theta1)
    assert _gap(_qm(mod), fit.qm) < 1e-11                # the same solve again, the same mean


def _set_qm(mod, qm):
    with torch.no_grad():
        lam = -2 * mod.global_theta2
        if mod.name == "mean-field":
            mod.global_theta1.copy_(lam * qm)
        else:
            mod.global_theta1.copy_(mod.block_diag_multiply(lam, qm.t()).t())


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_fitted_mean_maximises_the_elbo_fp64(family):
    """The whole data as one batch, shared noise: the ELBO after fit_mean is no lower than before it and no
    lower than at qm +- 1e-3 d for three seeded unit directions d."""
    dt = torch.float64
    mod = _model(family, dt)
    x, y, _ = _data(dt)
    with torch.no_grad():
        T = mod.toeplitz()
        e0 = float(mod.elbo(x, y, maxiter_cg=CG, Kmm=T))
        fit = mod.fit_mean(x, y, tol=1e-10, maxiter=2000, Kmm=T)
        e1 = float(mod.elbo(x, y, maxiter_cg=CG, Kmm=T))
        print(f"\nelbo {family}: before {e0:.12e}, after fit_mean {e1:.12e} ({fit.iters} iterations)")
        assert e1 >= e0
        g = torch.Generator(device="cpu").manual_seed(23)
        for i in range(3):
            d = torch.randn(mod.Mprime, 1, generator=g, dtype=dt)
            d = (d / d.norm()).to(DEV)
            for sgn in (1., -1.):
                _set_qm(mod, fit.qm + sgn * 1e-3 * d)
                e = float(mod.elbo(x, y, maxiter_cg=CG, Kmm=T))
                print(f"  direction {i} {sgn:+.0f}: elbo - optimum = {e - e1:.3e}")
                assert e <= e1
        _set_qm(mod, fit.qm)


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_predict_mean_from_the_fitted_weights_matches_predict_fp64(family):
    dt = torch.float64
    mod = _model(family, dt)
    x, y, sd = _data(dt)
    fit = mod.fit_mean(x, y, noise_std=sd, tol=1e-10, maxiter=2000)
    g = torch.Generator(device="cpu").manual_seed(6)
    xt = (torch.rand(37, 2, generator=g, dtype=dt) * 2.2 - 1.1).to(DEV)
    mu_ref, _ = mod.predict(xt, maxiter_cg=CG, fused=False, streamed=False)
    mu = mod.predict_mean(xt, weights=fit.weights)
    gap = _gap(mu, mu_ref)
    print(f"\npredict_mean(weights=beta) vs predict {family}: relative gap {gap:.3e} "
          f"(measured worst {GAP_PREDICT_F64_MEASURED:.1e}, limit 10 x)")
    assert tuple(mu.shape) == tuple(mu_ref.shape) == (37, 1)
    assert gap <= 10 * GAP_PREDICT_F64_MEASURED


@pytest.mark.parametrize("estimator,kern", [("analytic", ("sqexp", None)), ("mc-biased", ("matern", 2.5))],
                         ids=["analytic-sqexp", "mc-biased-matern2.5"])
def test_fit_mean_line_integrals_match_the_dense_formula_fp64(estimator, kern):
    """(6, 5, 4) grid, 200 line-integral observations, the fused line-integral products on both sides
    of the operator, against (I + sum iv kn kn^T)^-1 sum iv y kn with kn from the materialised
    `_make_grams` and `compute_kn`."""
    dt = torch.float64
    nobs = 200
    mod = _model("mean-field", dt, dims=(6, 5, 4), kern=kern, nobs=nobs)
    x, y, sd = _data(dt, d=3, nobs=nobs, line=True)
    u = torch.tensor([0.37], dtype=dt, device=DEV)
    kw = dict(integrated_obs=True, semi_integrated_estimator=estimator, semi_integrated_samps=6)
    if estimator == "mc-biased":
        kw["mc_offset"] = u
    with torch.no_grad():
        Knm, _ = mod._make_grams(x, **kw)
        kn = mod.compute_kn(Knm, maxiter_cg=CG)
        iv = 1 / sd ** 2
        big = torch.eye(mod.Mprime, dtype=dt, device=DEV) + (iv * kn).t().matmul(kn)
        mstar = torch.linalg.solve(big, (iv * y * kn).sum(dim=0)[:, None])
    fit = mod.fit_mean(x, y, noise_std=sd, tol=1e-10, maxiter=2000, update=False, **kw)
    gap = _gap(fit.qm, mstar)
    print(f"\nfit_mean {estimator} {kern[0]}: relative gap to the dense formula {gap:.3e} after {fit.iters} iterations "
          f"(measured worst {GAP_LINE_F64_MEASURED:.1e}, limit 10 x)")
    assert fit.relres < 1e-10
    assert gap <= 10 * GAP_LINE_F64_MEASURED
    if estimator == "mc-biased":
        again = mod.fit_mean(x, y, noise_std=sd, tol=1e-10, maxiter=2000, update=False, **kw)
        assert torch.equal(fit.weights, again.weights) and torch.equal(fit.qm, again.qm) and fit.iters == again.iters
