"""The fused Fourier-feature product (hgp_rff_matvec), `hipgp_amd.rff` and the pathwise-conditioned
draws `predict_samples` without a GPU: the ABI and its argument checks (all made before any HIP
call), the register budget of the fp32 kernels, the spectral sampler against the kernels, and the
model method on the fp64 oracle stand-in (where the feature product takes its torch route) against a
dense NumPy restatement and, statistically, against `predict`'s mean and sd."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from grid_posterior_cases import dense_R, max_rel
from oracle import ziggy_oracle as zo
from test_kernel_resources_cpu import _kernels
from test_kuf_matvec_cpu import SolvingKmm, _dense_S_half, _model, _oracle, _points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
F32 = 0


def test_header_declares_and_library_exports_the_entry():
    from hipgp_amd import _lib
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    assert re.search(r"\bint\s+hgp_rff_matvec\s*\(", src), "include/hipgp.h does not declare hgp_rff_matvec"
    assert hasattr(_lib.lib(), "hgp_rff_matvec"), "libhipgp.so does not export hgp_rff_matvec"
    assert "hgp_rff_matvec" in _lib.EXPORTS


class _Args:
    """A well-formed argument set in explicit-points mode (host addresses standing in for device ones:
    every call below must return before anything is launched), with fields replaced per case."""

    def __init__(self):
        self.buf = (ctypes.c_float * 64)()
        p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.p = p
        self.m = (ctypes.c_int64 * 2)(4, 4)
        self.grids = (ctypes.c_void_p * 2)(p.value, p.value)
        self.kw = dict(dtype=F32, ndim=2, m=None, grids=None, x=p, nobs=2, omega=p, phase=p, nfeat=3, w=p, nw=2,
                       scale=1.0, transposed=0, beta=0.0, nsplit=0, out=p)

    def mesh(self):
        return dict(x=None, m=self.m, grids=self.grids, nobs=0)

    def call(self, L, **over):
        a = dict(self.kw, **over)
        return L.hgp_rff_matvec(a["dtype"], a["ndim"], a["m"], a["grids"], a["x"], a["nobs"], a["omega"], a["phase"],
                                a["nfeat"], a["w"], a["nw"], a["scale"], a["transposed"], a["beta"], a["nsplit"],
                                a["out"], None)


def _bad_cases():
    a = _Args()
    null_grid = (ctypes.c_void_p * 2)(a.p.value, None)
    zero_m = (ctypes.c_int64 * 2)(4, 0)
    return [
        ("null_omega", dict(omega=None)), ("null_phase", dict(phase=None)), ("null_w", dict(w=None)),
        ("null_out", dict(out=None)), ("bad_dtype", dict(dtype=7)), ("ndim0", dict(ndim=0)), ("ndim4", dict(ndim=4)),
        ("negative_nobs", dict(nobs=-1)), ("negative_nfeat", dict(nfeat=-1)), ("negative_nw", dict(nw=-1)),
        ("negative_nsplit", dict(nsplit=-1)), ("nfeat0_with_points", dict(nfeat=0)),
        ("x_and_grids", dict(m=a.m, grids=a.grids)), ("neither_x_nor_grids", dict(x=None)),
        ("mesh_null_m", dict(a.mesh(), m=None)), ("mesh_null_grid", dict(a.mesh(), grids=null_grid)),
        ("mesh_size0", dict(a.mesh(), m=zero_m)), ("mesh_null_omega", dict(a.mesh(), omega=None)),
        ("mesh_nfeat0", dict(a.mesh(), nfeat=0)), ("mesh_null_out_transposed", dict(a.mesh(), out=None, transposed=1)),
    ]


BAD = _bad_cases()


@pytest.mark.parametrize("tag,over", BAD, ids=[c[0] for c in BAD])
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
    assert a.call(_lib.lib(), **dict(a.mesh(), nw=0, w=None)) == 0
    assert all(v == 3.0 for v in a.buf), "an empty product wrote something"


def test_fp32_feature_kernels_do_not_spill():
    ks = [k for k in _kernels() if re.search(r"hgp::k_rff_\w+<float", k[0])]
    assert sum("k_rff_mv<float" in k[0] for k in ks) == 3 and any("k_rff_finish<float" in k[0] for k in ks), ks
    bad = [f"{n} (spill {s}, scratch {p}, vgpr {v})" for n, s, p, v in ks if s or p]
    assert not bad, "fp32 feature kernels spilling to scratch:\n" + "\n".join(bad)
    assert all(v <= 64 for _, _, _, v in ks), ks          # 8 waves per SIMD


def test_wrapper_declines_cpu_tensors_and_checks_shapes():
    from hipgp_amd import rff
    om, ph, W = torch.ones(5, 2, dtype=torch.float64), torch.zeros(5, dtype=torch.float64), torch.ones(2, 5)
    assert rff.rff_matvec(om, ph, W, x=torch.zeros(3, 2)) is None
    assert rff.rff_matvec(om, ph, W, xgrids=[torch.linspace(0, 1, 4)] * 2) is None
    with pytest.raises(TypeError):
        rff.rff_matvec(om, ph, W)
    with pytest.raises(TypeError):
        rff.rff_matvec(om, ph, W, x=torch.zeros(3, 2), xgrids=[torch.linspace(0, 1, 4)] * 2)
    assert list(inspect.signature(rff.spectral_features).parameters) == ["kernel", "params", "ndim", "nfeat",
                                                                       "generator", "device", "dtype"]


# ---- the spectral sampler ---------------------------------------------------------------------
def _kernel_cases():
    import hipgp_amd.ziggy.kernels as zk
    dt = torch.float64
    return [("sqexp", zk.SqExp(dtype=dt)), ("matern12", zk.Matern(nu=.5, dtype=dt)),
            ("matern32", zk.Matern(nu=1.5, dtype=dt)), ("matern52", zk.Matern(nu=2.5, dtype=dt))]


@pytest.mark.parametrize("name", ["sqexp", "matern12", "matern32", "matern52"])
def test_spectral_features_reproduce_the_kernel(name):
    """(2 sig2 / F) sum_f cos(w.x + b) cos(w.y + b) is a mean of F terms bounded by 2 sig2 with
    expectation k(x, y): 10 sig2 / sqrt(F) is five standard deviations of that mean at the most."""
    from hipgp_amd import rff
    kernel = dict(_kernel_cases())[name]
    sig2, ell, F = 1.7, 0.3, 2 ** 14
    g = torch.Generator().manual_seed(1234)
    omega, phase = rff.spectral_features(kernel, (sig2, ell), 2, F, generator=g)
    assert tuple(omega.shape) == (F, 2) and tuple(phase.shape) == (F,) and omega.dtype == torch.float64
    assert float(phase.min()) >= 0 and float(phase.max()) < 2 * np.pi
    x = torch.rand(50, 2, generator=g, dtype=torch.float64)
    y = x + (torch.rand(50, 2, generator=g, dtype=torch.float64) - .5) * torch.linspace(0, 2, 50)[:, None]
    cx = torch.cos(x @ omega.t() + phase)
    cy = torch.cos(y @ omega.t() + phase)
    approx = (2 * sig2 / F) * torch.sum(cx * cy, dim=1)
    exact = torch.stack([kernel(x[i:i + 1], y[i:i + 1], (sig2, ell))[0, 0] for i in range(50)])
    err = float((approx - exact).abs().max())
    print(f"{name}: max |rff - k| = {err:.4f}, bound {10 * sig2 / np.sqrt(F):.4f}")
    assert err < 10 * sig2 / np.sqrt(F)
    # reproducible from the seed; a tensor ell of one element is a scalar
    o2, p2 = rff.spectral_features(kernel, (sig2, torch.tensor([ell], dtype=torch.float64)), 2, F,
                                   generator=torch.Generator().manual_seed(1234))
    assert torch.equal(o2, omega) and torch.equal(p2, phase)


def test_spectral_features_refuse_gneiting_and_ard():
    import hipgp_amd.ziggy.kernels as zk
    from hipgp_amd import rff
    with pytest.raises(NotImplementedError, match="Gneiting"):
        rff.spectral_features(zk.Gneiting(dtype=torch.float64), (1., .3), 2, 16)
    with pytest.raises(NotImplementedError, match="SqExp"):
        rff.spectral_features(zk.SqExp(dtype=torch.float64), (1., torch.tensor([.3, .4])), 2, 16)


# ---- predict_samples on the oracle stand-in ------------------------------------------------------
class FullKmm(SolvingKmm):
    """`SolvingKmm` with the R^T that `predict` needs."""

    def _matmul_by_RT(self, v):
        return torch.from_numpy(self.O.matmul_RT(v.detach().numpy()).reshape(v.shape[0], -1))


def _dense_samples(mod, Kmm, R, x, eps, omega, phase, W, xi):
    """The five steps in NumPy: (n, N)."""
    sig2, _ = mod.get_kernel_params()
    F = omega.shape[0]
    s = np.sqrt(2 * float(sig2) / F)
    qm = mod.standard_variational_params()[0].detach().numpy().reshape(-1)
    U = mod.xinduce.numpy()
    prior = lambda p: s * np.cos(p @ omega.T + phase[None, :]) @ W.T                 # (points, n)
    V = qm[None, :] + eps @ _dense_S_half(mod).T
    u = R @ V.T                                                                      # (M, n)
    u_prior = prior(U) + np.sqrt(mod.jitter_val) * xi.T
    alpha = np.linalg.solve(Kmm.K, u - u_prior)
    Knm = mod.kernel(x, mod.xinduce, mod.get_kernel_params()).detach().numpy()
    return (prior(x.numpy()) + Knm @ alpha).T


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_predict_samples_match_the_dense_restatement(family):
    from hipgp_amd import rff
    mod, O = _model(family), _oracle()
    Kmm = SolvingKmm(O)
    R = dense_R(O)
    x = _points()
    n, F = 3, 37
    g = torch.Generator().manual_seed(8)
    dt = torch.float64
    eps = torch.randn(n, O.Mp, generator=g, dtype=dt)
    omega, phase = rff.spectral_features(mod.kernel, mod.get_kernel_params(), 2, F, generator=g)
    W = torch.randn(n, F, generator=g, dtype=dt)
    xi = torch.randn(n, O.M, generator=g, dtype=dt)
    keep = [t.clone() for t in (eps, omega, phase, W, xi)]
    ref = _dense_samples(mod, Kmm, R, x, eps.numpy(), omega.numpy(), phase.numpy(), W.numpy(), xi.numpy())
    kw = dict(eps=eps, features=(omega, phase), prior_w=W, nugget_eps=xi, Kmm=Kmm)
    d = mod.predict_samples(x, n, **kw)
    assert tuple(d.shape) == (n, 13) and d.device.type == "cpu" and not d.requires_grad
    assert all(torch.equal(a, b) for a, b in zip(keep, (eps, omega, phase, W, xi))), "a caller's input changed"
    assert Kmm.calls == [("R", (n, O.Mp)), ("solve", (n, O.M))]
    err = max_rel(d.numpy(), ref)
    print(f"{family}: predict_samples vs dense restatement {err:.2e}")
    assert err < 1e-9
    assert torch.equal(mod.predict_samples(x, n, **kw), d)
    # the same draws from a generator twice; shapes of given inputs are checked
    a = mod.predict_samples(x, 2, nfeat=16, generator=torch.Generator().manual_seed(3), Kmm=Kmm)
    b = mod.predict_samples(x, 2, nfeat=16, generator=torch.Generator().manual_seed(3), Kmm=Kmm)
    assert torch.equal(a, b) and tuple(a.shape) == (2, 13)
    for bad in (dict(prior_w=W[:, :-1]), dict(nugget_eps=xi[:, :-1]), dict(eps=eps[:, :-1]),
                dict(features=(omega[:, :1], phase))):
        with pytest.raises(ValueError):
            mod.predict_samples(x, n, **dict(kw, **bad))


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_predict_samples_refuse_cholesky_whitening_and_line_integrals(family):
    Kmm = SolvingKmm(_oracle())
    x = _points()
    with pytest.raises(NotImplementedError, match="cholesky whitening has no circulant R"):
        _model(family, whitened_type="cholesky").predict_samples(x, 2, nfeat=8, Kmm=Kmm)
    with pytest.raises(NotImplementedError, match="integrated_obs"):
        _model(family).predict_samples(x, 2, nfeat=8, Kmm=Kmm, integrated_obs=True)
    assert Kmm.calls == []


def test_predict_samples_have_predicts_mean_and_variance_where_predict_draws_do_not():
    """12 x 10 grid on [0, 1]^2, SqExp(1, 0.05), jitter 1e-3, F = 4096, 20 000 draws, at points where
    the residual ktilde is at least half of `predict`'s variance: the draws' variance over
    `predict`'s lies in [0.8, 1.25] and their mean within 0.05 sd of `predict`'s, while the projected
    draws of `predict_draws` have less than 0.6 of the variance."""
    import hipgp_amd.ziggy.hipgp as hg
    import hipgp_amd.ziggy.kernels as zk
    dt = torch.float64
    dims, ell, jit, F, n = (12, 10), .05, 1e-3, 4096, 20000
    grids = [np.linspace(0, 1, m) for m in dims]
    O = zo.ToeplitzOracle(zo.toeplitz_column(grids, lambda a, b: zo.kernel_eval("sqexp", a, b, (1., ell)), jit), dims)
    Kmm = FullKmm(O)
    torch.manual_seed(2)
    mod = hg.MeanFieldToeplitzGP(zk.SqExp(dtype=dt), [torch.tensor(g) for g in grids], num_obs=50, sig2_init=1.,
                                 ell_init=ell, noise2_init=.05, learn_kernel=False, dtype=dt, jitter_val=jit)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=dt))
        mod.global_theta2.copy_(-(torch.rand(mod.Mprime, 1, generator=g, dtype=dt) * 4 + 1))     # S in [0.1, 0.5]
    h0, h1 = 1 / 11, 1 / 9
    x = torch.tensor([[2.5 * h0, 3.5 * h1], [6.5 * h0, 0.5 * h1], [9.5 * h0, 7.5 * h1], [4.5 * h0, 5 * h1],
                      [7 * h0, 2.5 * h1], [-.06, .45], [1.07, 1.06]], dtype=dt)
    mu, sd = mod.predict(x, maxiter_cg=50, Kmm=Kmm)
    mu, var = mu.numpy().reshape(-1), sd.numpy().reshape(-1) ** 2
    proj_var = mod.predict_draws(x, n, generator=g, Kmm=Kmm).numpy().var(axis=0)
    Knm = mod.kernel(x, mod.xinduce, mod.get_kernel_params()).numpy()
    kn = O.matmul_RT(np.linalg.solve(Kmm.K, Knm.T).T).reshape(len(x), -1)
    ktilde = 1. - np.sum(kn * kn, axis=1)
    print("ktilde / predict variance:", np.round(ktilde / var, 3))
    assert np.all(ktilde >= .5 * var), ktilde / var
    draws = mod.predict_samples(x, n, nfeat=F, generator=g, Kmm=Kmm).numpy()
    ratio = draws.var(axis=0) / var
    shift = (draws.mean(axis=0) - mu) / np.sqrt(var)
    pratio = proj_var / var
    print("variance ratio:", np.round(ratio, 3), "mean shift / sd:", np.round(shift, 4), "projected:", np.round(pratio, 3))
    assert np.all((ratio >= .8) & (ratio <= 1.25)), ratio
    assert np.all(np.abs(shift) < .05), shift
    assert np.all(pratio < .6), pratio
