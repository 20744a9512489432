"""The fused line-integral feature product (hgp_rff_line_matvec behind
`hipgp_amd.rff.rff_line_matvec`) against the closed form in torch fp64 on the device
(`rff.line_features`, which tests/test_rff_line_cpu.py holds to a quadrature), and
`predict_line_samples` on the device against a dense restatement.

The product's error is max |out - ref| over max |ref| of the fp64 reference
ref = beta * out0 + scale * L W^T, L[i, f] = |x_i| cos(b_f + T / 2) sinc(T / 2), T = omega_f . x_i:
  fp64: at most 1e-12, the bound tests/test_rff_gpu.py holds the point kernel to.
  fp32: at most 4 x the error of torch's own fp32 evaluation of the same closed form on the same
        inputs against fp64, plus 1e-6 (the project's 4 x rule as DESIGN section 4 states it and
        tests/test_rff_gpu.py applies it).
Shapes as there: 1 to 3 dimensions, a tile of 64 lines short by one, full, over by one and several
tiles; one run of 256 features short by one, full, over by one and several runs; weight rows below,
at and above a group of 8; a forced split.  In every case the last rows and features are the
special ones of `rff_line_cases` as far as they fit: the row x_s and the row x = 0; omega . x_s = 0
exactly, then |omega . x_s| = 1e-9, 1e-3, 0.2499, 0.2501 (both signs) and 500.3 revolutions.
`predict_line_samples`: fp64 to 1e-7 of the restatement with PCG at maxiter_cg = 200; fp32 within
4 x the error of the same model's `predict_draws(integrated_obs=True)` against its own restatement;
with xpoint the point rows are bit-equal to `predict_samples`.
Each test prints its figures before it asserts."""
import functools
import itertools

import numpy as np
import pytest
import torch

from rff_line_cases import with_specials

pytestmark = pytest.mark.gpu
DEV = "cuda"

NOBS = (1, 63, 64, 65, 200)
NFEAT = (1, 255, 256, 257, 1000)
NWS = (1, 8, 9)
NSPLITS = (0, 1, 3)
ELL = 0.3
SCALE = 0.37
F64_BOUND = 1e-12
dtype_of = lambda tag: torch.float64 if tag == "f64" else torch.float32


def _expr(x, omega, phase, W, scale, transposed, base, beta):
    """beta * base + scale * L W^T in the dtype of the inputs."""
    from hipgp_amd import rff
    acc = scale * (rff.line_features(omega, phase, x) @ W.t())
    if transposed:
        acc = acc.t()
    return acc if beta == 0 else beta * base + acc


@functools.lru_cache(maxsize=None)
def _inputs(ndim, nobs, nfeat, tag):
    """Rows in [-0.8, 0.8]^ndim, omega ~ N(0, I / ell^2) and phase ~ U[0, 2 pi) in fp64, the special rows
    and features last, 9 weight rows and a tensor to accumulate into, in the test dtype; made once
    and shared, never changed."""
    dt = dtype_of(tag)
    g = torch.Generator(device="cpu").manual_seed(100 * ndim + nobs + 7 * nfeat)
    x = torch.rand(nobs, ndim, generator=g, dtype=torch.float64) * 1.6 - .8
    omega = torch.randn(nfeat, ndim, generator=g, dtype=torch.float64) / ELL
    x, omega = with_specials(x, omega, ndim)
    phase = (torch.rand(nfeat, generator=g, dtype=torch.float64) * 2 * np.pi).to(DEV)
    W = torch.randn(max(NWS), nfeat, generator=g, dtype=dt).to(DEV)
    base = torch.randn(nobs, max(NWS), generator=g, dtype=dt).to(DEV)
    return x.to(dt).to(DEV), omega.to(DEV), phase, W, base


def _one(x, omega, phase, W, base, nw, ns, tr, beta, tag):
    """(error of the kernel, error of torch in the test dtype or None, the kernel's result)."""
    from hipgp_amd import rff
    dt = dtype_of(tag)
    b = base[:, :nw].t().contiguous() if tr else base[:, :nw].contiguous()
    out = b.clone() if beta else torch.full_like(b, float("nan"))
    res = rff.rff_line_matvec(omega, phase, W[:nw], x, scale=SCALE, transposed=tr, out=out, beta=beta, nsplit=ns)
    assert res is out and out.dtype == dt
    ref = _expr(x.double(), omega, phase, W[:nw].double(), SCALE, tr, b.double(), beta)
    top = float(ref.abs().max())
    err = float((out.double() - ref).abs().max()) / top
    e32 = None
    if tag == "f32":
        t32 = _expr(x, omega.to(dt), phase.to(dt), W[:nw], SCALE, tr, b, beta)
        e32 = float((t32.double() - ref).abs().max()) / top
    return err, e32, out


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_rff_line_matvec_matches_the_closed_form(ndim, tag):
    worst, worst32, fails = 0.0, 0.0, []
    for nobs, nfeat in itertools.product(NOBS, NFEAT):
        x, omega, phase, W, base = _inputs(ndim, nobs, nfeat, tag)
        for nw, ns, tr, beta in itertools.product(NWS, NSPLITS, (False, True), (0.0, 1.0)):
            err, e32, _ = _one(x, omega, phase, W, base, nw, ns, tr, beta, tag)
            bound = F64_BOUND if tag == "f64" else 4 * e32 + 1e-6
            worst, worst32 = max(worst, err), max(worst32, e32 or 0.0)
            if not err <= bound:
                fails.append((nobs, nfeat, nw, ns, tr, beta, err, bound))
    print(f"\nrff line {ndim}-D {tag}: worst error / max |ref| = {worst:.3e}"
          + (f" (torch fp32 worst: {worst32:.3e})" if tag == "f32" else "") + f"; {len(fails)} cases over their bound")
    for f in fails[:20]:
        print("  (nobs, nfeat, nw, nsplit, transposed, beta, error, bound) =", f)
    assert not fails


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_zero_rows_are_exactly_zero_reruns_bit_equal_and_splits_agree(tag):
    """The row x = 0 (the last one) gives exactly 0 in every layout and split; two calls give the same
    bits; a forced nsplit of 1 against 3 adds the SAME F = 1000 terms in another order (fp32 also cuts
    its 256-feature runs elsewhere), so element by element the two differ by at most twice the
    a-priori bound of a sum of F terms plus the rounding of the result, 2 (F + 2) u sum_f |term_f|,
    u = 2^-53 in fp64 (the rounding of fp64 sums) and 2^-24 in fp32."""
    from hipgp_amd import rff
    for ndim in (1, 2, 3):
        x, omega, phase, W, _ = _inputs(ndim, 200, 1000, tag)
        assert not x[-1].any()
        got = {}
        for ns, tr in itertools.product(NSPLITS, (False, True)):
            a = rff.rff_line_matvec(omega, phase, W, x, scale=SCALE, transposed=tr, nsplit=ns)
            b = rff.rff_line_matvec(omega, phase, W, x, scale=SCALE, transposed=tr, nsplit=ns)
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (tag, ndim, ns, tr)
            zero = a[:, -1] if tr else a[-1]
            assert not zero.any(), (tag, ndim, ns, tr, zero)
            got[ns, tr] = a
        diff = (got[1, False].double() - got[3, False].double()).abs()
        terms = SCALE * (rff.line_features(omega, phase, x.double()).abs() @ W.double().abs().t())
        allowed = 2 * (omega.shape[0] + 2) * (2.0 ** -53 if tag == "f64" else 2.0 ** -24) * terms
        print(f"\n{ndim}-D {tag}: nsplit 1 against 3 differ by {float(diff.max() / got[1, False].abs().max()):.3e} of "
              f"max |out|, at most {float((diff[:-1] / allowed[:-1]).max()):.3f} of the allowed difference")
        assert bool((diff <= allowed).all())
        assert torch.equal(got[1, False], got[1, True].t()) and torch.equal(got[3, False], got[3, True].t())


def test_empty_products_and_shape_checks():
    from hipgp_amd import rff
    x, omega, phase, W, _ = _inputs(2, 65, 257, "f32")
    assert tuple(rff.rff_line_matvec(omega, phase, W, x[:0]).shape) == (0, 9)
    assert tuple(rff.rff_line_matvec(omega, phase, W[:0], x).shape) == (65, 0)
    assert tuple(rff.rff_line_matvec(omega, phase, W[0], x, transposed=True).shape) == (1, 65)
    with pytest.raises(ValueError):
        rff.rff_line_matvec(omega, phase, W[:, :-1], x)
    with pytest.raises(ValueError):
        rff.rff_line_matvec(omega, phase, W, x, beta=1.0)
    with pytest.raises(ValueError):
        rff.rff_line_matvec(omega, phase, W, x, out=torch.empty(9, 65, device=DEV))
    with pytest.raises(ValueError):
        rff.rff_line_matvec(omega, phase, W, x[:, :1])


# ---- predict_line_samples on the device -------------------------------------------------------------
NLINES, NPOINT, NDRAW, NF = 37, 11, 3, 300
MAXITER = 200
CASES = {"sqexp-24x20": ((24, 20), "analytic"), "matern52-6x5x4": ((6, 5, 4), "mc-biased")}
NPTS_MC, U_MC = 7, 0.3


def _model(case, family, dt):
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    dims, _ = CASES[case]
    grids = [torch.linspace(-1, 1, m, dtype=dt) for m in dims]
    torch.manual_seed(5)
    kw = dict(num_obs=64, sig2_init=1., ell_init=.3, noise2_init=.05, learn_kernel=False, dtype=dt)
    g = torch.Generator().manual_seed(11)
    k = zk.SqExp(dtype=dt) if case.startswith("sqexp") else zk.Matern(nu=2.5, dtype=dt)
    d64 = torch.float64
    if family == "block":
        mod = hg.BlockToeplitzGP(k, grids, block_sizes=[2] * len(dims), **kw)
        with torch.no_grad():
            A = torch.randn(mod.num_blocks, mod.block_size, mod.block_size, generator=g, dtype=d64) * .5
            mod.global_theta2.copy_(-.5 * (A.matmul(A.transpose(1, 2)) + torch.eye(mod.block_size, dtype=d64)))
    else:
        mod = hg.MeanFieldToeplitzGP(k, grids, **kw)
        with torch.no_grad():
            mod.global_theta2.copy_(-(torch.rand(mod.Mprime, 1, generator=g, dtype=d64) * 4 + .5))
    with torch.no_grad():
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=d64))
    return mod.cuda_params(0)


def _route(case, dt):
    if CASES[case][1] == "analytic":
        return dict(semi_integrated_estimator="analytic")
    return dict(semi_integrated_estimator="mc-biased", semi_integrated_samps=NPTS_MC,
                mc_offset=torch.tensor([U_MC], dtype=dt, device=DEV))


@functools.lru_cache(maxsize=None)
def _dense(case, family):
    """The fp64 model on the device, its random inputs, and the dense restatements of
    `predict_line_samples` (lines and points) and `predict_draws(integrated_obs=True)`; made once."""
    from hipgp_amd import rff
    d64 = torch.float64
    mod = _model(case, family, d64)
    nd = len(CASES[case][0])
    g = torch.Generator(device="cpu").manual_seed(6)
    x = (torch.rand(NLINES, nd, generator=g, dtype=d64) * 2.2 - 1.1).float().double().to(DEV)
    xpoint = (torch.rand(NPOINT, nd, generator=g, dtype=d64) * 2.2 - 1.1).float().double().to(DEV)
    eps = torch.randn(NDRAW, mod.Mprime, generator=g).double().to(DEV)            # fp32 values: exact in both
    W = torch.randn(NDRAW, NF, generator=g).double().to(DEV)
    xi = torch.randn(NDRAW, mod.M, generator=g).double().to(DEV)
    params = mod.get_kernel_params()
    omega, phase = rff.spectral_features(mod.kernel, params, nd, NF, generator=g, device=DEV)
    with torch.no_grad():
        T = mod.toeplitz()
        T.set_batch_shape((mod.Mprime,))
        Rt = T._matmul_by_R(torch.eye(mod.Mprime, dtype=d64, device=DEV)).reshape(mod.Mprime, mod.M)   # R^T
        K = mod.kernel(mod.xinduce, mod.xinduce, params) + mod.jitter_val * torch.eye(mod.M, dtype=d64, device=DEV)
        if CASES[case][1] == "analytic":
            Ksemi = mod.kernel.k_semi(mod.xinduce, x, params).t()                    # (N, M)
        else:
            Ksemi = mod.kernel.k_semi_mc(mod.xinduce, x, params, npts=NPTS_MC,
                                         u=torch.tensor([U_MC], dtype=d64, device=DEV)).t()
        Knm = mod.kernel(xpoint, mod.xinduce, params)
        V = mod.variational_draws(NDRAW, eps=eps)
        u = V @ Rt                                                                   # (n, M)
        s = float(np.sqrt(2 * float(params[0]) / NF))
        prior = lambda p: s * (W @ torch.cos(p @ omega.t() + phase).t())            # (n, points)
        rhs = u - prior(mod.xinduce) - float(np.sqrt(mod.jitter_val)) * xi
        alpha = torch.linalg.solve(K, rhs.t()).t()
        lines = s * (W @ rff.line_features(omega, phase, x).t()) + alpha @ Ksemi.t()
        points = prior(xpoint) + alpha @ Knm.t()
        draws = torch.linalg.solve(K, u.t()).t() @ Ksemi.t()
    return dict(x=x, xpoint=xpoint, eps=eps, W=W, xi=xi, features=(omega, phase), lines=lines.cpu(),
                points=points.cpu(), draws=draws.cpu())


def _gap(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("family", ["mean-field", "block"])
@pytest.mark.parametrize("case", list(CASES))
def test_predict_line_samples_fp64_match_the_dense_restatement(case, family):
    c = _dense(case, family)
    mod = _model(case, family, torch.float64)
    kw = dict(eps=c["eps"], features=c["features"], prior_w=c["W"], nugget_eps=c["xi"], maxiter_cg=MAXITER)
    d = mod.predict_line_samples(c["x"], NDRAW, **kw, **_route(case, torch.float64))
    assert tuple(d.shape) == (NDRAW, NLINES) and d.device.type == "cpu" and d.dtype == torch.float64
    gap = _gap(d, c["lines"])
    print(f"\n{case} {family} fp64: predict_line_samples vs dense restatement {gap:.3e}")
    assert gap <= 1e-7
    dl, dp = mod.predict_line_samples(c["x"], NDRAW, xpoint=c["xpoint"], **kw, **_route(case, torch.float64))
    gp = _gap(dp, c["points"])
    print(f"{case} {family} fp64: point rows vs dense restatement {gp:.3e}")
    assert torch.equal(dl, d) and tuple(dp.shape) == (NDRAW, NPOINT) and gp <= 1e-7
    assert torch.equal(dp, mod.predict_samples(c["xpoint"], NDRAW, **kw))


@pytest.mark.parametrize("family", ["mean-field", "block"])
@pytest.mark.parametrize("case", list(CASES))
def test_predict_line_samples_fp32_as_good_as_predict_draws(case, family):
    c = _dense(case, family)
    dt = torch.float32
    mod = _model(case, family, dt)
    kw = dict(eps=c["eps"], features=c["features"], prior_w=c["W"], nugget_eps=c["xi"], maxiter_cg=MAXITER)
    d, dp = mod.predict_line_samples(c["x"], NDRAW, xpoint=c["xpoint"], **kw, **_route(case, dt))
    p = mod.predict_draws(c["x"].float(), NDRAW, eps=c["eps"], maxiter_cg=MAXITER, integrated_obs=True,
                          **_route(case, dt))
    assert tuple(d.shape) == (NDRAW, NLINES) and d.dtype == dt
    gs, gd = _gap(d, c["lines"]), _gap(p, c["draws"])
    print(f"\n{case} {family} fp32: predict_line_samples vs restatement {gs:.3e}, "
          f"predict_draws(integrated_obs=True) vs its restatement {gd:.3e}")
    assert gs <= 4 * gd
    assert torch.equal(dp, mod.predict_samples(c["xpoint"], NDRAW, **kw))
