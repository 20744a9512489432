"""The fused Fourier-feature product (hgp_rff_matvec behind `hipgp_amd.rff.rff_matvec`) against the
same expression in torch fp64 on the device, and `predict_samples` on the device against a dense
restatement of pathwise conditioning.

The product's error is max |out - ref| over max |ref| of the fp64 reference
ref = beta * out0 + scale * cos(p omega^T + phase) W^T:
  fp64: at most 1e-12.
  fp32: at most 4 x the error of torch's own fp32 evaluation of the same expression on the same
        inputs against fp64, plus 1e-6 (the project's usual rule).
Shapes are the smallest at which the kernel can go wrong: 1 to 3 dimensions, a tile of 64 points
short by one, full, over by one and several tiles; one run of 256 features short by one, full, over
by one and several runs; weight rows below, at and above a group of 8; a forced split.
`predict_samples`: fp64 to 1e-7 of the restatement with PCG at maxiter_cg = 200; fp32 within 4 x the
error of the same model's `predict_draws` against its own restatement.
Each test prints its figures before it asserts."""
import functools
import itertools

import numpy as np
import pytest
import torch

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
    """beta * base + scale * cos(x omega^T + phase) W^T in the dtype of the inputs."""
    acc = scale * (torch.cos(x @ omega.t() + phase) @ W.t())
    if transposed:
        acc = acc.t()
    return acc if beta == 0 else beta * base + acc


@functools.lru_cache(maxsize=None)
def _inputs(ndim, nobs, nfeat, tag, ell=ELL):
    """Points in [0, 1]^ndim, omega ~ N(0, I / ell^2) and phase ~ U[0, 2 pi) in fp64, 9 weight rows
    and a tensor to accumulate into, in the test dtype; made once and shared, never changed."""
    dt = dtype_of(tag)
    g = torch.Generator(device="cpu").manual_seed(100 * ndim + nobs + 7 * nfeat)
    x = torch.rand(nobs, ndim, generator=g, dtype=dt).to(DEV)
    omega = (torch.randn(nfeat, ndim, generator=g, dtype=torch.float64) / ell).to(DEV)
    phase = (torch.rand(nfeat, generator=g, dtype=torch.float64) * 2 * np.pi).to(DEV)
    W = torch.randn(max(NWS), nfeat, generator=g, dtype=dt).to(DEV)
    base = torch.randn(nobs, max(NWS), generator=g, dtype=dt).to(DEV)
    return x, omega, phase, W, base


def _one(x, omega, phase, W, base, nw, ns, tr, beta, tag):
    """(error of the kernel, error of torch in the test dtype or None), both over max |ref|."""
    from hipgp_amd import rff
    dt = dtype_of(tag)
    b = base[:, :nw].t().contiguous() if tr else base[:, :nw].contiguous()
    out = b.clone() if beta else torch.full_like(b, float("nan"))
    res = rff.rff_matvec(omega, phase, W[:nw], x=x, scale=SCALE, transposed=tr, out=out, beta=beta, nsplit=ns)
    assert res is out and out.dtype == dt
    ref = _expr(x.double(), omega, phase, W[:nw].double(), SCALE, tr, b.double(), beta)
    top = float(ref.abs().max())
    err = float((out.double() - ref).abs().max()) / top
    e32 = None
    if tag == "f32":
        t32 = _expr(x, omega.to(dt), phase.to(dt), W[:nw], SCALE, tr, b, beta)
        e32 = float((t32.double() - ref).abs().max()) / top
    return err, e32


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_rff_matvec_matches_torch(ndim, tag):
    worst, worst32, fails = 0.0, 0.0, []
    for nobs, nfeat in itertools.product(NOBS, NFEAT):
        x, omega, phase, W, base = _inputs(ndim, nobs, nfeat, tag)
        for nw, ns, tr, beta in itertools.product(NWS, NSPLITS, (False, True), (0.0, 1.0)):
            err, e32 = _one(x, omega, phase, W, base, nw, ns, tr, beta, tag)
            bound = F64_BOUND if tag == "f64" else 4 * e32 + 1e-6
            worst, worst32 = max(worst, err), max(worst32, e32 or 0.0)
            if not err <= bound:
                fails.append((nobs, nfeat, nw, ns, tr, beta, err, bound))
    print(f"\nrff {ndim}-D {tag}: worst error / max |ref| = {worst:.3e}"
          + (f" (torch fp32 worst: {worst32:.3e})" if tag == "f32" else "") + f"; {len(fails)} cases over their bound")
    for f in fails[:20]:
        print("  (nobs, nfeat, nw, nsplit, transposed, beta, error, bound) =", f)
    assert not fails


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_rff_matvec_large_arguments(tag):
    """ell = 0.01 on [0, 1]^2: arguments of hundreds of radians, the range reduction's case."""
    x, omega, phase, W, base = _inputs(2, 200, 1000, tag, ell=0.01)
    top = float((x.double() @ omega.t() + phase).abs().max())
    assert top > 300
    for nw, ns in itertools.product(NWS, NSPLITS):
        err, e32 = _one(x, omega, phase, W, base, nw, ns, False, 0.0, tag)
        bound = F64_BOUND if tag == "f64" else 4 * e32 + 1e-6
        print(f"\nlarge arguments (max {top:.0f} rad) {tag} nw={nw} nsplit={ns}: error {err:.3e}"
              + ("" if e32 is None else f" (torch fp32: {e32:.3e})"))
        assert err <= bound


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("dims", [(7, 6), (6, 5, 4)], ids=["7x6", "6x5x4"])
def test_mesh_mode_equals_explicit_points_bit_for_bit(dims, tag):
    from hipgp_amd import rff
    dt = dtype_of(tag)
    grids = [torch.linspace(-.3, 1.1, m, dtype=dt, device=DEV) + .01 * a for a, m in enumerate(dims)]
    mesh = torch.stack([a.reshape(-1) for a in torch.meshgrid(*grids, indexing="ij")], dim=-1).contiguous()
    _, omega, phase, W, _ = _inputs(len(dims), 65, 257, tag)
    for ns, tr in itertools.product(NSPLITS, (False, True)):
        a = rff.rff_matvec(omega, phase, W, xgrids=grids, scale=SCALE, transposed=tr, nsplit=ns)
        b = rff.rff_matvec(omega, phase, W, x=mesh, scale=SCALE, transposed=tr, nsplit=ns)
        assert tuple(a.shape) == ((9, mesh.shape[0]) if tr else (mesh.shape[0], 9))
        assert torch.equal(a, b), (dims, tag, ns, tr)
        # accumulated in place on the same start: the same bits too
        start = torch.randn(a.shape, generator=torch.Generator().manual_seed(1), dtype=dt).to(DEV)
        a1 = rff.rff_matvec(omega, phase, W, xgrids=grids, scale=-SCALE, transposed=tr, nsplit=ns, out=start.clone(),
                            beta=1.0)
        b1 = rff.rff_matvec(omega, phase, W, x=mesh, scale=-SCALE, transposed=tr, nsplit=ns, out=start.clone(), beta=1.0)
        assert torch.equal(a1, b1)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_two_calls_are_bit_equal(tag):
    from hipgp_amd import rff
    x, omega, phase, W, _ = _inputs(2, 200, 1000, tag)
    for ns, tr in itertools.product(NSPLITS, (False, True)):
        a = rff.rff_matvec(omega, phase, W, x=x, scale=SCALE, transposed=tr, nsplit=ns)
        b = rff.rff_matvec(omega, phase, W, x=x, scale=SCALE, transposed=tr, nsplit=ns)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (tag, ns, tr)


def test_empty_products_and_shape_checks():
    from hipgp_amd import rff
    x, omega, phase, W, _ = _inputs(2, 65, 257, "f32")
    assert tuple(rff.rff_matvec(omega, phase, W, x=x[:0]).shape) == (0, 9)
    assert tuple(rff.rff_matvec(omega, phase, W[:0], x=x).shape) == (65, 0)
    assert tuple(rff.rff_matvec(omega, phase, W[0], x=x, transposed=True).shape) == (1, 65)
    with pytest.raises(ValueError):
        rff.rff_matvec(omega, phase, W[:, :-1], x=x)
    with pytest.raises(ValueError):
        rff.rff_matvec(omega, phase, W, x=x, beta=1.0)
    with pytest.raises(ValueError):
        rff.rff_matvec(omega, phase, W, x=x, out=torch.empty(9, 65, device=DEV))


# ---- predict_samples on the device ------------------------------------------------------------------
MDIMS = (24, 20)
NPTS, NDRAW, NF = 37, 3, 300
MAXITER = 200


def _model(family, dt):
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    grids = [torch.linspace(-1, 1, m, dtype=dt) for m in MDIMS]
    torch.manual_seed(5)
    kw = dict(num_obs=64, sig2_init=1., ell_init=.3, noise2_init=.05, learn_kernel=False, dtype=dt)
    g = torch.Generator().manual_seed(11)
    k = zk.Matern(nu=1.5, dtype=dt)
    d64 = torch.float64
    if family == "block":
        mod = hg.BlockToeplitzGP(k, grids, block_sizes=[2, 2], **kw)
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


@functools.lru_cache(maxsize=None)
def _dense(family):
    """The fp64 model on the device, its random inputs, and the dense restatements of
    `predict_samples` (the five steps) and `predict_draws`, (n, N) each; made once."""
    from hipgp_amd import rff
    d64 = torch.float64
    mod = _model(family, d64)
    g = torch.Generator(device="cpu").manual_seed(6)
    x = (torch.rand(NPTS, 2, generator=g, dtype=d64) * 2.2 - 1.1).float().double().to(DEV)
    eps = torch.randn(NDRAW, mod.Mprime, generator=g).double().to(DEV)            # fp32 values: exact in both
    W = torch.randn(NDRAW, NF, generator=g).double().to(DEV)
    xi = torch.randn(NDRAW, mod.M, generator=g).double().to(DEV)
    params = mod.get_kernel_params()
    omega, phase = rff.spectral_features(mod.kernel, params, 2, NF, generator=g, device=DEV)
    with torch.no_grad():
        T = mod.toeplitz()
        T.set_batch_shape((mod.Mprime,))
        Rt = T._matmul_by_R(torch.eye(mod.Mprime, dtype=d64, device=DEV)).reshape(mod.Mprime, mod.M)   # R^T
        K = mod.kernel(mod.xinduce, mod.xinduce, params) + mod.jitter_val * torch.eye(mod.M, dtype=d64, device=DEV)
        Knm = mod.kernel(x, mod.xinduce, params)
        V = mod.variational_draws(NDRAW, eps=eps)
        u = V @ Rt                                                                   # (n, M)
        s = float(np.sqrt(2 * float(params[0]) / NF))
        prior = lambda p: s * (W @ torch.cos(p @ omega.t() + phase).t())            # (n, points)
        rhs = u - prior(mod.xinduce) - float(np.sqrt(mod.jitter_val)) * xi
        samples = prior(x) + torch.linalg.solve(K, rhs.t()).t() @ Knm.t()
        draws = torch.linalg.solve(K, u.t()).t() @ Knm.t()
    return dict(x=x, eps=eps, W=W, xi=xi, features=(omega, phase), samples=samples.cpu(), draws=draws.cpu())


def _gap(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_predict_samples_fp64_match_the_dense_restatement(family):
    c = _dense(family)
    mod = _model(family, torch.float64)
    d = mod.predict_samples(c["x"], NDRAW, eps=c["eps"], features=c["features"], prior_w=c["W"], nugget_eps=c["xi"],
                            maxiter_cg=MAXITER)
    assert tuple(d.shape) == (NDRAW, NPTS) and d.device.type == "cpu" and d.dtype == torch.float64
    gap = _gap(d, c["samples"])
    print(f"\n{family} fp64: predict_samples vs dense restatement {gap:.3e}")
    assert gap <= 1e-7
    again = mod.predict_samples(c["x"], NDRAW, eps=c["eps"], features=c["features"], prior_w=c["W"],
                                nugget_eps=c["xi"], maxiter_cg=MAXITER)
    assert torch.equal(d, again)


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_predict_samples_fp32_as_good_as_predict_draws(family):
    c = _dense(family)
    mod = _model(family, torch.float32)
    d = mod.predict_samples(c["x"], NDRAW, eps=c["eps"], features=c["features"], prior_w=c["W"], nugget_eps=c["xi"],
                            maxiter_cg=MAXITER)
    p = mod.predict_draws(c["x"].float(), NDRAW, eps=c["eps"], maxiter_cg=MAXITER)
    assert tuple(d.shape) == (NDRAW, NPTS) and d.dtype == torch.float32
    gs, gd = _gap(d, c["samples"]), _gap(p, c["draws"])
    print(f"\n{family} fp32: predict_samples vs restatement {gs:.3e}, predict_draws vs its restatement {gd:.3e}")
    assert gs <= 4 * gd
