"""The fused Kuf backward (hgp_kuf_grid_grad / hgp_kuf_semi_mc_grad / hgp_kuf_semi_sqexp_grad behind
`kuf_grid_ad` / `kuf_semi_mc_ad` / `kuf_semi_sqexp_ad`) against torch autograd through the broadcast
kernels of ziggy.kernels (`forward`, `k_semi_mc` with the same u, `k_semi`) in fp64 on the device.

Every error is measured relative to S = sum |G o dK/dtheta| of the fp64 reference, so a sum that
cancels (the random-sign G) does not inflate it.
  fp64: |error| <= 1e-10 S -- a cap from worst-case linear accumulation (at most 1e5 terms of a few
        operations each, 1.1e-16 apiece).  Measured worst case over the matrix: 2.2e-16 S (point
        observations), 3.4e-16 S (semi-mc).
  fp64, semi-sqexp: the Phi difference cancels, so no bound is fixed in advance: 10 x the worst
        case measured over this matrix.  Measured: see SEMI_SQEXP_F64_MEASURED.
  fp32: SURVEY §8(c) as tests/test_hyper_gpu.py applies it: no worse than 4 x the error of torch's
        own fp32 autograd on the same inputs, plus a 1e-5 S floor.
Each test prints its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch

from golden_cases import load, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

KERNELS = [("sqexp", None), ("matern", 0.5), ("matern", 1.5), ("matern", 2.5)]
GRIDS = [(300,), (1500,), (64, 48), (3, 1100), (17, 9, 5)]      # (1500,): two chunks with a tail
NOBS = 37
PARAMS = (1.3, 0.27)
F64_BOUND = 1e-10
SEMI_SQEXP_F64_MEASURED = 2.1e-15      # worst |error| / S of kuf_semi_sqexp_ad in fp64 over the matrix
SEMI_SQEXP_F64_BOUND = 10 * SEMI_SQEXP_F64_MEASURED
kid = lambda k: f"{k[0]}{k[1] or ''}"
did = lambda d: "x".join(map(str, d))


def _kern(kind, nu, dtype):
    import ziggy.kernels as zk
    return zk.SqExp(dtype=dtype) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dtype)


def _inputs(dims, dtype, semi, nobs=NOBS):
    """grids, x as test_kuf_matches_broadcast_kernel draws them, one observation moved onto a grid
    node (r = 0); for line integrals every endpoint has |x| >= 0.2 (the reference is NaN at 0)."""
    grids = [torch.linspace(-1, 1, m, dtype=dtype, device=DEV) for m in dims]
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.rand(nobs, len(dims), generator=g, dtype=dtype) * 2.4 - 1.2
    if semi:
        nrm = x.norm(dim=1, keepdim=True)
        x = torch.where(nrm < 0.25, x * (0.25 / nrm), x)
    x = x.to(DEV)
    if nobs > 3:
        x[3] = torch.stack([gr[len(gr) // 3] for gr in grids])
    return grids, x


def _mesh(grids):
    return torch.stack([a.reshape(-1) for a in torch.meshgrid(*grids, indexing="ij")], dim=-1)


def _upstream(nobs, M):
    g = torch.Generator(device="cpu").manual_seed(11)
    sign = (torch.randint(0, 2, (nobs, M), generator=g, dtype=torch.int64) * 2 - 1).double()
    return {"ones": torch.ones(nobs, M, dtype=torch.float64, device=DEV), "sign": sign.to(DEV)}


def _torch_K(entry, k, xs, x, params, npts, u):
    if entry == "grid":
        return k.forward(x, xs, params=params)
    if entry == "semi_mc":
        return k.k_semi_mc(xs, x, params, npts=npts, u=u).transpose(0, 1)
    return k.k_semi(xs, x, params).transpose(0, 1)


def ref_grads(fn, leaves, Gs):
    """fn(*leaves) -> K in fp64.  For every upstream G: torch autograd's gradients and
    S = sum |G o dK/dleaf| (the elementwise derivative is the gradient, with respect to the
    grad_outputs V, of autograd's own sum V . dK/dleaf)."""
    K = fn(*leaves)
    V = torch.ones_like(K, requires_grad=True)
    gv = torch.autograd.grad(K, leaves, grad_outputs=V, create_graph=True)
    D = [torch.autograd.grad(g, V, retain_graph=True)[0] for g in gv]
    out = {}
    for name, G in Gs.items():
        gr = torch.autograd.grad(K, leaves, grad_outputs=G.to(K.dtype), retain_graph=True)
        out[name] = (np.array([float(v) for v in gr]), np.array([float((G * d).abs().sum()) for d in D]))
    return out


@functools.lru_cache(maxsize=None)
def _case(entry, dims, kern, npts, tag):
    """Inputs in the test dtype, the fp64 reference on those same values, and (fp32) torch's own
    fp32 autograd; computed once and shared."""
    dtype = torch.float64 if tag == "f64" else torch.float32
    grids, x = _inputs(dims, dtype, semi=entry != "grid")
    u = torch.tensor([0.37], dtype=dtype, device=DEV)
    p = [torch.tensor(v, dtype=dtype, device=DEV) for v in PARAMS]
    M = int(np.prod(dims))
    Gs = _upstream(NOBS, M)
    xs64 = _mesh([g.double() for g in grids])
    leaves = [v.double().clone().requires_grad_(True) for v in p]
    k64 = _kern(*kern, torch.float64)
    ref = ref_grads(lambda s, e: _torch_K(entry, k64, xs64, x.double(), (s, e), npts, u.double()), leaves, Gs)
    t32 = None
    if tag == "f32":
        k32, xs32, t32 = _kern(*kern, dtype), _mesh(grids), {}
        for name, G in Gs.items():
            lv = [v.detach().clone().requires_grad_(True) for v in p]
            _torch_K(entry, k32, xs32, x, lv, npts, u).backward(G.float())
            t32[name] = np.array([float(v.grad) for v in lv])
    return dict(grids=grids, x=x, u=u, p=p, Gs=Gs, ref=ref, t32=t32, dtype=dtype)


def _ad(entry, k, grids, x, params, npts, u):
    from hipgp_amd import kuf
    if entry == "grid":
        return kuf.kuf_grid_ad(k, grids, x, params)
    if entry == "semi_mc":
        return kuf.kuf_semi_mc_ad(k, grids, x, params, npts, u=u)
    return kuf.kuf_semi_sqexp_ad(k, grids, x, params)


def _plain(entry, k, grids, x, params, npts, u):
    from hipgp_amd import kuf
    if entry == "grid":
        return kuf.kuf_grid(k, grids, x, params)
    if entry == "semi_mc":
        return kuf.kuf_semi_mc(k, grids, x, params, npts, u=u)
    return kuf.kuf_semi_sqexp(k, grids, x, params)


def grad_errors(entry, dims, kern, npts, tag):
    """[(G name, |error| / S per parameter, torch-fp32 |error| / S or None)] of the fused backward."""
    c = _case(entry, dims, kern, npts, tag)
    k = _kern(*kern, c["dtype"])
    out = []
    for name, G in c["Gs"].items():
        lv = [v.detach().clone().requires_grad_(True) for v in c["p"]]
        K = _ad(entry, k, c["grids"], c["x"], lv, npts, c["u"])
        assert K is not None and type(K.grad_fn).__name__ == "_KufADBackward"
        K.backward(G.to(c["dtype"]))
        mine = np.array([float(v.grad) for v in lv])
        g64, S = c["ref"][name]
        assert np.all(np.isfinite(g64)) and np.all(S > 0)
        e32 = None if c["t32"] is None else np.abs(c["t32"][name] - g64) / S
        out.append((name, np.abs(mine - g64) / S, e32))
    return out


def _check(entry, dims, kern, npts, tag, f64_bound):
    for name, e, e32 in grad_errors(entry, dims, kern, npts, tag):
        print(f"{entry} {did(dims)} {kid(kern)} npts={npts} {tag} G={name}: err/S (sig2, ell) = "
              f"{e[0]:.3e} {e[1]:.3e}" + ("" if e32 is None else f"  torch fp32: {e32[0]:.3e} {e32[1]:.3e}"))
        if tag == "f64":
            assert np.all(e <= f64_bound), (name, e)
        else:
            assert np.all(e <= 4 * e32 + 1e-5), (name, e, e32)


# ---- 1. per-entry gradients ----------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("kern", KERNELS, ids=kid)
@pytest.mark.parametrize("dims", GRIDS, ids=did)
def test_grid_grad_vs_autograd(dims, kern, tag):
    _check("grid", dims, kern, 0, tag, F64_BOUND)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("npts", [1, 7])
@pytest.mark.parametrize("kern", KERNELS, ids=kid)
@pytest.mark.parametrize("dims", GRIDS, ids=did)
def test_semi_mc_grad_vs_autograd(dims, kern, npts, tag):
    _check("semi_mc", dims, kern, npts, tag, F64_BOUND)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("dims", GRIDS, ids=did)
def test_semi_sqexp_grad_vs_autograd(dims, tag):
    _check("semi_sqexp", dims, KERNELS[0], 0, tag, SEMI_SQEXP_F64_BOUND)


# ---- 2. forward values ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("entry,kern,npts", [("grid", KERNELS[0], 0), ("grid", KERNELS[2], 0),
                                             ("semi_mc", KERNELS[3], 7), ("semi_sqexp", KERNELS[0], 0)],
                         ids=["grid-sqexp", "grid-matern1.5", "semi_mc-matern2.5", "semi_sqexp"])
def test_ad_forward_is_bitwise_the_plain_forward(entry, kern, npts, tag):
    dims = (64, 48)
    c = _case(entry, dims, kern, npts, tag)
    k = _kern(*kern, c["dtype"])
    lv = [v.detach().clone().requires_grad_(True) for v in c["p"]]
    K = _ad(entry, k, c["grids"], c["x"], lv, npts, c["u"])
    assert K.requires_grad
    with torch.no_grad():
        P = _plain(entry, k, c["grids"], c["x"], lv, npts, c["u"])
    assert P is not None and torch.equal(K.detach(), P)
    # no hyper-parameter asks for a gradient: the plain forward's result, no graph
    K0 = _ad(entry, k, c["grids"], c["x"], c["p"], npts, c["u"])
    assert not K0.requires_grad and torch.equal(K0, P)


# ---- 3. determinism ------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,kern,npts", [("grid", KERNELS[2], 0), ("semi_mc", KERNELS[0], 7),
                                             ("semi_sqexp", KERNELS[0], 0)], ids=["grid", "semi_mc", "semi_sqexp"])
def test_backward_is_bit_reproducible(entry, kern, npts):
    c = _case(entry, (64, 48), kern, npts, "f32")
    k = _kern(*kern, torch.float32)
    G = c["Gs"]["sign"].float()
    res = []
    for _ in range(2):
        lv = [v.detach().clone().requires_grad_(True) for v in c["p"]]
        _ad(entry, k, c["grids"], c["x"], lv, npts, c["u"]).backward(G)
        res.append(torch.stack([v.grad for v in lv]))
    assert torch.equal(res[0], res[1])


# ---- 4. edge cases -------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["grid", "semi_mc", "semi_sqexp"])
def test_no_observations_gives_zero_gradients(entry):
    k = _kern("sqexp", None, torch.float32)
    grids = [torch.linspace(-1, 1, 8, device=DEV)] * 2
    lv = [torch.tensor(v, device=DEV, requires_grad=True) for v in PARAMS]
    K = _ad(entry, k, grids, torch.zeros(0, 2, device=DEV), lv, 3, torch.tensor([0.5], device=DEV))
    assert K.shape == (0, 64)
    K.sum().backward()
    assert float(lv[0].grad) == 0. and float(lv[1].grad) == 0.


def test_ad_declines_x_grad_and_gneiting():
    import ziggy.kernels as zk
    from hipgp_amd import kuf
    grids = [torch.linspace(-1, 1, 8, device=DEV)] * 2
    ell = torch.tensor(0.3, device=DEV, requires_grad=True)
    k = _kern("sqexp", None, torch.float32)
    xg = torch.full((3, 2), 0.4, device=DEV, requires_grad=True)
    assert kuf.kuf_grid_ad(k, grids, xg, (1.0, ell)) is None
    assert kuf.kuf_semi_mc_ad(k, grids, xg, (1.0, ell), 4) is None
    assert kuf.kuf_semi_sqexp_ad(k, grids, xg, (1.0, ell)) is None
    x = xg.detach()
    gn = zk.Gneiting(dtype=torch.float32)
    assert kuf.kuf_grid_ad(gn, grids, x, (1.0, ell)) is None
    assert kuf.kuf_semi_mc_ad(gn, grids, x, (1.0, ell), 4) is None
    assert kuf.kuf_semi_sqexp_ad(_kern("matern", 1.5, torch.float32), grids, x, (1.0, ell)) is None
    assert kuf.kuf_grid_ad(k, grids, x, (1.0, torch.tensor([0.3, 0.4], device=DEV, requires_grad=True))) is None
    assert kuf.kuf_grid(k, grids, x, (1.0, ell)) is None          # the plain entry still declines


def test_knn_doubly_diag_ad_equals_the_kernel():
    from hipgp_amd.kuf import knn_doubly_diag, knn_doubly_diag_ad
    g = torch.Generator().manual_seed(3)
    N = 9
    grid = torch.linspace(0, 4., N, dtype=torch.float64)
    knn = torch.rand(N, generator=g, dtype=torch.float64)
    tab = torch.stack([grid, knn, torch.cat([(knn[1:] - knn[:-1]) / 0.5, torch.zeros(1, dtype=torch.float64)])]).to(DEV)
    x = (torch.rand(11, 2, generator=g, dtype=torch.float64) * 1.6).to(DEV)
    x[0] = 0.
    a = knn_doubly_diag_ad(tab, x, (torch.tensor(1.3, dtype=torch.float64, device=DEV), 0.7))
    b = knn_doubly_diag(tab, x, (1.3, 0.7))
    assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-14


# ---- 5. memory -----------------------------------------------------------------------------------
def test_make_grams_keeps_only_Knm():
    import ziggy.hipgp as hg
    dt, B, m = torch.float32, 64, 256
    grids = [torch.linspace(-1, 1, m, dtype=dt) for _ in range(2)]
    mod = hg.MeanFieldToeplitzGP(_kern("sqexp", None, dt), grids, num_obs=B, sig2_init=1.3, ell_init=.05,
                                 noise2_init=.01, learn_kernel=True, learn_noise=False, dtype=dt).cuda_params(0)
    mod.kuf_grad = True
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(B, 2, generator=g) * 2 - 1).to(DEV)
    G = torch.randn(B, m * m, generator=g).to(DEV)
    for measured in (False, True):        # the first round warms up (library load, the .grad buffers)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        Knm, _ = mod._make_grams(x)
        assert type(Knm.grad_fn).__name__ == "_KufADBackward"
        Knm.backward(G)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del Knm
    knm_bytes = B * m * m * 4
    print(f"peak above the level before the call: {peak} bytes = {peak / knm_bytes:.4f} x Knm ({knm_bytes} bytes)")
    assert peak <= 1.25 * knm_bytes, (peak, knm_bytes)
    assert torch.isfinite(mod.log_ell.grad) and float(mod.log_ell.grad) != 0.


# ---- 6. end to end -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["G16", "G17"], ids=["mean_field", "block"])
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_elbo_hyper_grads_with_kuf_grad(name, tag):
    """test_hyper_gpu.test_elbo_hyper_grads_vs_reference with the knob on: the same fixtures, model and
    bounds."""
    from test_hyper_gpu import HYPER, _hyper, _model
    dtype = torch.float64 if tag == "f64" else torch.float32
    fx, f64 = load(name, tag), load(name, "f64")
    mod = _model(fx, name, dtype)
    mod.kuf_grad = True
    x = torch.tensor(fx["xobs"], device=DEV)
    y = torch.tensor(fx["yobs"], device=DEV)
    assert type(mod._make_grams(x)[0].grad_fn).__name__ == "_KufADBackward"
    elbo = mod.elbo_and_grad(x, y, maxiter_cg=20)
    assert elbo.requires_grad
    elbo.backward()
    g = _hyper(mod)
    ref64 = np.array([float(f64[k]) for k in HYPER])
    print(f"{name} {tag}: elbo {float(elbo.detach())!r} hyper grads {g} reference fp64 {ref64}")
    if tag == "f64":
        assert abs(float(elbo) - float(fx["elbo"])) < 1e-8 * abs(float(fx["elbo"]))
        assert rel_err(mod.global_theta1.grad.cpu().numpy(), fx["theta1_grad"]) < 1e-7
        assert rel_err(mod.global_theta2.grad.cpu().numpy(), fx["theta2_grad"]) < 1e-7
        assert np.all(np.abs(g - ref64) <= 1e-6 * np.abs(ref64) + 1e-9), (g, ref64)
    else:
        ref32 = np.array([float(fx[k]) for k in HYPER])
        e_me, e_ref = np.abs(g - ref64), np.abs(ref32 - ref64)
        assert np.all(e_me <= 4 * e_ref + 1e-5 * np.abs(ref64)), (g, ref32, ref64)
        assert abs(float(elbo) - float(f64["elbo"])) < 1e-4 * abs(float(f64["elbo"]))


@pytest.mark.parametrize("estimator", ["analytic", "mc-biased"])
def test_integrated_grams_carry_the_graph(estimator):
    """(12, 10) grid, B = 6, SqExp, fp64: d/dlog_sig2 and d/dlog_ell of <G, Knm> + <w, Knn_diag> from
    `_make_grams(integrated_obs=True)` with the knob on, against the torch mirrors k_semi / k_semi_mc
    and the doubly-integrated table formula in torch, to the bounds of item 1."""
    import ziggy.hipgp as hg
    dt, B, npts = torch.float64, 6, 7
    k = _kern("sqexp", None, dt)
    grids = [torch.linspace(-1, 1, m, dtype=dt) for m in (12, 10)]
    mod = hg.MeanFieldToeplitzGP(k, grids, num_obs=B, sig2_init=1.3, ell_init=.27, noise2_init=.01,
                                 learn_kernel=True, learn_noise=False, dtype=dt).cuda_params(0)
    mod.kuf_grad = True
    _, x = _inputs((12, 10), dt, semi=True, nobs=B)
    g = torch.Generator().manual_seed(7)
    G = torch.randn(B, 120, generator=g, dtype=dt).to(DEV)
    w = torch.randn(B, generator=g, dtype=dt).to(DEV)
    u = torch.tensor([0.37], dtype=dt, device=DEV)
    Knm, Knn = mod._make_grams(x, integrated_obs=True, semi_integrated_estimator=estimator,
                               semi_integrated_samps=npts, mc_offset=u)
    assert type(Knm.grad_fn).__name__ == "_KufADBackward" and Knn.requires_grad
    ((Knm * G).sum() + (Knn * w).sum()).backward()
    mine = np.array([float(mod.log_sig2.grad), float(mod.log_ell.grad)])

    leaves = [mod.log_sig2.detach().clone().requires_grad_(True), mod.log_ell.detach().clone().requires_grad_(True)]
    entry = "semi_sqexp" if estimator == "analytic" else "semi_mc"
    r1 = ref_grads(lambda a, b: _torch_K(entry, k, mod.xinduce, x, (torch.exp(a), torch.exp(b)), npts, u),
                   leaves, {"G": G})["G"]
    tgrid, tknn, tslopes = k.diag_interp.table(x.device, dt)

    def knn_ref(a, b):
        sig2, ell = torch.exp(a), torch.exp(b)
        dists = torch.sqrt(torch.sum((x / ell) ** 2, dim=-1))
        lo = torch.sum(dists[:, None] > tgrid, dim=-1) - 1
        return ell * ell * sig2 * (tknn[lo] + tslopes[lo] * (dists - tgrid[lo]))
    r2 = ref_grads(knn_ref, leaves, {"w": w})["w"]
    ref = r1[0] + r2[0]
    bound = (SEMI_SQEXP_F64_BOUND if estimator == "analytic" else F64_BOUND) * r1[1] + F64_BOUND * r2[1]
    print(f"{estimator}: grads {mine} reference {ref} |error| {np.abs(mine - ref)} bound {bound}")
    assert np.all(r2[1] > 0) and np.all(np.abs(mine - ref) <= bound), (mine, ref, bound)
