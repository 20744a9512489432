"""The fused Kuf products (hgp_kuf_grid_matvec / hgp_kuf_semi_mc_matvec / hgp_kuf_semi_sqexp_matvec behind
`kuf_grid_matvec` / `kuf_semi_mc_matvec` / `kuf_semi_sqexp_matvec`) against the broadcast kernels of
ziggy.kernels (`forward`, `k_semi_mc` with the same u, `k_semi`) materialised in fp64 on the device
and multiplied by W^T, and the model methods on top of them (mean_weights / predict_mean /
predict_draws) against the materialised `predict` / `compute_kn`.

Every error of a product is measured relative to S[n, s] = sum_j |Kuf[n, j] w[s, j]| of the fp64
reference, so a sum that cancels (the random-sign W) does not inflate it.
  fp64: |error| <= 1e-10 S -- the cap of tests/test_kuf_grad_gpu.py from worst-case linear
        accumulation (at most 1e4 terms here of a few operations each, 1.1e-16 apiece).
  fp64, semi-sqexp: the Phi difference cancels, so no bound is fixed in advance: 10 x the worst
        case measured over this matrix, SEMI_SQEXP_F64_MEASURED.
  fp32: no worse than 4 x the error of torch's own fp32 Knm32 @ W32^T on the same inputs, plus a
        1e-5 S floor.
The model routes truncate different solves (one right-hand side R qm against one per point), so
their gap has no derivable bound: 10 x the worst relative gap measured over the cases
(MODEL_GAP_F64_MEASURED / MODEL_GAP_F32_MEASURED), with both PCGs at their break test.
Each test prints its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

KERNELS = [("sqexp", None), ("matern", 0.5), ("matern", 1.5), ("matern", 2.5)]
GRIDS = [(300,), (1500,), (64, 48), (3, 1100), (17, 9, 5)]
NOBS = 37
NOBS_TAIL = 700                 # point entry: 10 full tiles of 64 points and a tail of 60
NWS = (1, 3, 9)                 # 9: a group of 8 weight rows and a tail group
NSPLITS = (0, 1, 2, 7)
NPTS = 6
PARAMS = (1.3, 0.27)
F64_BOUND = 1e-10
SEMI_SQEXP_F64_MEASURED = 5.6e-15     # worst |error| / S of kuf_semi_sqexp_matvec in fp64 over the matrix
SEMI_SQEXP_F64_BOUND = 10 * SEMI_SQEXP_F64_MEASURED
MODEL_GAP_F64_MEASURED = 8.7e-9       # worst max|a - b| / max|b| of the model checks in fp64
MODEL_GAP_F32_MEASURED = 8.0e-5       # ... and in fp32
kid = lambda k: f"{k[0]}{k[1] or ''}"
did = lambda d: "x".join(map(str, d))


def _kern(kind, nu, dtype):
    import ziggy.kernels as zk
    if kind == "gneiting":
        return zk.Gneiting(dtype=dtype)
    return zk.SqExp(dtype=dtype) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dtype)


def _inputs(dims, dtype, semi, nobs):
    """grids on [-1, 1], x in [-1.2, 1.2]^d (some outside the grid's hull), one observation moved
    onto a grid node (r = 0); for line integrals every endpoint has |x| >= 0.25 (NaN at 0)."""
    grids = [torch.linspace(-1, 1, m, dtype=dtype, device=DEV) for m in dims]
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.rand(nobs, len(dims), generator=g, dtype=dtype) * 2.4 - 1.2
    if semi:
        nrm = x.norm(dim=1, keepdim=True)
        x = torch.where(nrm < 0.25, x * (0.25 / nrm), x)
    x = x.to(DEV)
    x[3] = torch.stack([gr[len(gr) // 3] for gr in grids])
    return grids, x


def _mesh(grids):
    return torch.stack([a.reshape(-1) for a in torch.meshgrid(*grids, indexing="ij")], dim=-1)


def _weights(M, dtype):
    """{name: (9, M)}: random signs times random magnitudes, and all ones; rows [:nw] are used."""
    g = torch.Generator(device="cpu").manual_seed(11)
    sign = (torch.randint(0, 2, (max(NWS), M), generator=g, dtype=torch.int64) * 2 - 1).to(dtype)
    mag = torch.rand(max(NWS), M, generator=g, dtype=dtype) + 0.5
    return {"sign": (sign * mag).to(DEV), "ones": torch.ones(max(NWS), M, dtype=dtype, device=DEV)}


def _torch_K(entry, k, xs, x, params, u):
    if entry == "grid":
        return k.forward(x, xs, params=params)
    if entry == "semi_mc":
        return k.k_semi_mc(xs, x, params, npts=NPTS, u=u).transpose(0, 1)
    return k.k_semi(xs, x, params).transpose(0, 1)


def _matvec(entry, k, grids, x, W, nsplit, u):
    from hipgp_amd import kuf
    if entry == "grid":
        return kuf.kuf_grid_matvec(k, grids, x, PARAMS, W, nsplit=nsplit)
    if entry == "semi_mc":
        return kuf.kuf_semi_mc_matvec(k, grids, x, PARAMS, NPTS, u=u, W=W, nsplit=nsplit)
    return kuf.kuf_semi_sqexp_matvec(k, grids, x, PARAMS, W, nsplit=nsplit)


@functools.lru_cache(maxsize=None)
def _case(entry, dims, kern, tag, nobs):
    """Inputs in the test dtype, the fp64 reference products and S on those same values, and (fp32)
    torch's own fp32 product; computed once and shared, never changed."""
    dtype = torch.float64 if tag == "f64" else torch.float32
    grids, x = _inputs(dims, dtype, entry != "grid", nobs)
    u = torch.tensor([0.37], dtype=dtype, device=DEV)
    Ws = _weights(int(np.prod(dims)), dtype)
    K64 = _torch_K(entry, _kern(*kern, torch.float64), _mesh([g.double() for g in grids]), x.double(), PARAMS,
                   u.double())
    assert bool(torch.isfinite(K64).all())
    ref = {n: (K64 @ W.double().t(), K64.abs() @ W.double().abs().t()) for n, W in Ws.items()}
    t32 = None
    if tag == "f32":
        K32 = _torch_K(entry, _kern(*kern, dtype), _mesh(grids), x, PARAMS, u)
        t32 = {n: (K32 @ W.t()).double() for n, W in Ws.items()}
    return dict(grids=grids, x=x, u=u, Ws=Ws, ref=ref, t32=t32, dtype=dtype)


def _errors(entry, dims, kern, tag, nobs=NOBS):
    """[(W name, nw, nsplit, max |error| / S, torch-fp32 max |error| / S or None)], and every output."""
    c = _case(entry, dims, kern, tag, nobs)
    k = _kern(*kern, c["dtype"])
    rows, outs = [], {}
    for name, W in c["Ws"].items():
        ref, S = c["ref"][name]
        assert bool((S > 0).all())
        for nw in NWS:
            e32 = None if c["t32"] is None else float(((c["t32"][name] - ref).abs() / S)[:, :nw].max())
            for ns in NSPLITS:
                out = _matvec(entry, k, c["grids"], c["x"], W[:nw], ns, c["u"])
                assert out is not None and tuple(out.shape) == (nobs, nw) and out.dtype == c["dtype"]
                outs[(name, nw, ns)] = out
                rows.append((name, nw, ns, float(((out.double() - ref[:, :nw]).abs() / S[:, :nw]).max()), e32))
    return rows, outs


def _check(entry, dims, kern, tag, f64_bound, nobs=NOBS):
    rows, outs = _errors(entry, dims, kern, tag, nobs)
    worst = max(r[3] for r in rows)
    w32 = max((r[4] for r in rows if r[4] is not None), default=None)
    print(f"\n{entry} {did(dims)} {kid(kern)} {tag} nobs={nobs}: worst |error|/S = {worst:.3e}"
          + ("" if w32 is None else f" (torch fp32 worst: {w32:.3e})"))
    for name, nw, ns, e, e32 in rows:
        bound = f64_bound if tag == "f64" else 4 * e32 + 1e-5
        assert e <= bound, (entry, dims, kern, tag, name, nw, ns, e, bound)
    # split invariance: every nsplit against nsplit = 1, relative to S, within the same bound
    c = _case(entry, dims, kern, tag, nobs)
    gap = 0.0
    for (name, nw, ns), out in outs.items():
        S = c["ref"][name][1][:, :nw]
        gap = max(gap, float(((out.double() - outs[(name, nw, 1)].double()).abs() / S).max()))
    lim = f64_bound if tag == "f64" else 4 * (w32 or 0.0) + 1e-5
    print(f"  split invariance: worst |out(nsplit) - out(1)| / S = {gap:.3e} (limit {lim:.1e})")
    assert gap <= lim
    return worst


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("kern", KERNELS, ids=kid)
@pytest.mark.parametrize("dims", GRIDS, ids=did)
def test_grid_matvec_matches_torch(dims, kern, tag):
    _check("grid", dims, kern, tag, F64_BOUND)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("kern", [KERNELS[0], KERNELS[2]], ids=kid)
@pytest.mark.parametrize("dims", [(1500,), (64, 48), (17, 9, 5)], ids=did)
def test_grid_matvec_with_a_tail_tile(dims, kern, tag):
    _check("grid", dims, kern, tag, F64_BOUND, nobs=NOBS_TAIL)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("kern", KERNELS + [("gneiting", None)], ids=kid)
@pytest.mark.parametrize("dims", GRIDS, ids=did)
def test_semi_mc_matvec_matches_torch(dims, kern, tag):
    _check("semi_mc", dims, kern, tag, F64_BOUND)


@pytest.mark.parametrize("dims", GRIDS, ids=did)
def test_semi_sqexp_matvec_matches_torch_fp32(dims):
    _check("semi_sqexp", dims, KERNELS[0], "f32", None)


def test_semi_sqexp_matvec_matches_torch_fp64():
    worst = max(_check("semi_sqexp", dims, KERNELS[0], "f64", SEMI_SQEXP_F64_BOUND) for dims in GRIDS)
    print(f"\nsemi-sqexp fp64 worst |error|/S over the matrix = {worst:.3e} "
          f"(SEMI_SQEXP_F64_MEASURED = {SEMI_SQEXP_F64_MEASURED:.1e})")


@pytest.mark.parametrize("entry", ["grid", "semi_mc", "semi_sqexp"])
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_two_calls_are_bit_equal(entry, tag):
    dims = (64, 48)
    c = _case(entry, dims, KERNELS[0], tag, NOBS)
    k = _kern(*KERNELS[0], c["dtype"])
    for ns in NSPLITS:
        a = _matvec(entry, k, c["grids"], c["x"], c["Ws"]["sign"], ns, c["u"])
        b = _matvec(entry, k, c["grids"], c["x"], c["Ws"]["sign"], ns, c["u"])
        assert torch.equal(a, b), (entry, tag, ns)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("kern", KERNELS, ids=kid)
def test_identity_weights_give_the_forward(kern, tag):
    """nw = M, W = I: the product's columns are the forward's element values, not only sums."""
    from hipgp_amd import kuf
    dims = (12, 10)
    dtype = torch.float64 if tag == "f64" else torch.float32
    grids, x = _inputs(dims, dtype, False, NOBS)
    k = _kern(*kern, dtype)
    K = kuf.kuf_grid(k, grids, x, PARAMS)
    tol = 1e-14 if tag == "f64" else 1e-6
    for ns in NSPLITS:
        out = kuf.kuf_grid_matvec(k, grids, x, PARAMS, torch.eye(120, dtype=dtype, device=DEV), nsplit=ns)
        rel = float(((out - K).double().abs() / K.double().abs().clamp_min(1e-300)).max())
        print(f"\nidentity {kid(kern)} {tag} nsplit={ns}: worst relative difference to kuf_grid = {rel:.3e}")
        assert rel <= tol
    # the line-integral entries: the same against their forwards (fp64 values of different orders of
    # magnitude per row; relative to the row's largest entry)
    if kern[0] == "sqexp":
        grids, x = _inputs(dims, dtype, True, NOBS)
        u = torch.tensor([0.37], dtype=dtype, device=DEV)
        eye = torch.eye(120, dtype=dtype, device=DEV)
        for fwd, out in ((kuf.kuf_semi_mc(k, grids, x, PARAMS, NPTS, u=u),
                          kuf.kuf_semi_mc_matvec(k, grids, x, PARAMS, NPTS, u=u, W=eye)),
                         (kuf.kuf_semi_sqexp(k, grids, x, PARAMS), kuf.kuf_semi_sqexp_matvec(k, grids, x, PARAMS, eye))):
            rel = float(((out - fwd).abs() / fwd.abs().amax(dim=1, keepdim=True)).max())
            print(f"identity line-integral {tag}: worst difference / row max = {rel:.3e}")
            assert rel <= tol


def test_empty_products_and_declined_kernels():
    from hipgp_amd import kuf
    dt = torch.float32
    grids, x = _inputs((12, 10), dt, True, NOBS)
    k = _kern("sqexp", None, dt)
    W = torch.ones(2, 120, dtype=dt, device=DEV)
    u = torch.tensor([0.37], dtype=dt, device=DEV)
    for f in (lambda xx, ww: kuf.kuf_grid_matvec(k, grids, xx, PARAMS, ww),
              lambda xx, ww: kuf.kuf_semi_mc_matvec(k, grids, xx, PARAMS, NPTS, u=u, W=ww),
              lambda xx, ww: kuf.kuf_semi_sqexp_matvec(k, grids, xx, PARAMS, ww)):
        assert tuple(f(x[:0], W).shape) == (0, 2)
        assert tuple(f(x, W[:0]).shape) == (NOBS, 0)
        assert tuple(f(x, W[0]).shape) == (NOBS, 1)                      # an (M,) vector is one row
    assert kuf.kuf_grid_matvec(_kern("gneiting", None, dt), grids, x, PARAMS, W) is None
    assert kuf.kuf_semi_sqexp_matvec(_kern("matern", 1.5, dt), grids, x, PARAMS, W) is None
    assert kuf.kuf_grid_matvec(k, grids, x, (1.0, torch.tensor([.2, .3], device=DEV)), W) is None
    ell = torch.tensor(0.3, device=DEV, requires_grad=True)
    assert kuf.kuf_grid_matvec(k, grids, x, (1.0, ell), W) is None
    with pytest.raises(ValueError):
        kuf.kuf_grid_matvec(k, grids, x, PARAMS, W[:, :-1])
    # |x| = 0 in the analytic line integral: NaN in that row, as the forward, and only there
    x0 = x.clone()
    x0[5] = 0.
    out = kuf.kuf_semi_sqexp_matvec(k, grids, x0, PARAMS, W)
    fwd = kuf.kuf_semi_sqexp(k, grids, x0, PARAMS)
    assert bool(torch.isnan(fwd[5]).all()) and bool(torch.isnan(out[5]).all())
    assert int(torch.isnan(out).any(dim=1).sum()) == 1


# ---- the model methods ---------------------------------------------------------------------------
MDIMS = (24, 20)
MAXITER = 400


def _model(family, dt, kern=("matern", 1.5)):
    import ziggy.hipgp as hg
    grids = [torch.linspace(-1, 1, m, dtype=dt) for m in MDIMS]
    torch.manual_seed(5)
    kw = dict(num_obs=64, sig2_init=1., ell_init=.3, noise2_init=.05, learn_kernel=False, dtype=dt)
    g = torch.Generator().manual_seed(11)
    if family == "block":
        mod = hg.BlockToeplitzGP(_kern(*kern, dt), grids, block_sizes=[2, 2], **kw)
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


def _model_points(dt):
    g = torch.Generator(device="cpu").manual_seed(6)
    x = torch.rand(NOBS, 2, generator=g, dtype=dt) * 2.2 - 1.1
    nrm = x.norm(dim=1, keepdim=True)
    return torch.where(nrm < 0.25, x * (0.25 / nrm), x).to(DEV)


def _gap(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def _model_gaps(family, dt):
    """[(what, max|new - materialised| / max|materialised|)] with both PCGs at their break test."""
    mod = _model(family, dt)
    sq = _model("mean-field", dt, kern=("sqexp", None)) if family == "mean-field" else None
    x = _model_points(dt)
    out = []
    with torch.no_grad():
        T = mod.toeplitz()
        Knm, _ = mod._make_grams(x)
        _, it_points = T._plan.pcg(Knm.clone(), MAXITER, 1e-8, precond=True, return_iters=True)
        qm, _ = mod.standard_variational_params()
        T.set_batch_shape((1,))
        b = T._matmul_by_R(qm.detach().reshape(1, -1).contiguous())
        _, it_mean = T._plan.pcg(b.clone(), MAXITER, 1e-8, precond=True, return_iters=True)
        print(f"\n{family} {dt}: PCG broke after {it_points} (one RHS per point) / {it_mean} (R qm) of {MAXITER}")
        assert it_points < MAXITER and it_mean < MAXITER
        mu_ref, _ = mod.predict(x, maxiter_cg=MAXITER, fused=False, streamed=False)
        mu = mod.predict_mean(x, maxiter_cg=MAXITER)
        assert tuple(mu.shape) == tuple(mu_ref.shape) == (NOBS, 1) and mu.device.type == "cpu"
        out.append(("predict_mean", _gap(mu, mu_ref)))
        eps = torch.randn(3, mod.Mprime, generator=torch.Generator().manual_seed(3), dtype=dt)
        kn = mod.compute_kn(mod._make_grams(x)[0], maxiter_cg=MAXITER)
        V = mod.variational_draws(3, eps=eps)
        d = mod.predict_draws(x, 3, eps=eps, maxiter_cg=MAXITER)
        assert tuple(d.shape) == (3, NOBS) and d.device.type == "cpu"
        out.append(("predict_draws", _gap(d, (kn @ V.t()).t())))
        # line-integral observations: analytic (SqExp only: the fused entry on a SqExp model, the
        # chunked fallback on this Matern one) and mc-biased with a given offset
        u = torch.tensor([0.37], dtype=dt, device=DEV)
        routes = [(mod, "mc-biased", dict(semi_integrated_samps=NPTS, mc_offset=u))]
        if sq is not None:
            routes.append((sq, "analytic", {}))
        for m_, est, kw in routes:
            Knm_i, _ = m_._make_grams(x, integrated_obs=True, semi_integrated_estimator=est,
                                      semi_integrated_samps=NPTS, mc_offset=kw.get("mc_offset"))
            kn_i = m_.compute_kn(Knm_i, maxiter_cg=MAXITER)
            ref = kn_i.matmul(m_.standard_variational_params()[0])
            mu_i = m_.predict_mean(x, integrated_obs=True, semi_integrated_estimator=est, maxiter_cg=MAXITER, **kw)
            out.append((f"predict_mean {est}", _gap(mu_i, ref)))
    return out


@pytest.mark.parametrize("family", ["mean-field", "block"])
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_model_routes_agree_with_the_materialised_ones(family, tag):
    dt = torch.float64 if tag == "f64" else torch.float32
    measured = MODEL_GAP_F64_MEASURED if tag == "f64" else MODEL_GAP_F32_MEASURED
    gaps = _model_gaps(family, dt)
    for what, g in gaps:
        print(f"  {family} {tag} {what}: relative gap {g:.3e} (measured worst {measured:.1e}, limit 10 x)")
    for what, g in gaps:
        assert g <= 10 * measured, (family, tag, what, g)


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_kept_weights_give_the_same_bits(family):
    mod = _model(family, torch.float64)
    x = _model_points(torch.float64)
    alpha = mod.mean_weights()
    assert tuple(alpha.shape) == (1, mod.M) and alpha.is_cuda and not alpha.requires_grad
    assert torch.equal(mod.predict_mean(x, weights=alpha), mod.predict_mean(x))
    # the chunked fallback (what a kernel without a fused entry takes) agrees with the fused product
    from hipgp_amd import kuf
    fused = mod.predict_mean(x, weights=alpha)
    Knm = kuf.kuf_grid(mod.kernel, mod.xgrids, x, mod.get_kernel_params())
    assert _gap(fused, Knm @ alpha.t()) < 1e-12


def test_predict_mean_never_holds_knm():
    """256^2 grid, fp32, 4096 points: Knm would be 1 GiB; the torch peak above the level before
    the call stays under 1/16 of it (measured on the second call)."""
    import ziggy.hipgp as hg
    dt = torch.float32
    m, N = 256, 4096
    grids = [torch.linspace(-1, 1, m, dtype=dt) for _ in range(2)]
    mod = hg.MeanFieldToeplitzGP(_kern("sqexp", None, dt), grids, num_obs=N, sig2_init=1., ell_init=.05,
                                 noise2_init=.05, learn_kernel=False, dtype=dt).cuda_params(0)
    g = torch.Generator(device="cpu").manual_seed(2)
    x = (torch.rand(N, 2, generator=g, dtype=dt) * 2 - 1).to(DEV)
    alpha = mod.mean_weights(maxiter_cg=5)
    mu1 = mod.predict_mean(x, weights=alpha)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    mu2 = mod.predict_mean(x, weights=alpha)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    knm_bytes = N * m * m * 4
    print(f"\npredict_mean 256^2 x {N}: torch peak {peak} B = {peak / knm_bytes:.2e} of Knm's {knm_bytes} B")
    assert torch.equal(mu1, mu2) and bool(torch.isfinite(mu2).all())
    assert peak <= knm_bytes / 16
