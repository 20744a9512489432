"""The transposed fused Kuf products (hgp_kuf_grid_rmatvec / hgp_kuf_semi_mc_rmatvec /
hgp_kuf_semi_sqexp_rmatvec behind `kuf_grid_rmatvec` / `kuf_semi_mc_rmatvec` / `kuf_semi_sqexp_rmatvec`)
against the broadcast kernels of ziggy.kernels (`forward`, `k_semi_mc` with the same u, `k_semi`)
materialised in fp64 on the device and multiplied from the left by C.

Every error of a product row s is measured relative to S[s] = max_j sum_n |Kuf[n, j] c[s, n]| of the
fp64 reference, so a sum that cancels (the random-sign C) does not inflate it.
  fp64: |error| <= 1e-10 S -- the forward product's cap (worst-case linear accumulation of at most
        300 terms here of a few operations each, 1.1e-16 apiece).
  fp64, semi-sqexp: the Phi difference cancels, so no bound is fixed in advance: 10 x the worst case
        measured over this matrix, SEMI_SQEXP_F64_MEASURED (the forward product's convention).
  fp32: no worse than 4 x the error of torch's own fp32 C32 @ Knm32 on the same inputs, plus 1e-7 S.
Adjoint identity <Kuf w, c> = <w, Kuf^T c> with the existing `*_matvec` on the left, relative to
sum |Kuf| |w| |c|: fp64 <= 1e-12; semi-sqexp 10 x the measured ADJ_SEMI_SQEXP_F64_MEASURED.
Each test prints its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

KERNELS = [("sqexp", None), ("matern", 0.5), ("matern", 1.5), ("matern", 2.5)]
GRIDS = [(70,), (8, 6), (24, 20), (6, 5, 4)]      # (8, 6): M = 48, less than one wave
NOBS = (1, 63, 257, 300)                           # across the 64-lane and the 256-run boundaries
NCS = (1, 3, 8, 9)                                 # 9: a group of 8 coefficient rows and a tail group
NSPLITS = (0, 1, 3, 99)                            # 99: more than the number of runs
NPTS = 6
PARAMS = (1.3, 0.27)
F64_BOUND = 1e-10
F32_FLOOR = 1e-7
SEMI_SQEXP_F64_MEASURED = 1.2e-15     # worst |error| / S of kuf_semi_sqexp_rmatvec in fp64 over the matrix
SEMI_SQEXP_F64_BOUND = 10 * SEMI_SQEXP_F64_MEASURED
ADJ_F64_BOUND = 1e-12
ADJ_SEMI_SQEXP_F64_MEASURED = 6.7e-18  # worst adjoint gap of the semi-sqexp pair in fp64
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
    x[min(3, nobs - 1)] = torch.stack([gr[len(gr) // 3] for gr in grids])
    return grids, x


def _mesh(grids):
    return torch.stack([a.reshape(-1) for a in torch.meshgrid(*grids, indexing="ij")], dim=-1)


def _coefs(nobs, dtype):
    """(9, nobs): random signs times random magnitudes; rows [:nc] are used."""
    g = torch.Generator(device="cpu").manual_seed(11)
    sign = (torch.randint(0, 2, (max(NCS), nobs), generator=g, dtype=torch.int64) * 2 - 1).to(dtype)
    mag = torch.rand(max(NCS), nobs, generator=g, dtype=dtype) + 0.5
    return (sign * mag).to(DEV)


def _torch_K(entry, k, xs, x, params, u):
    if entry == "grid":
        return k.forward(x, xs, params=params)
    if entry == "semi_mc":
        return k.k_semi_mc(xs, x, params, npts=NPTS, u=u).transpose(0, 1)
    return k.k_semi(xs, x, params).transpose(0, 1)


def _rmatvec(entry, k, grids, x, C, nsplit, u):
    from hipgp_amd import kuf
    if entry == "grid":
        return kuf.kuf_grid_rmatvec(k, grids, x, PARAMS, C, nsplit=nsplit)
    if entry == "semi_mc":
        return kuf.kuf_semi_mc_rmatvec(k, grids, x, PARAMS, NPTS, u=u, C=C, nsplit=nsplit)
    return kuf.kuf_semi_sqexp_rmatvec(k, grids, x, PARAMS, C, nsplit=nsplit)


def _matvec(entry, k, grids, x, W, u):
    from hipgp_amd import kuf
    if entry == "grid":
        return kuf.kuf_grid_matvec(k, grids, x, PARAMS, W)
    if entry == "semi_mc":
        return kuf.kuf_semi_mc_matvec(k, grids, x, PARAMS, NPTS, u=u, W=W)
    return kuf.kuf_semi_sqexp_matvec(k, grids, x, PARAMS, W)


@functools.lru_cache(maxsize=None)
def _case(entry, dims, kern, tag, nobs):
    """Inputs in the test dtype, the fp64 reference product and S on those same values, and (fp32)
    torch's own fp32 product; computed once and shared, never changed."""
    dtype = torch.float64 if tag == "f64" else torch.float32
    grids, x = _inputs(dims, dtype, entry != "grid", nobs)
    u = torch.tensor([0.37], dtype=dtype, device=DEV)
    C = _coefs(nobs, dtype)
    K64 = _torch_K(entry, _kern(*kern, torch.float64), _mesh([g.double() for g in grids]), x.double(), PARAMS,
                   u.double())
    assert bool(torch.isfinite(K64).all())
    ref = C.double() @ K64
    S = (C.double().abs() @ K64.abs()).amax(dim=1, keepdim=True)          # (9, 1)
    t32 = None
    if tag == "f32":
        K32 = _torch_K(entry, _kern(*kern, dtype), _mesh(grids), x, PARAMS, u)
        t32 = (C @ K32).double()
    return dict(grids=grids, x=x, u=u, C=C, ref=ref, S=S, t32=t32, dtype=dtype, K64=K64)


def _check(entry, dims, kern, tag, f64_bound):
    """Every (nobs, nc, nsplit): the error bound, bit-equality of a second call, and the slices'
    agreement with nsplit = 1 within the same bound.  Returns the worst |error| / S."""
    M = int(np.prod(dims))
    worst, worst32 = 0.0, 0.0
    for nobs in NOBS:
        c = _case(entry, dims, kern, tag, nobs)
        k = _kern(*kern, c["dtype"])
        assert bool((c["S"] > 0).all())
        for nc in NCS:
            ref, S = c["ref"][:nc], c["S"][:nc]
            e32 = None if c["t32"] is None else float(((c["t32"][:nc] - ref).abs() / S).max())
            bound = f64_bound if tag == "f64" else 4 * e32 + F32_FLOOR
            outs = {}
            for ns in NSPLITS:
                out = _rmatvec(entry, k, c["grids"], c["x"], c["C"][:nc], ns, c["u"])
                assert out is not None and tuple(out.shape) == (nc, M) and out.dtype == c["dtype"]
                again = _rmatvec(entry, k, c["grids"], c["x"], c["C"][:nc], ns, c["u"])
                assert torch.equal(out, again), (entry, dims, kern, tag, nobs, nc, ns, "second call differs")
                outs[ns] = out
                e = float(((out.double() - ref).abs() / S).max())
                worst, worst32 = max(worst, e), max(worst32, e32 or 0.0)
                print(f"{entry} {did(dims)} {kid(kern)} {tag} nobs={nobs} nc={nc} nsplit={ns}: |error|/S = {e:.3e}"
                      + ("" if e32 is None else f" (torch fp32: {e32:.3e})"))
                assert e <= bound, (entry, dims, kern, tag, nobs, nc, ns, e, bound)
            for ns in NSPLITS:
                gap = float(((outs[ns].double() - outs[1].double()).abs() / S).max())
                assert gap <= bound, (entry, dims, kern, tag, nobs, nc, ns, "split gap", gap, bound)
            if nobs <= 256:         # one run: every nsplit is clamped to one slice, the same bits
                assert all(torch.equal(outs[ns], outs[1]) for ns in NSPLITS)
    print(f"{entry} {did(dims)} {kid(kern)} {tag}: worst |error|/S = {worst:.3e}"
          + ("" if tag == "f64" else f" (torch fp32 worst: {worst32:.3e})"))
    return worst


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("kern", KERNELS, ids=kid)
@pytest.mark.parametrize("dims", GRIDS, ids=did)
def test_grid_rmatvec_matches_torch(dims, kern, tag):
    _check("grid", dims, kern, tag, F64_BOUND)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("kern", KERNELS + [("gneiting", None)], ids=kid)
@pytest.mark.parametrize("dims", GRIDS, ids=did)
def test_semi_mc_rmatvec_matches_torch(dims, kern, tag):
    _check("semi_mc", dims, kern, tag, F64_BOUND)


@pytest.mark.parametrize("dims", GRIDS, ids=did)
def test_semi_sqexp_rmatvec_matches_torch_fp32(dims):
    _check("semi_sqexp", dims, KERNELS[0], "f32", None)


def test_semi_sqexp_rmatvec_matches_torch_fp64():
    worst = max(_check("semi_sqexp", dims, KERNELS[0], "f64", SEMI_SQEXP_F64_BOUND) for dims in GRIDS)
    print(f"\nsemi-sqexp fp64 worst |error|/S over the matrix = {worst:.3e} "
          f"(SEMI_SQEXP_F64_MEASURED = {SEMI_SQEXP_F64_MEASURED:.1e})")


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("kern", KERNELS, ids=kid)
def test_identity_coefficients_give_the_forward_transposed(kern, tag):
    """nc = nobs, C = I: the product's rows are the forward's element values, not only sums."""
    from hipgp_amd import kuf
    dims, nobs = (12, 10), 37
    dtype = torch.float64 if tag == "f64" else torch.float32
    grids, x = _inputs(dims, dtype, False, nobs)
    k = _kern(*kern, dtype)
    K = kuf.kuf_grid(k, grids, x, PARAMS)
    tol = 1e-14 if tag == "f64" else 1e-6
    eye = torch.eye(nobs, dtype=dtype, device=DEV)
    for ns in NSPLITS:
        out = kuf.kuf_grid_rmatvec(k, grids, x, PARAMS, eye, nsplit=ns)
        rel = float(((out - K).double().abs() / K.double().abs().clamp_min(1e-300)).max())
        print(f"\nidentity {kid(kern)} {tag} nsplit={ns}: worst relative difference to kuf_grid = {rel:.3e}")
        assert rel <= tol
    if kern[0] == "sqexp":      # the line-integral entries against their forwards, relative to the row's largest
        grids, x = _inputs(dims, dtype, True, nobs)
        u = torch.tensor([0.37], dtype=dtype, device=DEV)
        for fwd, out in ((kuf.kuf_semi_mc(k, grids, x, PARAMS, NPTS, u=u),
                          kuf.kuf_semi_mc_rmatvec(k, grids, x, PARAMS, NPTS, u=u, C=eye)),
                         (kuf.kuf_semi_sqexp(k, grids, x, PARAMS), kuf.kuf_semi_sqexp_rmatvec(k, grids, x, PARAMS, eye))):
            rel = float(((out - fwd).abs() / fwd.abs().amax(dim=1, keepdim=True)).max())
            print(f"identity line-integral {tag}: worst difference / row max = {rel:.3e}")
            assert rel <= tol


@pytest.mark.parametrize("entry,kern", [("grid", KERNELS[0]), ("grid", KERNELS[3]), ("semi_mc", KERNELS[2]),
                                        ("semi_mc", ("gneiting", None)), ("semi_sqexp", KERNELS[0])],
                         ids=lambda v: v if isinstance(v, str) else kid(v))
def test_adjoint_identity_with_the_forward_product_fp64(entry, kern):
    """<Kuf w, c> = <w, Kuf^T c>: the existing product on the left, the new one on the right, one
    recorded offset u for both sides of semi-mc."""
    worst = 0.0
    for dims in GRIDS:
        c = _case(entry, dims, kern, "f64", 300)
        k = _kern(*kern, torch.float64)
        M = int(np.prod(dims))
        g = torch.Generator(device="cpu").manual_seed(17)
        w = torch.randn(1, M, generator=g, dtype=torch.float64).to(DEV)
        cc = c["C"][:1]
        left = torch.sum(_matvec(entry, k, c["grids"], c["x"], w, c["u"])[:, 0] * cc[0])
        right = torch.sum(w[0] * _rmatvec(entry, k, c["grids"], c["x"], cc, 0, c["u"])[0])
        scale = float(cc.abs() @ c["K64"].abs() @ w.abs().t())
        gap = abs(float(left - right)) / scale
        worst = max(worst, gap)
        print(f"adjoint {entry} {kid(kern)} {did(dims)}: |<Kuf w, c> - <w, Kuf^T c>| / sum|Kuf||w||c| = {gap:.3e}")
    bound = 10 * ADJ_SEMI_SQEXP_F64_MEASURED if entry == "semi_sqexp" else ADJ_F64_BOUND
    assert worst <= bound, (entry, kern, worst, bound)


def test_empty_products_and_declined_kernels():
    from hipgp_amd import kuf
    dt = torch.float32
    nobs = 37
    grids, x = _inputs((12, 10), dt, True, nobs)
    k = _kern("sqexp", None, dt)
    C = torch.ones(2, nobs, dtype=dt, device=DEV)
    u = torch.tensor([0.37], dtype=dt, device=DEV)
    for f in (lambda xx, cc: kuf.kuf_grid_rmatvec(k, grids, xx, PARAMS, cc),
              lambda xx, cc: kuf.kuf_semi_mc_rmatvec(k, grids, xx, PARAMS, NPTS, u=u, C=cc),
              lambda xx, cc: kuf.kuf_semi_sqexp_rmatvec(k, grids, xx, PARAMS, cc)):
        empty = f(x[:0], C[:, :0])                                         # an empty sum is zero
        assert tuple(empty.shape) == (2, 120) and bool((empty == 0).all())
        assert tuple(f(x, C[:0]).shape) == (0, 120)
        assert tuple(f(x, C[0]).shape) == (1, 120)                         # an (nobs,) vector is one row
    assert kuf.kuf_grid_rmatvec(_kern("gneiting", None, dt), grids, x, PARAMS, C) is None
    assert kuf.kuf_semi_sqexp_rmatvec(_kern("matern", 1.5, dt), grids, x, PARAMS, C) is None
    assert kuf.kuf_grid_rmatvec(k, grids, x, (1.0, torch.tensor([.2, .3], device=DEV)), C) is None
    ell = torch.tensor(0.3, device=DEV, requires_grad=True)
    assert kuf.kuf_grid_rmatvec(k, grids, x, (1.0, ell), C) is None
    with pytest.raises(ValueError):
        kuf.kuf_grid_rmatvec(k, grids, x, PARAMS, C[:, :-1])
    # |x| = 0 in the analytic line integral: a NaN row of Kuf, so every sum over it is NaN, as the
    # dense product; a zero coefficient does not hide it (0 * NaN)
    x0 = x.clone()
    x0[5] = 0.
    fwd = kuf.kuf_semi_sqexp(k, grids, x0, PARAMS)
    out = kuf.kuf_semi_sqexp_rmatvec(k, grids, x0, PARAMS, C)
    assert bool(torch.isnan(fwd[5]).all()) and bool(torch.isnan(out).all())
    assert bool(torch.isnan(C @ fwd).all())
