"""HGP_OP_RSQ and the inducing-grid posterior on the device.

Truth for the op is the NumPy restatement on the fp64 oracle's spectrum (grid_posterior_cases.
oracle_rsq); the yardstick is HGP_OP_R itself: on the same plan, dtype and input, the max-abs error
of RSQ relative to max |y| may be at most 10x the same figure of R against oracle.matmul_R (R and
RSQ run the same passes on spectra of the same layout; the factor covers the different dynamic
range of s^2).

Which R-spectrum route a shape takes follows from hgp_plan_create's L_R rule (power of two >= 4m - 4,
or the shortest 2^k / 3 * 2^k >= 3m - 3 where that grid is below 0.6 of it) and is ASSERTED from
hgp_plan_info's L_R, not assumed: the spectrum is real iff d >= 2 and L_R >= 2n - 1 on every axis
(and no L_R beyond 16384 points: the long_r set-up keeps the complex transform).
(9, 7) and (32, 24) take the short complex L_R = (24, 24) / (96, 96); real 2-D / 3-D spectra need an
axis of at most 5 points, hence (9, 4), (32, 5) and (9, 5, 4)."""
import ctypes

import numpy as np
import pytest
import torch

from grid_posterior_cases import dense_R, max_rel, oracle_rsq
from oracle import ziggy_oracle as zo

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64

# dims -> (spectrum real?, L_R); fp32-only where fp64 takes the full-grid route
SHAPES = {
    "1d_33": ((33,), False, (128,)),
    "2d_9x7": ((9, 7), False, (24, 24)),
    "2d_32x24": ((32, 24), False, (96, 96)),
    "2d_9x4_real": ((9, 4), True, (32, 16)),
    "2d_32x5_real": ((32, 5), True, (128, 16)),
    "2d_33x33_tri": ((33, 33), False, (96, 96)),
    "3d_6x5x4": ((6, 5, 4), False, (16, 16, 16)),
    "3d_9x5x4_real": ((9, 5, 4), True, (32, 16, 16)),
    "3d_9x9x5_mixed": ((9, 9, 5), False, (24, 24, 16)),
    "2d_5500x3_long_r": ((5500, 3), False, (32768, 8)),
}
_CACHE = {}


def _column(dims, ell=.3, nu=.5, jitter=1e-3):
    grids = [np.linspace(-1, 1, m) for m in dims]
    return zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("matern", x, y, (1., ell), nu=nu), jitter)


def _oracle(dims, **kw):
    """One oracle (and its reference outputs) per column, shared by the tests."""
    key = (dims, tuple(sorted(kw.items())))
    if key not in _CACHE:
        col = _column(dims, **kw)
        _CACHE[key] = (col, zo.ToeplitzOracle(col, dims))
    return _CACHE[key]


def _plan(dims, dt, col):
    from hipgp_amd.plan import ToeplitzPlan
    P = ToeplitzPlan(dims, dt, DEV)
    nc = P.set_column(torch.tensor(col, device=DEV, dtype=dt), count_clamped=True)
    return P, nc


def _spec_real(P):
    d = len(P.dims)
    return d >= 2 and all(L >= 2 * n - 1 and L // 2 <= 8192 for L, n in zip(P.L_R[:d], P.ndims))


def _specR_bytes(P):
    """Bytes of the R pass spectrum (include/hipgp.h layout: 1-D L_R complex values; 2-D
    [L_R0][round_up(L_R1 / 2 + 1, 8)]; 3-D [L_R2 / 2 + 1][L_R1][L_R0]; real or complex)."""
    L = P.L_R[:len(P.dims)]
    es = 4 if P.dtype == F32 else 8
    if len(L) == 1:
        return L[0] * 2 * es
    last = (L[-1] // 2 + 1) if len(L) == 3 else (L[-1] // 2 + 1 + 7) // 8 * 8
    return int(np.prod(L[:-1])) * last * (es if _spec_real(P) else 2 * es)


def _errs(P, O, w, dt):
    """(RSQ error, R error) of the plan on input w (fp64 values of the dtype), relative to max |y|."""
    from hipgp_amd import _lib
    wt = torch.tensor(w, device=DEV, dtype=dt)
    w64 = wt.double().cpu().numpy()
    got_r = P.apply(_lib.OP_R, wt).double().cpu().numpy()
    got_q = P.apply(_lib.OP_RSQ, wt).double().cpu().numpy()
    ref_r, ref_q = O.matmul_R(w64), oracle_rsq(O, w64)
    assert got_q.shape == ref_q.shape == (w.shape[0], O.M)
    return max_rel(got_q, ref_q), max_rel(got_r, ref_r), got_q


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_rsq_parity(case, dt):
    from hipgp_amd import _lib
    dims, real, LR = SHAPES[case]
    col, O = _oracle(dims)
    P, _ = _plan(dims, dt, col)
    assert P.L_R[:len(dims)] == LR, (case, P.L_R)
    assert _spec_real(P) == real, (case, P.L_R, P.ndims)
    w = np.random.RandomState(4).randn(3, O.Mp)
    if case.endswith("long_r") and dt == F64:
        # fp64 lines of 16384 points: the full-grid route, refused by name (test_unsupported_routes)
        with pytest.raises(_lib.HipgpError, match="full-grid route"):
            P.apply(_lib.OP_RSQ, torch.tensor(w, device=DEV, dtype=dt))
        return
    e_q, e_r, _ = _errs(P, O, w, dt)
    print(f"RSQ parity {case} {dt}: L_R {LR} real {real}: RSQ {e_q:.3e}  R {e_r:.3e}")
    assert e_q <= 10 * e_r, (case, e_q, e_r)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims", [(33,), (12, 10), (9, 4), (6, 5, 4)], ids=str)
def test_rsq_of_ones_is_the_kernel_diagonal(dims, dt):
    """sum_k s^2[(j - k) mod n] = IFFT_n(D)[0] = column[0] (nugget included) where no eigenvalue is
    clamped: a Matern-1/2 column (ell 0.3 on [-1, 1], nugget 1e-3; its smallest eigenvalue on these
    grids is above 0.08)."""
    col, O = _oracle(dims)
    P, nclamp = _plan(dims, dt, col)
    assert nclamp == 0
    ones = np.ones((1, O.Mp))
    _, e_r, got = _errs(P, O, ones, dt)
    e_q = float(np.max(np.abs(got - col[0])) / col[0])
    print(f"RSQ ones {dims} {dt}: |RSQ 1 - column[0]| / column[0] = {e_q:.3e}  R {e_r:.3e}")
    assert e_q <= 10 * e_r, (dims, e_q, e_r)


@pytest.mark.parametrize("dims,dt", [((32, 24), F32), ((9, 4), F64), ((6, 5, 4), F32), ((33,), F64)], ids=str)
def test_lazy_table_and_invalidation(dims, dt):
    from hipgp_amd import _lib
    from hipgp_amd.plan import ToeplitzPlan, release_pool
    release_pool()                                    # a fresh plan: no table left by an earlier user
    col, O = _oracle(dims)
    P = ToeplitzPlan(dims, dt, DEV)
    P.set_column(torch.tensor(col, device=DEV, dtype=dt))
    w = torch.tensor(np.random.RandomState(6).randn(2, O.Mp), device=DEV, dtype=dt)
    t0 = P.mem()["tables"]
    r_before = P.apply(_lib.OP_R, w).clone()
    assert P.mem()["tables"] == t0                    # nothing but RSQ builds the table
    q1 = P.apply(_lib.OP_RSQ, w).clone()
    t1 = P.mem()["tables"]
    assert t1 - t0 == _specR_bytes(P), (t1 - t0, _specR_bytes(P))
    assert torch.equal(P.apply(_lib.OP_RSQ, w), q1) and P.mem()["tables"] == t1      # built once
    assert torch.equal(P.apply(_lib.OP_RSQ, w), q1)   # third identical call: the replayed graph
    P.trim()
    assert P.mem()["tables"] == t1                    # trim keeps it like the other tables
    assert torch.equal(P.apply(_lib.OP_RSQ, w), q1)
    assert torch.equal(P.apply(_lib.OP_R, w), r_before)        # R is bitwise what it was
    # a second column (after a trim: the set-up scratch is re-ensured): the table is dropped ...
    col2, O2 = _oracle(dims, ell=.15, nu=1.5, jitter=1e-2)
    P.trim()
    P.set_column(torch.tensor(col2, device=DEV, dtype=dt))
    assert P.mem()["tables"] == t0
    # ... and rebuilt from the new column (first use after a trim of the set-up scratch as well)
    P.trim()
    wn = np.random.RandomState(7).randn(2, O2.Mp)
    e_q, e_r, _ = _errs(P, O2, wn, dt)
    assert P.mem()["tables"] == t1
    assert e_q <= 10 * e_r, (e_q, e_r)
    assert max_rel(P.apply(_lib.OP_RSQ, w).double().cpu().numpy(), oracle_rsq(O, w.double().cpu().numpy())) > 1e-3


def test_unsupported_routes():
    """grid_r plans, the pass split, the slab split and the column gradient refuse HGP_OP_RSQ by
    name; the output buffer keeps its fill and no table is built."""
    from hipgp_amd import _lib
    from hipgp_amd.plan import ToeplitzPlan
    L = _lib.lib()
    E_UNSUPPORTED = -4
    dims = (9000,)                                     # the long-axis tests' smallest fp64 1-D axis beyond 8192
    grids = [np.linspace(-1, 1, dims[0])]
    col = zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("matern", x, y, (1., 40. / 9000), nu=1.5), .1)
    P = ToeplitzPlan(dims, F64, DEV)
    P.set_column(torch.tensor(col, device=DEV))
    x = torch.ones(1, P.Mprime, device=DEV, dtype=F64)
    y = torch.full((1, P.M), 7., device=DEV, dtype=F64)
    t0 = P.mem()["tables"]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.hgp_toeplitz_apply(P._h, _lib.OP_RSQ, p(x), p(y), 1) == E_UNSUPPORTED
    msg = L.hgp_last_error().decode()
    assert "full-grid route" in msg and "grid_r" in msg, msg
    assert P.mem()["tables"] == t0 and bool((y == 7.).all())
    # a pass-route plan: the other entry points
    dims = (9, 7)
    col, O = _oracle(dims)
    P, _ = _plan(dims, F64, col)
    x = torch.ones(1, P.Mprime, device=DEV, dtype=F64)
    y = torch.full((1, P.M), 7., device=DEV, dtype=F64)
    g = torch.ones(1, P.M, device=DEV, dtype=F64)
    cg = torch.full((P.M,), 7., device=DEV, dtype=F64)
    t0 = P.mem()["tables"]
    for pss in (-1, 0, 1):
        assert L.hgp_toeplitz_apply_pass(P._h, _lib.OP_RSQ, p(x), p(y), 1, pss) in (E_UNSUPPORTED, -1)
        assert b"RSQ" in L.hgp_last_error()
    assert L.hgp_plan_column_grad(P._h, _lib.OP_RSQ, p(x), p(g), 1, p(cg)) in (E_UNSUPPORTED, -1)
    assert b"RSQ" in L.hgp_last_error()
    with pytest.raises(_lib.HipgpError, match="RSQ"):
        P.column_grad(_lib.OP_RSQ, x, g)
    ng, inner = ctypes.c_int64(-5), ctypes.c_int64(-5)
    assert L.hgp_slab_info(P._h, _lib.OP_RSQ, ctypes.byref(ng), ctypes.byref(inner)) in (E_UNSUPPORTED, -1)
    assert (ng.value, inner.value) == (-5, -5)
    E = torch.full((4096,), 7., device=DEV, dtype=torch.complex128)
    assert L.hgp_slab_pass(P._h, _lib.OP_RSQ, _lib.SLAB_FWD, p(x), p(E), 1, 1, 0, 0) in (E_UNSUPPORTED, -1)
    assert b"RSQ" in L.hgp_last_error()
    torch.cuda.synchronize()
    assert P.mem()["tables"] == t0
    assert bool((y == 7.).all()) and bool((cg == 7.).all()) and bool((E == 7.).all())
    # an op number past the last one stays an argument error
    assert L.hgp_toeplitz_apply(P._h, 5, p(x), p(y), 1) == -1


def test_drop_in_rsq_and_autograd_refusal():
    import ziggy.kernels as zk
    from ziggy.misc.toeplitz_tensor import ToeplitzTensor
    dims = (9, 7)
    k = zk.Matern(nu=.5, dtype=F64)
    grids = [torch.linspace(-1, 1, m, dtype=F64, device=DEV) for m in dims]
    T = ToeplitzTensor(grids, lambda x, y: k.forward(x, y, params=(1., .3)), jitter_val=1e-3)
    O = zo.ToeplitzOracle(T.column.detach().cpu().numpy(), dims)
    w = torch.randn(2, O.Mp, device=DEV, dtype=F64, generator=torch.Generator(device=DEV).manual_seed(1))
    T.set_batch_shape((2,))
    got = T._matmul_by_Rsq(w.reshape((2,) + O.ndims))           # grid-shaped input as _matmul_by_R takes it
    assert max_rel(got.cpu().numpy(), oracle_rsq(O, w.cpu().numpy())) < 1e-12
    with pytest.raises(RuntimeError, match="no backward"):
        T._matmul_by_Rsq(w.clone().requires_grad_(True))
    with torch.no_grad():
        assert torch.equal(T._matmul_by_Rsq(w.clone().requires_grad_(True)), got)


# ---- model level ----------------------------------------------------------------------------------
MDIMS = (12, 10)
JITTER = 1e-3


def _gpu_model():
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    dt = F64
    grids = [torch.linspace(-1, 1, m, dtype=dt) for m in MDIMS]
    torch.manual_seed(5)
    mod = hg.MeanFieldToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, num_obs=40, sig2_init=1., ell_init=.3,
                                 noise2_init=.05, learn_kernel=False, dtype=dt, jitter_val=JITTER)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():       # random theta1 / theta2 (theta2 < 0)
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=dt))
        mod.global_theta2.copy_(-(torch.rand(mod.Mprime, 1, generator=g, dtype=dt) * 4 + .5))
    return mod.cuda_params(0)


def test_model_grid_posterior_and_draws_match_dense():
    from hipgp_amd import _lib
    mod = _gpu_model()
    T = mod.toeplitz()
    O = zo.ToeplitzOracle(T.column.detach().cpu().numpy(), MDIMS)
    R = dense_R(O)
    qm, qS = (t.detach().cpu().numpy().reshape(-1) for t in mod.standard_variational_params())
    eps = torch.randn(3, O.Mp, dtype=F64, generator=torch.Generator().manual_seed(3))
    v = qm[None, :] + np.sqrt(qS)[None, :] * eps.numpy()
    # the yardstick: R's own error on each input, on the model's plan
    P = T._plan
    e_r = {}
    for name, x in (("qm", qm[None, :]), ("qS", qS[None, :]), ("v", v), ("eps", eps.numpy()), ("one", np.ones((1, O.Mp)))):
        got = P.apply(_lib.OP_R, torch.tensor(x, device=DEV)).cpu().numpy()
        e_r[name] = max_rel(got, O.matmul_R(x))
    mean, sd = mod.grid_posterior(Kmm=T)
    assert mean.is_cuda and sd.is_cuda and tuple(mean.shape) == MDIMS and tuple(sd.shape) == MDIMS
    assert mean.dtype == F64 and not mean.requires_grad and not sd.requires_grad
    figs = {"mean": (max_rel(mean.cpu().numpy().reshape(-1), R @ qm), e_r["qm"]),
            "sd": (max_rel(sd.cpu().numpy().reshape(-1), np.sqrt((R * R) @ qS)), e_r["qS"])}
    u = mod.sample_grid(3, eps=eps.to(DEV), Kmm=T)
    assert tuple(u.shape) == (3,) + MDIMS and u.is_cuda
    figs["draw"] = (max_rel(u.cpu().numpy().reshape(3, -1), v @ R.T), e_r["v"])
    m0, sd0 = mod.grid_posterior(prior=True, Kmm=T)
    assert torch.count_nonzero(m0) == 0
    figs["prior sd"] = (max_rel(sd0.cpu().numpy().reshape(-1), np.sqrt((R * R).sum(1))), e_r["one"])
    u0 = mod.sample_grid(3, prior=True, eps=eps.to(DEV), Kmm=T)
    figs["prior draw"] = (max_rel(u0.cpu().numpy().reshape(3, -1), eps.numpy() @ R.T), e_r["eps"])
    for name, (e, er) in figs.items():
        print(f"model {name}: {e:.3e}  (R on the same input {er:.3e})")
    for name, (e, er) in figs.items():
        assert e <= 10 * er, (name, e, er)
    # a Kmm without the operator falls through to a fresh one; generator draws are reproducible
    mean2, sd2 = mod.grid_posterior(Kmm=object())
    assert torch.equal(mean2, mean) and torch.equal(sd2, sd)
    ga = torch.Generator(device=DEV).manual_seed(4)
    gb = torch.Generator(device=DEV).manual_seed(4)
    assert torch.equal(mod.sample_grid(2, generator=ga), mod.sample_grid(2, generator=gb))


def test_model_mean_against_predict_on_the_grid():
    """predict_mean(xinduce) = u - jitter K^-1 u with u = R qm (Knm = K - jitter I on the grid): the
    grid posterior is that of the inducing values, nugget included.  predict's PCG stops at residual
    1e-8 and lambda_min(K) >= jitter = 1e-3, so its K^-1 Knm^T rows are within 1e-5 |.| and the means
    within ~1e-5 |u|; asserted at 10x that, 1e-4 |u|_2."""
    mod = _gpu_model()
    T = mod.toeplitz()
    mean, _ = mod.grid_posterior(Kmm=T)
    u = mean.reshape(1, -1)
    T.set_batch_shape((1,))
    Kinv_u = T.inv_matmul(u.contiguous(), do_precond=True, maxiter=2000, tol=1e-12)
    _, iters = T._plan.pcg(u.contiguous(), 2000, 1e-12, precond=True, return_iters=True)
    assert iters < 2000                                    # the same solve reaches its break
    ref = (u - JITTER * Kinv_u).reshape(-1).cpu()
    mu, _ = mod.predict(mod.xinduce, maxiter_cg=2000, Kmm=T)
    # predict's own solve reached its break as well
    Knm, _ = mod._make_grams(mod.xinduce)
    _, it_p = T._plan.pcg(Knm.contiguous(), 2000, 1e-8, precond=True, return_iters=True)
    assert it_p < 2000
    diff = float(torch.linalg.norm(mu.reshape(-1) - ref))
    un = float(torch.linalg.norm(u))
    print(f"predict(xinduce) vs u - jitter K^-1 u: |diff|_2 = {diff:.3e}, |u|_2 = {un:.3e}, PCG iterations {iters} / {it_p}")
    assert diff <= 1e-4 * un, (diff, un)
