"""hgp_rt_block_stats / ToeplitzPlan.rt_block_stats / elbo_and_grad(streamed=True) /
predict(streamed=True): the block-diagonal family's sums of kn = R^T d (per-block grams
sum_n ivar_n kn_blk kn_blk^T and the rows (kn.qm, |kn|^2, kn^T S kn)) with kn held one piece of
right-hand sides at a time, the gram continuing from piece to piece.

Operator level: truth is the fp64 oracle's R^T followed by einsum over block_chunks indices (as
_ref_stats of tests/test_block_gpu.py); the yardstick is the materialised route on the same plan and
inputs (plan.apply(RT), then hgp_block_stats and hgp_meanfield_rowdots).  Per column of out3 (norm
over the batch) and for the gram (norm over all entries) the streamed error may be at most 4x the
materialised one plus a floor of 1e-6 (fp32) / 1e-12 (fp64) x |truth|.

Grids (as m; the blocks tile n = 2m - 2) and the k_block_stats_rt branch each reaches:
  (11, 9)   blocks (4, 4)    bs 16: TA = 0, one gram entry per thread, one block per workgroup
  (21, 16)  blocks (10, 10)  bs 100: 7 x 7 register tiles
  (9, 17)   blocks (8, 16)   bs 128: 8 x 8 register tiles (fp64: S read from global memory)
  (6, 5, 4) blocks (2, 2, 3) 3-D, bs 12
  (16, 8)   blocks (2, 2)    bs 4: 16 blocks per workgroup
  (10, 4)   blocks (3, 1)    bs 3: ragged last workgroup (36 blocks, 16 per workgroup)
Batches: B = 1; B = 17 with piece_rhs = 5 (three full pieces and a tail); B = 70 with piece_rhs = 0
(one piece, two 64-RHS chunks) and with piece_rhs = 33 (the continuation crosses a piece that does
not end on the chunk boundary)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from block_cases import block_model, noise_of
from golden_cases import load, rel_err
from oracle import ziggy_oracle as zo

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = [((11, 9), (4, 4)), ((21, 16), (10, 10)), ((9, 17), (8, 16)), ((6, 5, 4), (2, 2, 3)), ((16, 8), (2, 2)),
         ((10, 4), (3, 1))]
BATCHES = [(1, 0), (17, 5), (70, 0), (70, 33)]                # (B, piece_rhs)
_ID = lambda g: "x".join(str(m) for m in g)
_CASE = {}


def _column(dims):
    grids = [np.linspace(-1, 1, m) for m in dims]
    ell = 40.0 / max(max(dims), 80)
    return zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("matern", x, y, (1.0, ell), nu=1.5), 0.1)


def _case(dims, blocks, nb=70):
    """column, fp64 inputs and the fp64 kn in block order of one grid, computed once (read-only)."""
    key = (dims, blocks)
    if key not in _CASE:
        from hipgp_amd.ziggy.hipgp import block_chunks
        col = _column(dims)
        O = zo.ToeplitzOracle(col, dims)
        idx = block_chunks([2 * m - 2 for m in dims], blocks)[0].numpy()
        nblk, bs = idx.shape
        rs = np.random.RandomState(23)
        d = rs.randn(nb, O.M)
        qm = rs.randn(O.Mp)
        iv = rs.rand(nb) + 0.5
        A = rs.randn(nblk, bs, bs)
        S = A @ A.transpose(0, 2, 1) / bs
        kn = O.matmul_RT(d).reshape(nb, -1)
        kb = kn[:, idx]                                              # (B, nblk, bs)
        dots = np.stack([kn @ qm, (kn * kn).sum(1), np.einsum("bki,kij,bkj->b", kb, S, kb)], axis=1)
        for a in (d, qm, iv, S, kb, dots):
            a.setflags(write=False)
        _CASE[key] = (col, d, qm, iv, S, kb, dots)
    return _CASE[key]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _block_stats(P, blocks, kn, iv, S, trace=False):
    """hgp_block_stats on a materialised kn: (gram, knSkn[, trSG])."""
    from hipgp_amd import _lib
    nd = len(blocks)
    bs = int(np.prod(blocks))
    nblk = P.Mprime // bs
    B = kn.shape[0]
    G = torch.empty((nblk, bs, bs), dtype=kn.dtype, device=kn.device)
    q = torch.empty(B, dtype=kn.dtype, device=kn.device)
    tr = torch.empty((), dtype=kn.dtype, device=kn.device) if trace else None
    _lib.check(_lib.lib().hgp_block_stats(_lib.dtype_code(kn.dtype), nd, (ctypes.c_int64 * nd)(*P.ndims),
                                          (ctypes.c_int64 * nd)(*blocks), _p(kn), B, _p(iv), _p(S), _p(G), _p(q),
                                          _p(tr), _lib.stream_ptr(kn.device)))
    return (G, q, tr) if trace else (G, q)


def _materialised(P, blocks, d, qm, iv, S):
    from hipgp_amd import _lib
    kn = P.apply(_lib.OP_RT, d)
    B = d.shape[0]
    G, q = _block_stats(P, blocks, kn, iv, S)
    out = torch.empty((B, 3), dtype=d.dtype, device=d.device)
    _lib.check(_lib.lib().hgp_meanfield_rowdots(_lib.dtype_code(d.dtype), _p(kn), B, P.Mprime, _p(qm),
                                                _p(torch.zeros_like(qm)), _p(out), _lib.stream_ptr(d.device)))
    out[:, 2] = q
    return out, G


def _compare(tag, dtype, got3, gotG, mat3, matG, truth3, truthG):
    floor = 1e-6 if dtype == torch.float32 else 1e-12
    f, m = got3.double().cpu().numpy(), mat3.double().cpu().numpy()
    for c in range(3):
        tn = np.linalg.norm(truth3[:, c])
        ef, em = np.linalg.norm(f[:, c] - truth3[:, c]), np.linalg.norm(m[:, c] - truth3[:, c])
        print(f"{tag} col {c}: streamed {ef / tn:.3e} materialised {em / tn:.3e}")
        assert ef <= 4 * em + floor * tn, (tag, c, ef / tn, em / tn)
    if gotG is not None:
        tn = np.linalg.norm(truthG)
        ef = np.linalg.norm(gotG.double().cpu().numpy() - truthG)
        em = np.linalg.norm(matG.double().cpu().numpy() - truthG)
        print(f"{tag} gram: streamed {ef / tn:.3e} materialised {em / tn:.3e}")
        assert ef <= 4 * em + floor * tn, (tag, "gram", ef / tn, em / tn)


def _plan(dims, dtype, col):
    from hipgp_amd.plan import ToeplitzPlan
    P = ToeplitzPlan(dims, dtype, DEV)
    P.set_column(torch.tensor(col, device=DEV, dtype=dtype))
    return P


def _check(dims, blocks, dtype, batches, nb_case=70):
    col, d, qm, iv, S, kb, dots = _case(dims, blocks, nb_case)
    P = _plan(dims, dtype, col)
    t = lambda a: torch.tensor(a, device=DEV, dtype=dtype)
    qmd, Sd = t(qm), t(S)
    for nb, piece in batches:
        dd, ivd = t(d[:nb]), t(iv[:nb])
        out, G = P.rt_block_stats(dd, blocks, qmd, S=Sd, ivar=ivd, piece_rhs=piece)
        again, G2 = P.rt_block_stats(dd, blocks, qmd, S=Sd, ivar=ivd, piece_rhs=piece)
        assert out.shape == (nb, 3) and G.shape == S.shape
        assert torch.equal(out, again) and torch.equal(G, G2), "rt_block_stats is not deterministic"
        mat3, matG = _materialised(P, blocks, dd, qmd, ivd, Sd)
        truthG = np.einsum("b,bki,bkj->kij", iv[:nb], kb[:nb], kb[:nb])
        _compare(f"rt_block_stats {_ID(dims)} {str(dtype)[6:]} B={nb} piece={piece}", dtype, out, G, mat3, matG,
                 dots[:nb], truthG)
    return P


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims,blocks", GRIDS, ids=[_ID(g) for g, _ in GRIDS])
def test_rt_block_stats_against_oracle(dims, blocks, dtype):
    _check(dims, blocks, dtype, BATCHES)


def test_rt_block_stats_fallback_route_fp64():
    """fp64 m = (4, 4200): R^T outside the row-pair kernels; blocks (3, 2), B = 3 in pieces of 2."""
    _check((4, 4200), (3, 2), torch.float64, [(3, 2)], nb_case=3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_rt_block_stats_optional_outputs(dtype):
    dims, blocks = (11, 9), (4, 4)
    col, d, qm, iv, S, kb, dots = _case(dims, blocks)
    P = _plan(dims, dtype, col)
    t = lambda a: torch.tensor(a, device=DEV, dtype=dtype)
    dd, qmd, Sd, ivd = t(d[:17]), t(qm), t(S), t(iv[:17])
    full, G = P.rt_block_stats(dd, blocks, qmd, S=Sd, ivar=ivd, piece_rhs=5)
    nog, none = P.rt_block_stats(dd, blocks, qmd, S=Sd, gram=False, piece_rhs=5)
    assert none is None and torch.equal(nog, full)            # the dots do not depend on the gram output
    noS, G2 = P.rt_block_stats(dd, blocks, qmd, ivar=ivd, piece_rhs=5)
    floor = 1e-6 if dtype == torch.float32 else 1e-12
    # the same sums in the same order from another instantiation (S not staged): rounding apart
    assert bool((noS[:, 2] == 0).all()) and rel_err(G2.double().cpu().numpy(), G.double().cpu().numpy()) < floor
    bare, _ = P.rt_block_stats(dd, blocks, qmd, gram=False, piece_rhs=5)
    assert bool((bare[:, 2] == 0).all())
    mat3, _ = _materialised(P, blocks, dd, qmd, ivd, Sd)
    truth = dots[:17].copy()
    truth[:, 2] = 0
    mat3[:, 2] = 0
    for got in (noS, bare):
        for c in range(2):
            tn = np.linalg.norm(truth[:, c])
            ef = np.linalg.norm(got.double().cpu().numpy()[:, c] - truth[:, c])
            em = np.linalg.norm(mat3.double().cpu().numpy()[:, c] - truth[:, c])
            assert ef <= 4 * em + floor * tn, (c, ef / tn, em / tn)


def test_rt_block_stats_empty_batch_and_errors():
    from hipgp_amd import _lib
    L = _lib.lib()
    f = L.hgp_rt_block_stats
    dims, blocks = (11, 9), (4, 4)
    col = _case(dims, blocks)[0]
    P = _plan(dims, torch.float64, col)
    dt = torch.float64
    d = torch.randn(2, P.M, dtype=dt, device=DEV)
    qm = torch.rand(P.Mprime, dtype=dt, device=DEV)
    iv = torch.rand(2, dtype=dt, device=DEV) + .5
    S = torch.rand(20, 16, 16, dtype=dt, device=DEV)
    o = torch.full((2, 3), 5., dtype=dt, device=DEV)
    G = torch.full((20, 16, 16), 7., dtype=dt, device=DEV)
    blk = (ctypes.c_int64 * 2)(*blocks)
    # nrhs = 0: the gram of no observations, nothing else written
    assert f(P._h, None, 0, blk, 0, None, None, None, _p(o), _p(G)) == 0
    torch.cuda.synchronize()
    assert bool((G == 0).all()) and bool((o == 5).all())
    o0, G0 = P.rt_block_stats(d[:0], blocks, qm, S=S, ivar=iv[:0])
    assert o0.shape == (0, 3) and G0.shape == (20, 16, 16) and bool((G0 == 0).all())
    # argument errors: nothing is written
    G.fill_(7.)
    assert f(P._h, _p(d), -1, blk, 0, _p(qm), _p(S), _p(iv), _p(o), _p(G)) == -1
    assert f(P._h, _p(d), 2, blk, -1, _p(qm), _p(S), _p(iv), _p(o), _p(G)) == -1
    assert f(P._h, _p(d), 2, None, 0, _p(qm), _p(S), _p(iv), _p(o), _p(G)) == -1
    assert f(P._h, None, 2, blk, 0, _p(qm), _p(S), _p(iv), _p(o), _p(G)) == -1
    assert f(P._h, _p(d), 2, blk, 0, None, _p(S), _p(iv), _p(o), _p(G)) == -1
    assert f(P._h, _p(d), 2, blk, 0, _p(qm), _p(S), _p(iv), None, _p(G)) == -1
    assert f(P._h, _p(d), 2, blk, 0, _p(qm), _p(S), None, _p(o), _p(G)) == -1          # a gram needs ivar
    # refused block shapes, with block_geom's message
    for bad in ((3, 4), (20, 16)):
        assert f(P._h, _p(d), 2, (ctypes.c_int64 * 2)(*bad), 0, _p(qm), _p(S), _p(iv), _p(o), _p(G)) == -4, bad
    assert b"hgp_rt_block_stats" in L.hgp_last_error()
    torch.cuda.synchronize()
    assert bool((G == 7).all()) and bool((o == 5).all()), "a refused call wrote an output"
    # a 1-D plan
    P1 = _plan((33,), dt, _column((33,)))
    d1 = torch.randn(2, 33, dtype=dt, device=DEV)
    assert f(P1._h, _p(d1), 2, (ctypes.c_int64 * 1)(4), 0, _p(qm), None, _p(iv), _p(o), _p(G)) == -4
    # no column set: a plan of its own (a pooled one may carry a column)
    h = ctypes.c_void_p()
    _lib.check(L.hgp_plan_create(0, 2, (ctypes.c_int64 * 2)(*dims), _lib.HGP_F64, 0, _lib.stream_ptr(torch.device(DEV, 0)),
                                 ctypes.byref(h)))
    try:
        assert f(h, _p(d), 2, blk, 0, _p(qm), _p(S), _p(iv), _p(o), _p(G)) == -3
    finally:
        L.hgp_plan_destroy(h)
    # the Python wrapper's own checks
    with pytest.raises(ValueError):
        P.rt_block_stats(d, blocks, qm[:-1], S=S, ivar=iv)
    with pytest.raises(ValueError):
        P.rt_block_stats(d, blocks, qm, S=S)                      # gram=True without ivar
    with pytest.raises(ValueError):
        P.rt_block_stats(d, (4,), qm, S=S, ivar=iv)
    with pytest.raises(TypeError):
        P.rt_block_stats(d, blocks, qm, S=S.float(), ivar=iv)
    with pytest.raises(_lib.HipgpError):
        P.rt_block_stats(d, (3, 4), qm, ivar=iv)


def test_plan_scratch_is_one_piece_and_trimmed():
    """Plan scratch grows by one piece of kn plus the row partials, whatever nrhs, and trim frees it."""
    dims, blocks = (21, 16), (10, 10)
    col, d, qm, iv, S, kb, dots = _case(dims, blocks)
    P = _plan(dims, torch.float32, col)
    t = lambda a: torch.tensor(a, device=DEV, dtype=torch.float32)
    P.trim()
    assert P.mem()["scratch"] == 0
    from hipgp_amd import _lib
    P.apply(_lib.OP_RT, t(d[:5]))                               # R^T's own workspaces at the piece's size
    base = P.mem()["scratch"]
    P.rt_block_stats(t(d), blocks, t(qm), S=t(S), ivar=t(iv), piece_rhs=5)
    extra = P.mem()["scratch"] - base
    piece = 5 * P.Mprime * 4
    part = 3 * 5 * (P.Mprime // 100) * 4
    print(f"plan scratch above R^T's: {extra} B (piece {piece} B, partials {part} B)")
    assert piece + part <= extra <= 2 * (piece + part)
    P.trim()
    assert P.mem()["scratch"] == 0


def test_block_stats_unchanged_by_the_streamed_route():
    """hgp_block_stats on a fixed input gives the same bits before and after the streamed route
    has run on the plan (no shared state disturbed)."""
    dims, blocks = (21, 16), (10, 10)
    col, d, qm, iv, S, kb, dots = _case(dims, blocks)
    for dtype in (torch.float32, torch.float64):
        P = _plan(dims, dtype, col)
        t = lambda a: torch.tensor(a, device=DEV, dtype=dtype)
        g = torch.Generator().manual_seed(4)
        kn = torch.randn(33, P.Mprime, generator=g, dtype=torch.float64).to(DEV, dtype)
        before = _block_stats(P, blocks, kn, t(iv[:33]), t(S), trace=True)
        P.rt_block_stats(t(d), blocks, t(qm), S=t(S), ivar=t(iv), piece_rhs=33)
        after = _block_stats(P, blocks, kn, t(iv[:33]), t(S), trace=True)
        for a, b in zip(before, after):
            assert torch.equal(a, b)


def test_tensor_rt_block_stats_refuses_grad():
    import ziggy.kernels as zk
    from ziggy.misc.toeplitz_tensor import ToeplitzTensor
    k = zk.SqExp(dtype=torch.float64)
    grids = [torch.linspace(-1, 1, m, dtype=torch.float64, device=DEV) for m in (9, 7)]
    T = ToeplitzTensor(grids, lambda x, y: k.forward(x, y, params=(1., .3)), batch_shape=(2,), jitter_val=1e-2)
    d = torch.randn(2, T.M, dtype=torch.float64, device=DEV)
    q = torch.rand(T._plan.Mprime, dtype=torch.float64, device=DEV)
    iv = torch.rand(2, dtype=torch.float64, device=DEV) + .5
    out, G = T.rt_block_stats(d, (4, 3), q, ivar=iv)
    kn = T._matmul_by_RT(d)
    from hipgp_amd.ziggy.hipgp import block_chunks
    kb = kn[:, block_chunks((16, 12), (4, 3))[0].to(DEV)]
    assert rel_err(out[:, :2].cpu().numpy(), torch.stack([kn @ q, (kn * kn).sum(1)], dim=1).cpu().numpy()) < 1e-12
    assert rel_err(G.cpu().numpy(), torch.einsum("b,bki,bkj->kij", iv, kb, kb).cpu().numpy()) < 1e-12
    with pytest.raises(RuntimeError):
        T.rt_block_stats(d.clone().requires_grad_(True), (4, 3), q, ivar=iv)
    with pytest.raises(RuntimeError):
        T.rt_block_stats(d, (4, 3), q.clone().requires_grad_(True), ivar=iv)


# ---- model level ----------------------------------------------------------------------------------
PIECE = 6        # G11: 48 observations in 8 pieces, G12: 40 in 7; predict's 20 in 4


def _grads(mod):
    return mod.global_theta1.grad.clone(), mod.global_theta2.grad.clone()


def _count_hooks(mod):
    import ziggy.hipgp as hg
    calls = []
    fit, pred = hg.BlockToeplitzGP.streamed_fit_stats, hg.BlockToeplitzGP.streamed_predict_stats
    mod.streamed_fit_stats = lambda *a, **k: (calls.append("fit"), fit(mod, *a, **k))[1]
    mod.streamed_predict_stats = lambda *a, **k: (calls.append("predict"), pred(mod, *a, **k))[1]
    return calls


@pytest.mark.parametrize("name", ["G11", "G12"])
def test_block_model_streamed_fp64(name):
    """The bounds tests/test_block_gpu.py::test_block_model_reference_fp64 holds the materialised
    path to."""
    mod, fx = block_model(name, device=DEV)
    mod.kn_piece_rhs = PIECE
    calls = _count_hooks(mod)
    x = torch.tensor(fx["xobs"], device=DEV)
    y = torch.tensor(fx["yobs"], device=DEV)
    nstd = noise_of(fx, device=DEV)
    elbo = mod.elbo_and_grad(x, y, noise_std_batch=nstd, maxiter_cg=20, streamed=True)
    assert calls == ["fit"]
    print(f"{name} streamed fp64: elbo {abs(float(elbo) - float(fx['elbo'])) / abs(float(fx['elbo'])):.3e} "
          f"theta1 {rel_err(mod.global_theta1.grad.cpu().numpy(), fx['theta1_grad']):.3e} "
          f"theta2 {rel_err(mod.global_theta2.grad.cpu().numpy(), fx['theta2_grad']):.3e}")
    assert abs(float(elbo) - float(fx["elbo"])) < 1e-8 * abs(float(fx["elbo"]))
    assert mod.global_theta1.grad.shape == fx["theta1_grad"].shape
    assert mod.global_theta2.grad.shape == fx["theta2_grad"].shape
    assert rel_err(mod.global_theta1.grad.cpu().numpy(), fx["theta1_grad"]) < 1e-7
    assert rel_err(mod.global_theta2.grad.cpu().numpy(), fx["theta2_grad"]) < 1e-7
    mu, sig = mod.predict(x[:20], maxiter_cg=50, streamed=True)
    assert calls == ["fit", "predict"]
    assert mu.shape == fx["pred_mu"].shape and sig.shape == fx["pred_sig"].shape
    assert rel_err(mu.numpy(), fx["pred_mu"]) < 1e-7
    assert rel_err(sig.numpy(), fx["pred_sig"]) < 1e-7


@pytest.mark.parametrize("name", ["G11", "G12"])
def test_block_model_streamed_fp32(name):
    """fp32 against the fp64 reference: no worse than 4x the reference's own fp32 error on the theta
    gradients and the ELBO (the rule of tests/test_block_gpu.py::test_block_model_fp32)."""
    fx32, fx64 = load(name, "f32"), load(name, "f64")
    mod, _ = block_model(name, tag="f32", dtype=torch.float32, device=DEV)
    mod.kn_piece_rhs = PIECE
    x = torch.tensor(fx32["xobs"], device=DEV)
    y = torch.tensor(fx32["yobs"], device=DEV)
    nstd = noise_of(fx32, dtype=torch.float32, device=DEV)
    elbo = float(mod.elbo_and_grad(x, y, noise_std_batch=nstd, maxiter_cg=20, streamed=True))
    for key, mine in (("theta1_grad", mod.global_theta1.grad), ("theta2_grad", mod.global_theta2.grad)):
        e_me = np.linalg.norm(mine.double().cpu().numpy() - fx64[key])
        e_ref = np.linalg.norm(fx32[key].astype(np.float64) - fx64[key])
        print(f"{name} streamed fp32 {key}: {e_me:.3e} (reference fp32 {e_ref:.3e})")
        assert e_me <= 4 * e_ref + 1e-6 * np.linalg.norm(fx64[key]), (key, e_me, e_ref)
    e_ref = abs(float(fx32["elbo"]) - float(fx64["elbo"]))
    assert abs(elbo - float(fx64["elbo"])) <= 4 * e_ref + 1e-6 * abs(float(fx64["elbo"]))


def test_streamed_off_and_hyper_gradient_cases_are_the_materialised_path(monkeypatch):
    monkeypatch.delenv("HGP_BLOCK_STREAMED", raising=False)
    mod, fx = block_model("G11", device=DEV)
    calls = _count_hooks(mod)
    x = torch.tensor(fx["xobs"], device=DEV)
    y = torch.tensor(fx["yobs"], device=DEV)
    e0 = mod.elbo_and_grad(x, y, maxiter_cg=20)
    g0 = _grads(mod)
    e1 = mod.elbo_and_grad(x, y, maxiter_cg=20, streamed=False)
    g1 = _grads(mod)
    assert torch.equal(e0, e1) and torch.equal(g0[0], g1[0]) and torch.equal(g0[1], g1[1])
    p0, p1 = mod.predict(x[:20]), mod.predict(x[:20], streamed=False)
    assert torch.equal(p0[0], p1[0]) and torch.equal(p0[1], p1[1])
    assert not calls
    # learn_kernel: the autograd ELBO needs kn, so streamed=True never reaches the hook
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    dt = torch.float64
    grids = [torch.tensor(fx[f"grid{i}"], dtype=dt) for i in range(2)]
    lk = hg.BlockToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, num_obs=int(fx["num_obs"]),
                            block_sizes=[int(b) for b in fx["blocks"]], sig2_init=float(fx["params"][0]),
                            ell_init=float(fx["params"][1]), noise2_init=float(fx["noise2"]), learn_kernel=True, dtype=dt)
    with torch.no_grad():
        lk.global_theta1.copy_(torch.tensor(fx["theta1"], dtype=dt))
        lk.global_theta2.copy_(torch.tensor(fx["theta2"], dtype=dt))
    lk = lk.cuda_params(0)
    assert lk.hyper_grad_needed(None)
    calls = _count_hooks(lk)
    res = []
    for streamed in (False, True):
        for p in (lk.log_sig2, lk.log_ell):
            p.grad = None
        elbo = lk.elbo_and_grad(x, y, maxiter_cg=20, streamed=streamed)
        elbo.backward()
        res.append((elbo.detach().clone(), lk.log_sig2.grad.clone(), lk.log_ell.grad.clone(), *_grads(lk)))
    assert not calls, "the streamed hook ran although the ELBO needs kn"
    for u, v in zip(*res):
        assert torch.equal(u, v)


_ENV_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
from block_cases import block_model
import ziggy.hipgp as hg
mod, fx = block_model("G11", device="cuda")
x = torch.tensor(fx["xobs"], device="cuda")
y = torch.tensor(fx["yobs"], device="cuda")
calls = []
fit, pred = hg.BlockToeplitzGP.streamed_fit_stats, hg.BlockToeplitzGP.streamed_predict_stats
hg.BlockToeplitzGP.streamed_fit_stats = lambda self, *a, **k: (calls.append("fit"), fit(self, *a, **k))[1]
hg.BlockToeplitzGP.streamed_predict_stats = lambda self, *a, **k: (calls.append("predict"), pred(self, *a, **k))[1]
env = mod.elbo_and_grad(x, y, maxiter_cg=20)
g_env = mod.global_theta1.grad.clone()
on = mod.elbo_and_grad(x, y, maxiter_cg=20, streamed=True)
assert calls == ["fit", "fit"], calls
assert torch.equal(env, on) and torch.equal(g_env, mod.global_theta1.grad)
mod.elbo_and_grad(x, y, maxiter_cg=20, streamed=False)
assert calls == ["fit", "fit"], calls
p_env = mod.predict(x[:20])
p_on = mod.predict(x[:20], streamed=True)
assert calls == ["fit", "fit", "predict", "predict"], calls
assert torch.equal(p_env[0], p_on[0]) and torch.equal(p_env[1], p_on[1])
print("ENV_STREAMED_OK")
"""


def test_env_knob_selects_streamed_path():
    env = dict(os.environ, HGP_BLOCK_STREAMED="1")
    code = _ENV_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ENV_STREAMED_OK" in r.stdout, r.stdout + r.stderr


def test_elbo_and_grad_streamed_allocates_no_kn():
    """(256, 256) fp32, blocks (2, 2), B = 128, kn_piece_rhs = 16: kn would be 128 x 510^2 x 4 B =
    133 MB.  torch's peak during the streamed step stays under half of that above the level before
    the call; the materialised step exceeds it (so the measurement sees the difference).

    The streamed step holds Knm (33.6 MB), solved in place, the gram and the block-shaped
    temporaries of the update (65025 x 4 x 4 values, 4.2 MB each) and a handful of M'-vectors, far
    below the 66.6 MB bound; the 16-RHS piece of kn (16.6 MB) is plan scratch, outside torch."""
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    dt = torch.float32
    B = 128
    grids = [torch.linspace(-1, 1, 256, dtype=dt) for _ in range(2)]
    mod = hg.BlockToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, num_obs=B, block_sizes=[2, 2], sig2_init=1.,
                             ell_init=.05, noise2_init=.01, learn_kernel=False, dtype=dt).cuda_params(0)
    mod.kn_piece_rhs = 16
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, 2, generator=g, dtype=dt) * 1.8 - .9).to(DEV)
    y = torch.randn(B, 1, generator=g, dtype=dt).to(DEV)
    kn_bytes = B * mod.Mprime * 4

    def peak(streamed):
        mod.elbo_and_grad(x, y, maxiter_cg=5, streamed=streamed)    # warm-up: plans, pools, .grad
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        mod.elbo_and_grad(x, y, maxiter_cg=5, streamed=streamed)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    ps, pm = peak(True), peak(False)
    print(f"elbo_and_grad peak above base: streamed {ps / 2**20:.1f} MiB, materialised {pm / 2**20:.1f} MiB, "
          f"kn {kn_bytes / 2**20:.1f} MiB")
    assert pm > kn_bytes, (pm, kn_bytes)
    assert ps < kn_bytes / 2, (ps, kn_bytes)
