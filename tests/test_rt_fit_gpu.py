"""hgp_rt_fit_stats / ToeplitzPlan.rt_fit_stats / elbo_and_grad(fused=True): the sums the mean-field
natural-gradient step takes from kn = R^T d (`hipgp.py:234-250`: the three row dots and
lam[j] = sum_n ivar_n kn_nj^2) from the R^T row-inverse pass's EPI_LAM epilogue, kn never stored,
and dm = -sum_n bdiff_n kn_n as one single-RHS R^T of -sum_n bdiff_n d_n.

Operator level: truth is the fp64 oracle's R^T followed by numpy sums; the yardstick is the
materialised path on the same inputs (plan.apply(RT), then hgp_meanfield_rowdots and
hgp_meanfield_cols).  Per column of out3 (norm over the batch) and for lam (norm over M') the
fused error may be at most 4x the materialised path's, plus a floor of 1e-6 (fp32) / 1e-12 (fp64)
x |truth|.  The grids, and which k_row_inv_t<T, H, EPI, G> branch each reaches, are
those of tests/test_rt_stats_gpu.py; (32, 24) with B = 17 spans both streams (two lam
accumulators), a full 8-RHS chunk and a tail.  Fallbacks (R^T into plan scratch a piece at a time,
rows and columns of each piece reduced): 1-D (257,), fp64 (4, 4200) and (5500, 4)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_cases import load, rel_err
from oracle import ziggy_oracle as zo
from test_rt_stats_gpu import FALLBACKS, GRIDS, _ID, _column, _case as _stats_case, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CASE = {}


def _case(dims):
    """test_rt_stats_gpu's column and RandomState(11) inputs, plus ivar = rand + 0.5 and the fp64
    truth of out3 and (per batch size) lam; computed once, read-only."""
    if dims not in _CASE:
        col, d, qm, qS, truth3 = _stats_case(dims)
        rs = np.random.RandomState(11)
        nb = d.shape[0]
        rs.randn(nb, d.shape[1]); rs.randn(qm.shape[0]); rs.rand(qS.shape[0])    # the draws of that file
        iv = rs.rand(nb) + 0.5
        kn = zo.ToeplitzOracle(col, dims).matmul_RT(d).reshape(nb, -1)
        lam = {b: (iv[:b, None] * kn[:b] ** 2).sum(0) for b in ((1, 3, 17) if nb == 17 else (1, 3))}
        iv.setflags(write=False)
        _CASE[dims] = (col, d, qm, qS, iv, truth3, lam)
    return _CASE[dims]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _materialised(P, d, qm, qS, iv):
    from hipgp_amd import _lib
    kn = P.apply(_lib.OP_RT, d)
    B = d.shape[0]
    out = torch.empty((B, 3), dtype=d.dtype, device=d.device)
    lam = torch.empty(P.Mprime, dtype=d.dtype, device=d.device)
    dm = torch.empty(P.Mprime, dtype=d.dtype, device=d.device)
    code, st = _lib.dtype_code(d.dtype), _lib.stream_ptr(d.device)
    _lib.check(_lib.lib().hgp_meanfield_rowdots(code, _p(kn), B, P.Mprime, _p(qm), _p(qS), _p(out), st))
    _lib.check(_lib.lib().hgp_meanfield_cols(code, _p(kn), B, P.Mprime, _p(iv), _p(torch.zeros_like(iv)), _p(lam),
                                             _p(dm), st))
    return out, lam


def _check(dims, dtype, batches):
    from hipgp_amd.plan import ToeplitzPlan
    col, d, qm, qS, iv, truth3, truth_lam = _case(dims)
    P = ToeplitzPlan(dims, dtype, DEV)
    P.set_column(torch.tensor(col, device=DEV, dtype=dtype))
    t = lambda a: torch.tensor(a, device=DEV, dtype=dtype)
    qmd, qSd = t(qm), t(qS)
    floor = 1e-6 if dtype == torch.float32 else 1e-12
    tag = f"rt_fit_stats {_ID(dims)} {str(dtype)[6:]}"
    for nb in batches:
        dd, ivd = t(d[:nb]), t(iv[:nb])
        fused, lam = P.rt_fit_stats(dd, qmd, qSd, ivd)
        again, lam2 = P.rt_fit_stats(dd, qmd, qSd, ivd)
        mat, mlam = _materialised(P, dd, qmd, qSd, ivd)
        assert fused.shape == (nb, 3) and lam.shape == (P.Mprime,)
        assert torch.equal(fused, again) and torch.equal(lam, lam2), "rt_fit_stats is not deterministic"
        f, m = fused.double().cpu().numpy(), mat.double().cpu().numpy()
        for c in range(3):
            tn = np.linalg.norm(truth3[:nb, c])
            ef, em = np.linalg.norm(f[:, c] - truth3[:nb, c]), np.linalg.norm(m[:, c] - truth3[:nb, c])
            print(f"{tag} B={nb} col {c}: fused {ef / tn:.3e} materialised {em / tn:.3e}")
            assert ef <= 4 * em + floor * tn, (dims, dtype, nb, c, ef / tn, em / tn)
        tl = truth_lam[nb]
        tn = np.linalg.norm(tl)
        ef = np.linalg.norm(lam.double().cpu().numpy() - tl)
        em = np.linalg.norm(mlam.double().cpu().numpy() - tl)
        print(f"{tag} B={nb} lam: fused {ef / tn:.3e} materialised {em / tn:.3e}")
        assert ef <= 4 * em + floor * tn, (dims, dtype, nb, "lam", ef / tn, em / tn)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims", GRIDS, ids=_ID)
def test_rt_fit_stats_against_oracle(dims, dtype):
    _check(dims, dtype, (1, 3, 17) if dims == (32, 24) else (1, 3))


@pytest.mark.parametrize("dims,dtype", FALLBACKS, ids=[f"{_ID(g)}-{str(t)[6:]}" for g, t in FALLBACKS])
def test_rt_fit_stats_fallback_routes(dims, dtype):
    _check(dims, dtype, (1, 3))


def test_rt_fit_stats_argument_errors():
    from hipgp_amd import _lib
    from hipgp_amd.plan import ToeplitzPlan
    L = _lib.lib()
    P = ToeplitzPlan((9, 7), torch.float32, DEV)
    P.set_column(torch.tensor(_column((9, 7)), device=DEV, dtype=torch.float32))
    d = torch.randn(2, P.M, device=DEV)
    q = torch.rand(P.Mprime, device=DEV)
    iv = torch.rand(2, device=DEV)
    o = torch.zeros(2, 3, device=DEV)
    lam = torch.ones(P.Mprime, device=DEV)
    f = L.hgp_rt_fit_stats
    assert f(P._h, _p(d), -1, _p(q), _p(q), _p(iv), _p(o), _p(lam)) == -1
    assert f(P._h, None, 2, _p(q), _p(q), _p(iv), _p(o), _p(lam)) == -1
    assert f(P._h, _p(d), 2, _p(q), None, _p(iv), _p(o), _p(lam)) == -1
    assert f(P._h, _p(d), 2, _p(q), _p(q), None, _p(o), _p(lam)) == -1
    assert f(P._h, _p(d), 2, _p(q), _p(q), _p(iv), None, _p(lam)) == -1
    assert f(P._h, _p(d), 2, _p(q), _p(q), _p(iv), _p(o), None) == -1
    assert bool((lam == 1).all()), "a refused call wrote lam"
    assert f(P._h, None, 0, None, None, None, None, _p(lam)) == 0         # nrhs = 0: the empty sum
    torch.cuda.synchronize()
    assert bool((lam == 0).all())
    o0, l0 = P.rt_fit_stats(d[:0], q, q, iv[:0])
    assert o0.shape == (0, 3) and bool((l0 == 0).all())
    with pytest.raises(ValueError):
        P.rt_fit_stats(d, q[:-1], q, iv)
    with pytest.raises(ValueError):
        P.rt_fit_stats(d, q, q, iv[:1])
    with pytest.raises(TypeError):
        P.rt_fit_stats(d, q, q.double(), iv)
    with pytest.raises(TypeError):
        P.rt_fit_stats(d, q, q, iv.double())


def test_tensor_rt_fit_stats_refuses_grad():
    import ziggy.kernels as zk
    from ziggy.misc.toeplitz_tensor import ToeplitzTensor
    k = zk.SqExp(dtype=torch.float64)
    grids = [torch.linspace(-1, 1, m, dtype=torch.float64, device=DEV) for m in (9, 7)]
    T = ToeplitzTensor(grids, lambda x, y: k.forward(x, y, params=(1., .3)), batch_shape=(2,), jitter_val=1e-2)
    d = torch.randn(2, T.M, dtype=torch.float64, device=DEV)
    q = torch.rand(T._plan.Mprime, dtype=torch.float64, device=DEV)
    iv = torch.rand(2, dtype=torch.float64, device=DEV) + .5
    out, lam = T.rt_fit_stats(d, q, q, iv)
    kn = T._matmul_by_RT(d)
    ref = torch.stack([kn @ q, (kn * kn).sum(1), (kn * kn) @ q], dim=1)
    assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 1e-12
    assert rel_err(lam.cpu().numpy(), (iv[:, None] * kn * kn).sum(0).cpu().numpy()) < 1e-12
    with pytest.raises(RuntimeError):
        T.rt_fit_stats(d.clone().requires_grad_(True), q, q, iv)


# ---- model level ----------------------------------------------------------------------------------
def _grads(mod):
    return mod.global_theta1.grad.clone(), mod.global_theta2.grad.clone()


def test_elbo_and_grad_fused_G5_fp64():
    fx = load("G5", "f64")
    mod = _model(fx, torch.float64)
    x = torch.tensor(fx["xobs"], device=DEV)
    y = torch.tensor(fx["yobs"], device=DEV)
    elbo = mod.elbo_and_grad(x, y, maxiter_cg=20, fused=True)
    assert abs(float(elbo) - float(fx["elbo"])) < 1e-8 * abs(float(fx["elbo"]))
    assert mod.global_theta1.grad.shape == fx["theta1_grad"].shape
    assert rel_err(mod.global_theta1.grad.cpu().numpy(), fx["theta1_grad"]) < 1e-7
    assert rel_err(mod.global_theta2.grad.cpu().numpy(), fx["theta2_grad"]) < 1e-7
    # fused=False and the default are today's path
    e0 = mod.elbo_and_grad(x, y, maxiter_cg=20)
    g0 = _grads(mod)
    e1 = mod.elbo_and_grad(x, y, maxiter_cg=20, fused=False)
    g1 = _grads(mod)
    assert torch.equal(e0, e1) and torch.equal(g0[0], g1[0]) and torch.equal(g0[1], g1[1])


def test_elbo_and_grad_fused_G5_fp32():
    """Each gradient no worse than 4x the reference's own fp32-vs-fp64 golden error, plus the 1e-6
    floor."""
    fx32, fx64 = load("G5", "f32"), load("G5", "f64")
    mod = _model(fx32, torch.float32)
    x = torch.tensor(fx32["xobs"], device=DEV)
    y = torch.tensor(fx32["yobs"], device=DEV)
    mod.elbo_and_grad(x, y, maxiter_cg=20, fused=True)
    for got, key in ((mod.global_theta1.grad, "theta1_grad"), (mod.global_theta2.grad, "theta2_grad")):
        ref = fx64[key].astype(np.float64)
        e_me = np.linalg.norm(got.double().cpu().numpy().reshape(ref.shape) - ref)
        e_ref = np.linalg.norm(fx32[key].astype(np.float64) - ref)
        print(f"elbo_and_grad fused fp32 {key}: {e_me:.3e} (reference fp32 {e_ref:.3e})")
        assert e_me <= 4 * e_ref + 1e-6 * np.linalg.norm(ref), (key, e_me, e_ref)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_fit_stats_dict(dtype):
    """Twice the same bits; dm_sum (the linear route) against the fp64 truth within 4x the error of
    batch_stats(kn, ...) plus the floor, norm-wise over M', and lam_sum the same way."""
    tag = "f64" if dtype == torch.float64 else "f32"
    fx, fx64 = load("G5", tag), load("G5", "f64")
    mod = _model(fx, dtype)
    x = torch.tensor(fx["xobs"], device=DEV)
    y = torch.tensor(fx["yobs"], device=DEV)

    def run():
        Knm, kd = mod._make_grams(x)
        return mod.fit_stats(Knm, y, kd, None, maxiter_cg=20)

    a, b = run(), run()
    assert set(a) == {"an_sum", "lam_sum", "dm_sum", "n"} and a["n"] == 64
    for k in ("an_sum", "lam_sum", "dm_sum"):
        assert torch.equal(a[k], b[k]), k
    Knm, kd = mod._make_grams(x)
    mat = mod.batch_stats(mod.compute_kn(Knm, maxiter_cg=20), y, kd)
    assert a["lam_sum"].shape == mat["lam_sum"].shape and a["dm_sum"].shape == mat["dm_sum"].shape
    # fp64 truth from the reference's kn and the fp64 variational parameters
    import ziggy.hipgp as hg
    m64 = _model(fx64, torch.float64)
    kn64 = torch.tensor(fx64["kn"], device=DEV)
    truth = hg.MeanFieldToeplitzGP.batch_stats(m64, kn64, torch.tensor(fx64["yobs"], device=DEV),
                                               torch.tensor(fx64["Knn_diag"], device=DEV))
    floor = 1e-6 if dtype == torch.float32 else 1e-12
    for k in ("dm_sum", "lam_sum"):
        tr = truth[k].double().cpu().numpy().reshape(-1)
        ef = np.linalg.norm(a[k].double().cpu().numpy().reshape(-1) - tr)
        em = np.linalg.norm(mat[k].double().cpu().numpy().reshape(-1) - tr)
        tn = np.linalg.norm(tr)
        print(f"fit_stats {tag} {k}: fused {ef / tn:.3e} materialised {em / tn:.3e}")
        assert ef <= 4 * em + floor * tn, (k, ef / tn, em / tn)


def test_learn_kernel_takes_the_materialised_path():
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    fx = load("G5", "f64")
    dt = torch.float64
    grids = [torch.tensor(fx["grid0"], dtype=dt), torch.tensor(fx["grid1"], dtype=dt)]
    mod = hg.MeanFieldToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, num_obs=64, sig2_init=1., ell_init=.1,
                                 noise2_init=.01, learn_kernel=True, dtype=dt)
    with torch.no_grad():
        mod.global_theta1.copy_(torch.tensor(fx["theta1"], dtype=dt))
        mod.global_theta2.copy_(torch.tensor(fx["theta2"], dtype=dt))
    mod = mod.cuda_params(0)
    x = torch.tensor(fx["xobs"], device=DEV)
    y = torch.tensor(fx["yobs"], device=DEV)
    assert mod.hyper_grad_needed(None)
    calls = []
    orig = hg.MeanFieldToeplitzGP.fit_stats
    mod.fit_stats = lambda *a, **k: (calls.append(1), orig(mod, *a, **k))[1]
    res = []
    for fused in (False, True):
        for p in (mod.log_sig2, mod.log_ell):
            p.grad = None
        elbo = mod.elbo_and_grad(x, y, maxiter_cg=20, fused=fused)
        elbo.backward()
        res.append((elbo.detach().clone(), mod.log_sig2.grad.clone(), mod.log_ell.grad.clone(), *_grads(mod)))
    assert not calls, "the fused hook ran although the ELBO needs kn"
    for u, v in zip(*res):
        assert torch.equal(u, v)


def test_block_family_falls_back():
    from block_cases import block_model, noise_of
    mod, fx = block_model("G11", device=DEV)
    x = torch.tensor(fx["xobs"], device=DEV)
    y = torch.tensor(fx["yobs"], device=DEV)
    ns = noise_of(fx, device=DEV)
    ea = mod.elbo_and_grad(x, y, ns, maxiter_cg=20, fused=False)
    ga = _grads(mod)
    eb = mod.elbo_and_grad(x, y, ns, maxiter_cg=20, fused=True)
    gb = _grads(mod)
    assert torch.equal(ea, eb) and torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])


_ENV_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
from golden_cases import load
import test_rt_stats_gpu as t
fx = load("G5", "f64")
mod = t._model(fx, torch.float64)
x = torch.tensor(fx["xobs"], device="cuda")
y = torch.tensor(fx["yobs"], device="cuda")
calls = []
orig = type(mod).fit_stats
type(mod).fit_stats = lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1]
env = mod.elbo_and_grad(x, y, maxiter_cg=20)
g_env = mod.global_theta1.grad.clone()
fused = mod.elbo_and_grad(x, y, maxiter_cg=20, fused=True)
assert len(calls) == 2, calls
assert torch.equal(env, fused) and torch.equal(g_env, mod.global_theta1.grad)
mod.elbo_and_grad(x, y, maxiter_cg=20, fused=False)
assert len(calls) == 2, calls
print("ENV_FUSED_OK")
"""


def test_env_knob_selects_fused_path():
    env = dict(os.environ, HGP_FIT_FUSED="1")
    code = _ENV_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ENV_FUSED_OK" in r.stdout, r.stdout + r.stderr


def test_elbo_and_grad_fused_allocates_no_kn():
    """(256, 256) fp32, B = 128: kn would be 128 x 510^2 x 4 B = 133 MB.  torch's peak during the
    fused step stays under half of that above the level before the call; the materialised step
    exceeds it (so the measurement sees the difference).

    The fused step holds Knm (33.6 MB), solved in place, and a handful of M'-vectors (qm, qS, lam,
    dm, the gradients' temporaries: about 1 MB each), far below the 66.6 MB bound."""
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    dt = torch.float32
    B = 128
    grids = [torch.linspace(-1, 1, 256, dtype=dt) for _ in range(2)]
    mod = hg.MeanFieldToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, num_obs=B, sig2_init=1., ell_init=.05,
                                 noise2_init=.01, learn_kernel=False, dtype=dt).cuda_params(0)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, 2, generator=g, dtype=dt) * 1.8 - .9).to(DEV)
    y = torch.randn(B, 1, generator=g, dtype=dt).to(DEV)
    kn_bytes = B * mod.Mprime * 4

    def peak(fused):
        mod.elbo_and_grad(x, y, maxiter_cg=5, fused=fused)          # warm-up: plans, pools, .grad
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        mod.elbo_and_grad(x, y, maxiter_cg=5, fused=fused)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    pf, pm = peak(True), peak(False)
    print(f"elbo_and_grad peak above base: fused {pf / 2**20:.1f} MiB, materialised {pm / 2**20:.1f} MiB, "
          f"kn {kn_bytes / 2**20:.1f} MiB")
    assert pm > kn_bytes, (pm, kn_bytes)
    assert pf < kn_bytes / 2, (pf, kn_bytes)
