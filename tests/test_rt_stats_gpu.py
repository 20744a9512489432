"""hgp_rt_stats / ToeplitzPlan.rt_stats / predict(fused=True): the three numbers prediction takes
from kn = R^T d (kn.qm, |kn|^2, kn^2.qS; `hipgp.py:436-443`) from the R^T row-inverse pass's
EPI_STATS epilogue, kn never stored.

Operator level: truth is the fp64 oracle's R^T followed by three numpy dots; the yardstick is the
materialised path on the same inputs (plan.apply(RT), then hgp_meanfield_rowdots).  Per column of
out3 the fused norm-wise error over the batch may be at most 4x the materialised path's, plus a
floor of 1e-6 (fp32) / 1e-12 (fp64) x |truth| (the floor of test_model_gpu.py:58).

Which grid reaches which k_row_inv_t<T, H, EPI_STATS, G> (H = L_R[last] / 2; L_R per axis is the
power of two >= 4m - 4, or the shortest 2^k / 3 * 2^k >= 3m - 3 where that grid is below 0.6 of it;
TT = H / P threads per row pair, P = 16 fp32 / 8 fp64 for 2^k, 12 for 3 * 2^k, 24 grouped 3 * 2^k):
  (32, 24)      H = 48  (3 * 2^k), TT = 4: several pairs per wave (fp32) / plain (fp64); B = 17 here
                is two 8-RHS chunks on one stream and one on the other plus a 1-RHS tail
  (8, 6, 5)     H = 8, 3-D planes (q % out[0] addressing of qm / qS), rows shorter than a wave
  (64, 64)      H = 96  (3 * 2^k), TT = 8
  (4, 20)       H = 32, TT = 2 / 4; out_len = 38 > H: both halves reach the output
  (4, 128)      H = 256, TT = 16 / 32
  (4, 200)      H = 512, TT = 32 / 64 (fp64: the wave-uniform buffer branch)
  (4, 400)      H = 1024, TT = 64: the wave-uniform buffer branch, one wave per pair
  (4, 1024)     H = 2048, fp32 G = 2 (grouped columns), TT = 128
  (4, 2500)     H = 4096, fp32 G = 4 (quad order), TT = 256, complex spectrum
  (8, 700)      H = 1536 (3 * 2^k, ungrouped), TT = 128
  (8, 2740)     H = 6144 (3 * 2^k), fp32 G = 4, P = 24, TT = 256: the long mixed-radix rows
  (4, 6, 1024)  3-D, H = 1536 (3 * 2^k), TT = 128
Fallbacks (R^T into plan scratch a piece at a time + hgp_meanfield_rowdots): 1-D (257,), and in
fp64 (4, 4200) (rows of H = 8192 do not fit one CU's LDS: the generic sequence) and (5500, 4)
(L_R / 2 > 8192: the full-grid route)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_cases import load, rel_err
from oracle import ziggy_oracle as zo

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = [(32, 24), (8, 6, 5), (64, 64), (4, 20), (4, 128), (4, 200), (4, 400), (4, 1024), (4, 2500), (8, 700),
         (8, 2740), (4, 6, 1024)]
FALLBACKS = [((257,), torch.float32), ((257,), torch.float64), ((4, 4200), torch.float64), ((5500, 4), torch.float64)]
_ID = lambda g: "x".join(str(m) for m in g)


def _column(dims):
    grids = [np.linspace(-1, 1, m) for m in dims]
    ell = 40.0 / max(max(dims), 80)
    return zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("matern", x, y, (1.0, ell), nu=1.5), 0.1)


_CASE = {}


def _case(dims):
    """column, oracle and fp64 inputs / truth of one grid, computed once (read-only)."""
    if dims not in _CASE:
        col = _column(dims)
        O = zo.ToeplitzOracle(col, dims)
        rs = np.random.RandomState(11)
        nb = 17 if dims == (32, 24) else 3
        d = rs.randn(nb, O.M)
        qm = rs.randn(O.Mp)
        qS = rs.rand(O.Mp) + 0.1
        kn = O.matmul_RT(d).reshape(nb, -1)
        truth = np.stack([kn @ qm, (kn * kn).sum(1), (kn * kn) @ qS], axis=1)
        for a in (d, qm, qS, truth):
            a.setflags(write=False)
        _CASE[dims] = (col, d, qm, qS, truth)
    return _CASE[dims]


def _materialised(P, d, qm, qS):
    from hipgp_amd import _lib
    kn = P.apply(_lib.OP_RT, d)
    out = torch.empty((d.shape[0], 3), dtype=d.dtype, device=d.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().hgp_meanfield_rowdots(_lib.dtype_code(d.dtype), p(kn), d.shape[0], P.Mprime, p(qm), p(qS),
                                                p(out), _lib.stream_ptr(d.device)))
    return out


def _check(dims, dtype, batches):
    from hipgp_amd.plan import ToeplitzPlan
    col, d, qm, qS, truth = _case(dims)
    P = ToeplitzPlan(dims, dtype, DEV)
    P.set_column(torch.tensor(col, device=DEV, dtype=dtype))
    t = lambda a: torch.tensor(a, device=DEV, dtype=dtype)
    qmd, qSd = t(qm), t(qS)
    floor = 1e-6 if dtype == torch.float32 else 1e-12
    for nb in batches:
        dd = t(d[:nb])
        fused = P.rt_stats(dd, qmd, qSd)
        again = P.rt_stats(dd, qmd, qSd)
        mat = _materialised(P, dd, qmd, qSd)
        assert fused.shape == (nb, 3)
        assert torch.equal(fused, again), "rt_stats is not deterministic"
        f, m = fused.double().cpu().numpy(), mat.double().cpu().numpy()
        for c in range(3):
            tn = np.linalg.norm(truth[:nb, c])
            ef, em = np.linalg.norm(f[:, c] - truth[:nb, c]), np.linalg.norm(m[:, c] - truth[:nb, c])
            print(f"rt_stats {_ID(dims)} {str(dtype)[6:]} B={nb} col {c}: fused {ef / tn:.3e} materialised {em / tn:.3e}")
            assert ef <= 4 * em + floor * tn, (dims, dtype, nb, c, ef / tn, em / tn)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims", GRIDS, ids=_ID)
def test_rt_stats_against_oracle(dims, dtype):
    """B = 1 and 3 on every grid; (32, 24) also B = 17: more than the plan's 8-RHS R^T chunk per
    stream, and not a multiple of it."""
    _check(dims, dtype, (1, 3, 17) if dims == (32, 24) else (1, 3))


@pytest.mark.parametrize("dims,dtype", FALLBACKS, ids=[f"{_ID(g)}-{str(t)[6:]}" for g, t in FALLBACKS])
def test_rt_stats_fallback_routes(dims, dtype):
    _check(dims, dtype, (1, 3))


def test_rt_stats_argument_errors():
    from hipgp_amd import _lib
    from hipgp_amd.plan import ToeplitzPlan
    L = _lib.lib()
    P = ToeplitzPlan((9, 7), torch.float32, DEV)
    P.set_column(torch.tensor(_column((9, 7)), device=DEV, dtype=torch.float32))
    d = torch.randn(2, P.M, device=DEV)
    q = torch.rand(P.Mprime, device=DEV)
    o = torch.zeros(2, 3, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.hgp_rt_stats(P._h, p(d), -1, p(q), p(q), p(o)) == -1
    assert L.hgp_rt_stats(P._h, None, 2, p(q), p(q), p(o)) == -1
    assert L.hgp_rt_stats(P._h, p(d), 2, p(q), None, p(o)) == -1
    assert L.hgp_rt_stats(P._h, None, 0, None, None, None) == 0        # nrhs = 0: a no-op
    assert P.rt_stats(d[:0], q, q).shape == (0, 3)
    with pytest.raises(ValueError):
        P.rt_stats(d, q[:-1], q)
    with pytest.raises(TypeError):
        P.rt_stats(d, q.double(), q)


def test_pcg_in_place_of_rhs_is_bit_identical():
    """hgp_pcg_solve with x = b (what predict(fused=True) uses to hold one (B, M) tensor, not two):
    the same bits as the solve into a separate x, rows layout, both dtypes, with the break firing
    (tol 1e-6) and not (tol 1e-30)."""
    from hipgp_amd.plan import ToeplitzPlan
    for dims, dtype in (((32, 24), torch.float64), ((64, 64), torch.float32), ((8, 6, 5), torch.float32)):
        P = ToeplitzPlan(dims, dtype, DEV)
        P.set_column(torch.tensor(_column(dims), device=DEV, dtype=dtype))
        b = torch.randn(5, P.M, device=DEV, dtype=dtype, generator=torch.Generator(device=DEV).manual_seed(2))
        for tol in (1e-30, 1e-6):
            ref = P.pcg(b, 12, tol)
            w = b.clone()
            got = P.pcg(w, 12, tol, out=w)
            assert got.data_ptr() == w.data_ptr()
            assert torch.equal(got, ref), (dims, dtype, tol)


def test_tensor_rt_stats_refuses_grad():
    import ziggy.kernels as zk
    from ziggy.misc.toeplitz_tensor import ToeplitzTensor
    k = zk.SqExp(dtype=torch.float64)
    grids = [torch.linspace(-1, 1, m, dtype=torch.float64, device=DEV) for m in (9, 7)]
    T = ToeplitzTensor(grids, lambda x, y: k.forward(x, y, params=(1., .3)), batch_shape=(2,), jitter_val=1e-2)
    d = torch.randn(2, T.M, dtype=torch.float64, device=DEV)
    q = torch.rand(T._plan.Mprime, dtype=torch.float64, device=DEV)
    out = T.rt_stats(d, q, q)
    kn = T._matmul_by_RT(d)
    ref = torch.stack([kn @ q, (kn * kn).sum(1), (kn * kn) @ q], dim=1)
    assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 1e-12
    with pytest.raises(RuntimeError):
        T.rt_stats(d.clone().requires_grad_(True), q, q)


# ---- model level ----------------------------------------------------------------------------------
def _model(fx, dtype):
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    k = zk.Matern(nu=1.5, dtype=dtype)
    grids = [torch.tensor(fx["grid0"], dtype=dtype), torch.tensor(fx["grid1"], dtype=dtype)]
    mod = hg.MeanFieldToeplitzGP(k, grids, num_obs=64, sig2_init=1., ell_init=.1, noise2_init=.01,
                                 learn_kernel=False, dtype=dtype)
    with torch.no_grad():
        mod.global_theta1.copy_(torch.tensor(fx["theta1"], dtype=dtype))
        mod.global_theta2.copy_(torch.tensor(fx["theta2"], dtype=dtype))
    return mod.cuda_params(0)


def test_predict_fused_G5_fp64():
    fx = load("G5", "f64")
    mod = _model(fx, torch.float64)
    x = torch.tensor(fx["xobs"], device=DEV)[:50]
    mu, sig = mod.predict(x, maxiter_cg=50, fused=True)
    assert mu.shape == fx["pred_mu"].shape and sig.shape == fx["pred_sig"].shape
    assert rel_err(mu.numpy(), fx["pred_mu"]) < 1e-7
    assert rel_err(sig.numpy(), fx["pred_sig"]) < 1e-7
    # fused=False and the default are today's path
    mu0, sig0 = mod.predict(x, maxiter_cg=50)
    mu1, sig1 = mod.predict(x, maxiter_cg=50, fused=False)
    assert torch.equal(mu0, mu1) and torch.equal(sig0, sig1)
    assert mu.shape == mu0.shape and sig.shape == sig0.shape


def test_predict_fused_G5_fp32():
    """No worse than 4x the reference's own fp32-vs-fp64 golden error, plus the 1e-6 floor."""
    fx32, fx64 = load("G5", "f32"), load("G5", "f64")
    mod = _model(fx32, torch.float32)
    x = torch.tensor(fx32["xobs"], device=DEV)[:50]
    mu, sig = mod.predict(x, maxiter_cg=50, fused=True)
    for got, key in ((mu, "pred_mu"), (sig, "pred_sig")):
        ref = fx64[key].astype(np.float64)
        e_me = np.linalg.norm(got.double().numpy().reshape(ref.shape) - ref)
        e_ref = np.linalg.norm(fx32[key].astype(np.float64) - ref)
        print(f"predict fused fp32 {key}: {e_me:.3e} (reference fp32 {e_ref:.3e})")
        assert e_me <= 4 * e_ref + 1e-6 * np.linalg.norm(ref), (key, e_me, e_ref)


def test_predict_fused_block_family_falls_back():
    from block_cases import block_model
    mod, fx = block_model("G11", device=DEV)
    x = torch.tensor(fx["xobs"], device=DEV)[:16]
    a = mod.predict(x, maxiter_cg=20, fused=False)
    b = mod.predict(x, maxiter_cg=20, fused=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


_ENV_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
from golden_cases import load
import test_rt_stats_gpu as t
fx = load("G5", "f64")
mod = t._model(fx, torch.float64)
x = torch.tensor(fx["xobs"], device="cuda")[:8]
calls = []
orig = type(mod).predict_stats
type(mod).predict_stats = lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1]
env = mod.predict(x, maxiter_cg=50)
fused = mod.predict(x, maxiter_cg=50, fused=True)
assert len(calls) == 2, calls
assert torch.equal(env[0], fused[0]) and torch.equal(env[1], fused[1])
print("ENV_FUSED_OK")
"""


def test_env_knob_selects_fused_path():
    env = dict(os.environ, HGP_PREDICT_FUSED="1")
    code = _ENV_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ENV_FUSED_OK" in r.stdout, r.stdout + r.stderr


def test_predict_fused_allocates_no_kn():
    """(256, 256) fp32, B = 64: kn would be 64 x 510^2 x 4 B = 66 MB.  torch's peak during the fused
    predict stays under half of that above the level before the call; the materialised path
    exceeds it (so the measurement sees the difference).

    The fused call holds Knm, solved in place (ToeplitzTensor.inv_matmul_), and qm / qS: two (B, M)
    tensors side by side would alone be 2 x 64 x 256^2 x 4 B = 33.6 MB, above the bound."""
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    dt = torch.float32
    grids = [torch.linspace(-1, 1, 256, dtype=dt) for _ in range(2)]
    mod = hg.MeanFieldToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, num_obs=64, sig2_init=1., ell_init=.05,
                                 noise2_init=.01, learn_kernel=False, dtype=dt).cuda_params(0)
    x = (torch.rand(64, 2, generator=torch.Generator().manual_seed(5), dtype=dt) * 1.8 - .9).to(DEV)
    kn_bytes = 64 * mod.Mprime * 4

    def peak(fused):
        mod.predict(x, maxiter_cg=5, fused=fused)          # warm-up: plans, pools
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        mod.predict(x, maxiter_cg=5, fused=fused)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    pf, pm = peak(True), peak(False)
    print(f"predict peak above base: fused {pf / 2**20:.1f} MiB, materialised {pm / 2**20:.1f} MiB, kn {kn_bytes / 2**20:.1f} MiB")
    assert pm > kn_bytes, (pm, kn_bytes)
    assert pf < kn_bytes / 2, (pf, kn_bytes)
