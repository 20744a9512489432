"""hgp_rt_block_stats / elbo_and_grad(streamed=True) / predict(streamed=True) without a GPU: the
symbol is exported and bound with the declared signature, the header and the ctypes binding agree,
the argument error that needs no device returns its code, the Python entry points and hooks exist
(the block family overrides the streamed_* hooks and still inherits fit_stats / predict_stats), and
the host arithmetic of the streamed step (a_n and bdiff_n from the three dots, the gram as lam_sum,
dm_sum by the linear route R^T(-sum_n bdiff_n d_n)) reproduces the materialised CPU path on G11
with a stub Kmm made of the fp64 oracle's operators.  (The register check of the new
k_block_stats_rt instantiations is tests/test_kernel_resources_cpu.py's reader on the rebuilt
library, below.)"""
import ctypes
import inspect
import os
import re

import numpy as np
import torch

from block_cases import block_model, noise_of
from golden_cases import rel_err
from oracle import ziggy_oracle as zo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HGP_E_ARG = -1


def _header_decl():
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    m = re.search(r"\bint\s+hgp_rt_block_stats\s*\(([^)]*)\)\s*;", src)
    assert m, "include/hipgp.h does not declare hgp_rt_block_stats"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbol_exported_and_bound():
    from hipgp_amd import _lib
    L = _lib.lib()
    assert "hgp_rt_block_stats" in _lib.EXPORTS
    fn = L.hgp_rt_block_stats
    assert fn.restype is ctypes.c_int
    vp, i64, pi64 = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    assert list(fn.argtypes) == [vp, vp, i64, pi64, i64, vp, vp, vp, vp, vp]


def test_header_and_binding_agree():
    from hipgp_amd import _lib
    args = _header_decl()
    assert args == ["hgp_plan* plan", "const void* d", "int64_t nrhs", "const int64_t* blocks", "int64_t piece_rhs",
                    "const void* qm", "const void* S", "const void* ivar", "void* out3", "void* gram"]
    ctype_of = lambda a: (ctypes.POINTER(ctypes.c_int64) if "int64_t*" in a else ctypes.c_int64
                          if a.startswith("int64_t") else ctypes.c_void_p if "*" in a else None)
    assert [ctype_of(a) for a in args] == list(_lib.lib().hgp_rt_block_stats.argtypes)


def test_null_plan_is_an_argument_error():
    from hipgp_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    blk = (ctypes.c_int64 * 2)(2, 2)
    assert L.hgp_rt_block_stats(None, p, 1, blk, 0, p, p, p, p, p) == HGP_E_ARG
    assert b"null plan" in L.hgp_last_error()
    assert L.hgp_rt_block_stats(None, None, 0, None, 0, None, None, None, None, None) == HGP_E_ARG


def test_python_entry_points_and_hooks():
    from hipgp_amd.plan import ToeplitzPlan
    from hipgp_amd.ziggy.misc.toeplitz_tensor import ToeplitzTensor
    import hipgp_amd.ziggy.hipgp as hg
    assert callable(ToeplitzPlan.rt_block_stats) and callable(ToeplitzTensor.rt_block_stats)
    assert list(inspect.signature(ToeplitzPlan.rt_block_stats).parameters) == [
        "self", "d", "blocks", "qm", "S", "ivar", "gram", "piece_rhs"]
    for fn in (hg.ToeplitzInducingGP.elbo_and_grad, hg.ToeplitzInducingGP.predict):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "streamed" and params["streamed"].default is None
    base = hg.ToeplitzInducingGP
    assert list(inspect.signature(base.streamed_fit_stats).parameters) == [
        "self", "Knm", "ybatch", "Knn_diag", "noise_std_batch", "maxiter_cg", "Kmm"]
    assert list(inspect.signature(base.streamed_predict_stats).parameters) == ["self", "Knm", "maxiter_cg", "Kmm"]
    assert hg.BlockToeplitzGP.streamed_fit_stats is not base.streamed_fit_stats
    assert hg.BlockToeplitzGP.streamed_predict_stats is not base.streamed_predict_stats
    assert hg.BlockToeplitzGP.fit_stats is base.fit_stats
    assert hg.BlockToeplitzGP.predict_stats is base.predict_stats
    assert hg.MeanFieldToeplitzGP.streamed_fit_stats is base.streamed_fit_stats
    assert hg.MeanFieldToeplitzGP.streamed_predict_stats is base.streamed_predict_stats
    assert hg.BlockToeplitzGP.kn_piece_rhs == 0


def test_base_hooks_return_none():
    import hipgp_amd.ziggy.hipgp as hg
    Knm = torch.ones(2, 5)
    assert hg.ToeplitzInducingGP.streamed_fit_stats(None, Knm, None, None) is None
    assert hg.ToeplitzInducingGP.streamed_predict_stats(None, Knm) is None
    assert torch.equal(Knm, torch.ones(2, 5))


class _OracleKmm:
    """A Kmm whose operators are the fp64 oracle's, on CPU tensors: what `compute_kn` (inv_matmul,
    _matmul_by_RT) and the streamed hooks (inv_matmul, rt_block_stats, _matmul_by_RT) call.
    rt_block_stats is R^T followed by numpy sums over block_chunks indices."""

    def __init__(self, O):
        self.O = O
        self.column = torch.tensor(O.column)
        self.calls = []

    def inv_matmul(self, b, do_precond=True, maxiter=20, tol=1e-8):
        return torch.from_numpy(self.O.solve(b.detach().numpy().copy(), do_precond, maxiter, tol))

    def _matmul_by_RT(self, v):
        return torch.from_numpy(self.O.matmul_RT(v.detach().numpy()).reshape(v.shape[0], -1))

    def rt_block_stats(self, d, blocks, qm, S=None, ivar=None, gram=True, piece_rhs=0):
        from hipgp_amd.ziggy.hipgp import block_chunks
        self.calls.append({"gram": gram, "piece_rhs": piece_rhs, "blocks": list(blocks)})
        kn = self.O.matmul_RT(d.numpy()).reshape(d.shape[0], -1)
        idx = block_chunks([2 * m - 2 for m in self.O.dims], blocks)[0].numpy()
        kb = kn[:, idx]                                              # (B, nblk, bs)
        q = np.einsum("bki,kij,bkj->b", kb, S.numpy().reshape(idx.shape + idx.shape[1:]), kb) if S is not None \
            else np.zeros(kn.shape[0])
        out3 = np.stack([kn @ qm.numpy().reshape(-1), (kn * kn).sum(1), q], axis=1)
        G = torch.from_numpy(np.einsum("b,bki,bkj->kij", ivar.numpy().reshape(-1), kb, kb)) if gram else None
        return torch.from_numpy(out3), G


def _g11():
    mod, fx = block_model("G11")
    grids = [fx[f"grid{i}"] for i in range(2)]
    sig2, ell = (float(v) for v in fx["params"])
    col = zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("matern", x, y, (sig2, ell), nu=1.5), 1e-3)
    Kmm = _OracleKmm(zo.ToeplitzOracle(col, tuple(int(m) for m in fx["dims"])))
    return mod, fx, Kmm


def _step(mod, Kmm, x, y, noise, streamed):
    mod.global_theta1.grad = None
    mod.global_theta2.grad = None
    elbo = mod.elbo_and_grad(x, y, noise, maxiter_cg=30, Kmm=Kmm, streamed=streamed)
    return float(elbo), mod.global_theta1.grad.numpy().copy(), mod.global_theta2.grad.numpy().copy()


def test_streamed_host_arithmetic_matches_materialised_cpu_path():
    mod, fx, Kmm = _g11()
    x, y = torch.tensor(fx["xobs"]), torch.tensor(fx["yobs"])
    g = torch.Generator().manual_seed(7)
    for noise in (None, torch.rand(x.shape[0], generator=g, dtype=torch.float64) * .3 + .1):
        Kmm.calls.clear()
        e0, g1, g2 = _step(mod, Kmm, x, y, noise, False)
        assert not Kmm.calls
        mod.kn_piece_rhs = 6
        e1, h1, h2 = _step(mod, Kmm, x, y, noise, True)
        assert Kmm.calls == [{"gram": True, "piece_rhs": 6, "blocks": [4, 4]}], Kmm.calls
        assert abs(e1 - e0) <= 1e-10 * abs(e0), (e0, e1)
        assert h1.shape == g1.shape and h2.shape == g2.shape
        assert rel_err(h1, g1) < 1e-10 and rel_err(h2, g2) < 1e-10
    # the dict is batch_stats's, lam_sum the gram
    Knm, kd = mod._make_grams(x)
    kn = mod.compute_kn(Knm, maxiter_cg=30, Kmm=Kmm)
    ref = mod.batch_stats(kn, y, kd, None)
    st = mod.streamed_fit_stats(Knm, y, kd, None, maxiter_cg=30, Kmm=Kmm)
    assert set(st) == set(ref) and st["n"] == ref["n"]
    for k in ("an_sum", "lam_sum", "dm_sum"):
        assert st[k].shape == ref[k].shape, k
        assert rel_err(st[k].numpy(), ref[k].numpy()) < 1e-10, k


def test_streamed_predict_matches_materialised_cpu_path():
    mod, fx, Kmm = _g11()
    x = torch.tensor(fx["xobs"])[:20]
    mu0, sig0 = mod.predict(x, maxiter_cg=50, Kmm=Kmm, streamed=False)
    assert not Kmm.calls
    mu1, sig1 = mod.predict(x, maxiter_cg=50, Kmm=Kmm, streamed=True)
    assert Kmm.calls == [{"gram": False, "piece_rhs": 0, "blocks": [4, 4]}], Kmm.calls
    assert mu1.shape == mu0.shape and sig1.shape == sig0.shape
    assert rel_err(mu1.numpy(), mu0.numpy()) < 1e-10 and rel_err(sig1.numpy(), sig0.numpy()) < 1e-10


def test_default_and_declined_cases_stay_materialised(monkeypatch):
    monkeypatch.delenv("HGP_BLOCK_STREAMED", raising=False)
    mod, fx, Kmm = _g11()
    x, y = torch.tensor(fx["xobs"]), torch.tensor(fx["yobs"])
    _step(mod, Kmm, x, y, None, None)                      # default: HGP_BLOCK_STREAMED unset
    assert not Kmm.calls
    monkeypatch.setenv("HGP_BLOCK_STREAMED", "1")
    _step(mod, Kmm, x, y, None, None)
    assert len(Kmm.calls) == 1
    _step(mod, Kmm, x, y, None, False)                     # the keyword wins over the knob
    assert len(Kmm.calls) == 1
    mod.log_noise2.requires_grad_(True)                    # the autograd ELBO needs kn
    assert mod.hyper_grad_needed(None)
    mod.elbo_and_grad(x, y, None, maxiter_cg=30, Kmm=Kmm, streamed=True)
    assert len(Kmm.calls) == 1
    mod.log_noise2.requires_grad_(False)
    # the hook itself declines, Knm untouched: an empty batch, a Kmm without the entry point, cholesky
    ones = lambda n: torch.ones(n, Kmm.O.M, dtype=torch.float64)

    class _Bare:
        pass
    kd = torch.ones(2, dtype=torch.float64)
    assert mod.streamed_fit_stats(ones(0), y[:0], kd[:0], Kmm=Kmm) is None
    Knm = ones(2)
    assert mod.streamed_fit_stats(Knm, y[:2], kd, Kmm=_Bare()) is None
    assert mod.streamed_predict_stats(Knm, Kmm=_Bare()) is None
    mod.whitened_type = "cholesky"
    assert mod.streamed_fit_stats(Knm, y[:2], kd, Kmm=Kmm) is None
    assert mod.streamed_predict_stats(Knm, Kmm=Kmm) is None
    assert torch.equal(Knm, ones(2)) and len(Kmm.calls) == 1


def test_new_fp32_kernels_do_not_spill():
    """The fp32 k_block_stats_rt instantiations neither spill nor use scratch (the code-object notes
    of the built library, read as tests/test_kernel_resources_cpu.py reads them)."""
    import test_kernel_resources_cpu as kr
    ks = [k for k in kr._kernels() if "hgp::k_block_stats_rt<float" in k[0]]
    assert len(ks) == 16, [k[0] for k in ks]                 # TA in {0, 2..8} x SL in {false, true}
    bad = [k for k in ks if k[1] or k[2]]
    assert not bad, bad
