"""The inducing-grid posterior (HGP_OP_RSQ, grid_posterior / sample_grid) without a GPU: the op is in
the header and the binding with one value, the Python entry points exist and refuse what they
cannot do, and the host logic of `grid_posterior` / `sample_grid` on a stand-in Kmm made of the fp64
oracle's operators equals the dense computation R qm, sqrt((R o R) qS), R (qm + sqrt(qS) eps)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from grid_posterior_cases import OracleKmm, dense_R, max_rel, oracle_rsq
from oracle import ziggy_oracle as zo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (8, 6)


def test_op_in_header_equals_binding():
    from hipgp_amd import _lib
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    m = re.search(r"\bHGP_OP_RSQ\s*=\s*(\d+)", src)
    assert m, "include/hipgp.h does not define HGP_OP_RSQ"
    assert int(m.group(1)) == 4 == _lib.OP_RSQ
    ops = (_lib.OP_K, _lib.OP_CINV, _lib.OP_RT, _lib.OP_R, _lib.OP_RSQ)
    assert len(set(ops)) == 5
    assert re.search(r"HGP_OP_RSQ\s*:", src), "the op is not documented beside the other four"


def test_python_entry_points_exist():
    from hipgp_amd.ziggy.misc.toeplitz_tensor import ToeplitzTensor
    import hipgp_amd.ziggy.hipgp as hg
    assert callable(ToeplitzTensor._matmul_by_Rsq)
    assert list(inspect.signature(hg.MeanFieldToeplitzGP.grid_posterior).parameters) == ["self", "prior", "Kmm"]
    assert list(inspect.signature(hg.MeanFieldToeplitzGP.sample_grid).parameters) == [
        "self", "n", "prior", "generator", "eps", "Kmm"]
    assert hg.MeanFieldToeplitzGP.grid_posterior is not hg.ToeplitzInducingGP.grid_posterior
    assert hg.BlockToeplitzGP.grid_posterior is hg.ToeplitzInducingGP.grid_posterior
    assert hg.BlockToeplitzGP.sample_grid is hg.ToeplitzInducingGP.sample_grid


def test_oracle_restatement_is_the_squared_matrix():
    """The restated operator is R o R entry by entry (the premise of every other test here)."""
    O = _oracle()
    R = dense_R(O)
    Rsq = oracle_rsq(O, np.eye(O.Mp)).T
    assert R.shape == Rsq.shape == (O.M, O.Mp)
    assert max_rel(Rsq, R * R) < 1e-13


def _oracle():
    grids = [np.linspace(-1, 1, m) for m in DIMS]
    col = zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("matern", x, y, (1., .3), nu=1.5), 1e-3)
    return zo.ToeplitzOracle(col, DIMS)


def _model(whitened_type="ziggy", family="mean-field"):
    import hipgp_amd.ziggy.hipgp as hg
    import hipgp_amd.ziggy.kernels as zk
    dt = torch.float64
    grids = [torch.linspace(-1, 1, m, dtype=dt) for m in DIMS]
    torch.manual_seed(5)
    kw = dict(num_obs=40, sig2_init=1., ell_init=.3, noise2_init=.05, learn_kernel=False, dtype=dt,
              whitened_type=whitened_type)
    if family == "block":
        return hg.BlockToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, block_sizes=[2, 2], **kw)
    mod = hg.MeanFieldToeplitzGP(zk.Matern(nu=1.5, dtype=dt), grids, **kw)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():       # random theta1 / theta2 (theta2 < 0)
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=dt))
        mod.global_theta2.copy_(-(torch.rand(mod.Mprime, 1, generator=g, dtype=dt) * 4 + .5))
    return mod


def _dense(mod, O):
    R = dense_R(O)
    qm, qS = (t.detach().numpy().reshape(-1) for t in mod.standard_variational_params())
    return R, qm, qS


def test_grid_posterior_matches_dense():
    mod, O = _model(), _oracle()
    Kmm = OracleKmm(O)
    R, qm, qS = _dense(mod, O)
    mean, sd = mod.grid_posterior(Kmm=Kmm)
    assert tuple(mean.shape) == DIMS and tuple(sd.shape) == DIMS
    assert not mean.requires_grad and not sd.requires_grad
    assert max_rel(mean.numpy().reshape(-1), R @ qm) < 1e-12
    assert max_rel(sd.numpy().reshape(-1), np.sqrt((R * R) @ qS)) < 1e-12
    assert Kmm.calls == [("R", (1, O.Mp)), ("Rsq", (1, O.Mp))]


def test_prior_has_zero_mean_and_the_kernel_diagonal():
    mod, O = _model(), _oracle()
    Kmm = OracleKmm(O)
    R = dense_R(O)
    mean, sd = mod.grid_posterior(prior=True, Kmm=Kmm)
    assert tuple(mean.shape) == DIMS and torch.count_nonzero(mean) == 0
    assert max_rel(sd.numpy().reshape(-1), np.sqrt((R * R).sum(1))) < 1e-12
    assert Kmm.calls == [("Rsq", (1, O.Mp))]       # no R application for a zero mean
    g = torch.Generator().manual_seed(2)
    eps = torch.randn(3, O.Mp, generator=g, dtype=torch.float64)
    u = mod.sample_grid(3, prior=True, eps=eps, Kmm=Kmm)
    assert tuple(u.shape) == (3,) + DIMS
    assert max_rel(u.numpy().reshape(3, -1), eps.numpy() @ R.T) < 1e-12


def test_sample_grid_with_given_eps_matches_dense():
    mod, O = _model(), _oracle()
    Kmm = OracleKmm(O)
    R, qm, qS = _dense(mod, O)
    g = torch.Generator().manual_seed(3)
    eps = torch.randn(4, O.Mp, generator=g, dtype=torch.float64)
    keep = eps.clone()
    u = mod.sample_grid(4, eps=eps, Kmm=Kmm)
    assert tuple(u.shape) == (4,) + DIMS and not u.requires_grad
    assert torch.equal(eps, keep), "sample_grid changed the caller's eps"
    ref = (qm[None, :] + np.sqrt(qS)[None, :] * eps.numpy()) @ R.T
    assert max_rel(u.numpy().reshape(4, -1), ref) < 1e-12
    assert Kmm.calls == [("R", (4, O.Mp))]
    with pytest.raises(ValueError):
        mod.sample_grid(3, eps=eps, Kmm=Kmm)


def test_sample_grid_draws_from_the_generator():
    mod, O = _model(), _oracle()
    Kmm = OracleKmm(O)
    u1 = mod.sample_grid(2, generator=torch.Generator().manual_seed(9), Kmm=Kmm)
    u2 = mod.sample_grid(2, generator=torch.Generator().manual_seed(9), Kmm=Kmm)
    u3 = mod.sample_grid(2, generator=torch.Generator().manual_seed(10), Kmm=Kmm)
    assert torch.equal(u1, u2) and not torch.equal(u1, u3)
    eps = torch.randn((2, O.Mp), generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    assert torch.equal(u1, mod.sample_grid(2, eps=eps, Kmm=Kmm))


@pytest.mark.parametrize("family,whitened_type", [("block", "ziggy"), ("mean-field", "cholesky"),
                                                  ("block", "cholesky")])
def test_other_families_refuse(family, whitened_type):
    mod = _model(whitened_type=whitened_type, family=family)
    Kmm = OracleKmm(_oracle())
    for call in (lambda: mod.grid_posterior(Kmm=Kmm), lambda: mod.grid_posterior(prior=True, Kmm=Kmm),
                 lambda: mod.sample_grid(2, Kmm=Kmm)):
        with pytest.raises(NotImplementedError, match="block-diagonal S has no circulant"):
            call()
    assert Kmm.calls == []


def test_matmul_by_rsq_refuses_grad_inputs():
    """No backward: a grad-requiring vector or column raises instead of returning a graph-less tensor
    (checked on the method's own guard, without a device)."""
    from hipgp_amd.ziggy.misc.toeplitz_tensor import ToeplitzTensor

    class _Plan:
        def apply(self, op, x):
            raise AssertionError("the plan was reached")

    T = ToeplitzTensor.__new__(ToeplitzTensor)
    T._plan, T.cvec_shape = _Plan(), (1,)
    T.column = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no backward"):
        T._matmul_by_Rsq(torch.zeros(1, 4, dtype=torch.float64, requires_grad=True))
    T.column = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    with pytest.raises(RuntimeError, match="no backward"):
        T._matmul_by_Rsq(torch.zeros(1, 4, dtype=torch.float64))
