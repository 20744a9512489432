"""Product-form K matvec: a plan whose column is t0[i] t1[j] + sigma [i = j = 0] runs
HGP_OP_K as two 1-D Toeplitz passes.  Compared with the same plan created under HGP_SEPARABLE=0
(the general three-pass operator) and with the fp64 oracle.

Tolerances (set by the issue, not by what the code gives): fp64 -- the product form's error against
the oracle is at most 10x the general path's on the same input; fp32 -- at most 2x.  Columns that
are not products (Matern-3/2, a perturbed SqExp) must take the general path and equal the
HGP_SEPARABLE=0 plan bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ziggy_oracle as zo

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _column(kind, dims, params, jitter):
    grids = [np.linspace(-1, 1, m) for m in dims]
    nu = 1.5 if kind == "matern" else None
    return zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval(kind, x, y, params, nu=nu), jitter)


def _plans(dims, dt, col):
    """(default plan, HGP_SEPARABLE=0 plan) of one column (the knob is read by set_column)."""
    from hipgp_amd import plan as hp
    c = torch.tensor(col, device=DEV, dtype=dt)
    P = hp.ToeplitzPlan(dims, dt, DEV)
    P.set_column(c)
    Q = hp.ToeplitzPlan(dims, dt, DEV)
    old = os.environ.get("HGP_SEPARABLE")
    os.environ["HGP_SEPARABLE"] = "0"
    try:
        Q.set_column(c)
    finally:
        if old is None:
            del os.environ["HGP_SEPARABLE"]
        else:
            os.environ["HGP_SEPARABLE"] = old
    return P, Q, c


def _sep(P):
    from hipgp_amd import _lib
    s, r = ctypes.c_double(0), ctypes.c_double(0)
    return _lib.lib().hgp_plan_is_separable(P._h, ctypes.byref(s), ctypes.byref(r)), s.value, r.value


def _errs(P, Q, c, dims, nrhs, seed=3):
    from hipgp_amd import _lib
    M = int(np.prod(dims))
    x = torch.randn(nrhs, M, device=DEV, dtype=c.dtype, generator=torch.Generator(device=DEV).manual_seed(seed))
    ys = P.apply(_lib.OP_K, x).double().cpu().numpy()
    yg = Q.apply(_lib.OP_K, x).double().cpu().numpy()
    # the oracle on the column the plans hold (its stored values, in fp64)
    ref = zo.ToeplitzOracle(c.double().cpu().numpy(), dims).matmul_K(x.double().cpu().numpy())
    sc = np.max(np.abs(ref))
    return float(np.max(np.abs(ys - ref)) / sc), float(np.max(np.abs(yg - ref)) / sc)


# SqExp length scales at which the spectrum clamp (1e-6) changes nothing with the jitter 1e-3
F64 = [((48, 40), .1), ((33, 64), .1), ((64, 256), .02)]
# 600 x 24, 33 x 1024, 1024 x 17: one-wave lines (H = 1024) shorter than H (zero padding from the
# buffer range) and odd row counts (an absent second row) in either pass, and pitched rows of V
F32 = [((1024, 16), .05, 4), ((16, 1024), .05, 4), ((256, 256), .01, 4), ((96, 80), .05, 3), ((96, 80), .05, 9),
       ((2048, 16), .05, 2), ((600, 24), .05, 3), ((33, 1024), .05, 3), ((1024, 17), .05, 2)]


@pytest.mark.parametrize("dims,ell", F64, ids=[f"{d[0]}x{d[1]}" for d, _ in F64])
def test_product_form_fp64(dims, ell):
    from hipgp_amd import _lib
    P, Q, c = _plans(dims, torch.float64, _column("sqexp", dims, (1., ell), 1e-3))
    assert _sep(P)[0] == 1 and _sep(Q)[0] == 0
    es, eg = _errs(P, Q, c, dims, 3)
    print(f"fp64 {dims}: product form {es:.3e}, general {eg:.3e}")
    assert es <= 10 * eg, (es, eg)


@pytest.mark.parametrize("dims,ell,nrhs", F32, ids=[f"{d[0]}x{d[1]}_B{b}" for d, _, b in F32])
def test_product_form_fp32(dims, ell, nrhs):
    P, Q, c = _plans(dims, torch.float32, _column("sqexp", dims, (1., ell), 1e-3))
    assert _sep(P)[0] == 1 and _sep(Q)[0] == 0
    es, eg = _errs(P, Q, c, dims, nrhs)
    print(f"fp32 {dims} B={nrhs}: product form {es:.3e}, general {eg:.3e}")
    assert es <= 2 * eg, (es, eg)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", ["matern32", "perturbed"])
def test_non_product_columns_take_the_general_path(case, dt):
    from hipgp_amd import _lib
    dims = (96, 80)
    if case == "matern32":
        col = _column("matern", dims, (.1, .1), 1e-3)
    else:
        col = _column("sqexp", dims, (1., .05), 1e-3)
        col = col.reshape(dims).copy()
        col[3, 2] *= 1 + 1e-3
        col = col.reshape(-1)
    P, Q, c = _plans(dims, dt, col)
    sep, _, resid = _sep(P)
    assert sep == 0
    eps = 2.0 ** -24 if dt == torch.float32 else 2.0 ** -53
    assert resid > 100 * 4 * eps, resid                 # misses the bound by orders of magnitude
    x = torch.randn(5, dims[0] * dims[1], device=DEV, dtype=dt, generator=torch.Generator(device=DEV).manual_seed(1))
    assert torch.equal(P.apply(_lib.OP_K, x), Q.apply(_lib.OP_K, x))


@pytest.mark.parametrize("jitter", [0.0, 1e-3])
def test_jitter_recovered_and_unit_vector_gives_the_column(jitter):
    """sigma = c[0][0] - k00 within the column's rounding; K e0 = the column.  (A narrow kernel on
    a coarse grid: with no jitter its spectrum must still stay above the clamp.)"""
    from hipgp_amd import _lib
    dims = (48, 40)
    for dt, eps in ((torch.float32, 2.0 ** -24), (torch.float64, 2.0 ** -53)):
        P, Q, c = _plans(dims, dt, _column("sqexp", dims, (1., .03), jitter))
        sep, sigma, _ = _sep(P)
        assert sep == 1
        assert abs(sigma - jitter) <= 4 * eps * float(c.abs().max()), (sigma, jitter)
        e0 = torch.zeros(1, dims[0] * dims[1], device=DEV, dtype=dt)
        e0[0, 0] = 1
        y = P.apply(_lib.OP_K, e0)[0]
        # four transforms of L = 128 points, each within log2(L) eps of its largest value
        assert float((y - c).abs().max()) <= 4 * 7 * eps * float(c.abs().max()), float((y - c).abs().max())


def test_graph_replay_bitwise():
    """the second call is captured, later ones replay the graph: all equal the first bit for bit,
    with RHS chunks on both streams (17 RHS: chunks of 8 + 8 + 1) and after new arguments."""
    from hipgp_amd import _lib
    dims = (96, 80)
    P, Q, c = _plans(dims, torch.float32, _column("sqexp", dims, (1., .05), 1e-3))
    assert _sep(P)[0] == 1
    x = torch.randn(17, dims[0] * dims[1], device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    first = P.apply(_lib.OP_K, x).clone()
    y = torch.empty_like(first)
    for rep in range(4):
        y.fill_(float("nan"))
        P.apply(_lib.OP_K, x, out=y)
        assert torch.equal(y, first), rep
    x2 = x * 2
    a = P.apply(_lib.OP_K, x2).clone()
    assert torch.equal(P.apply(_lib.OP_K, x2), a)
    # the other operators of a product-form plan are the general ones
    for op in (_lib.OP_CINV, _lib.OP_RT):
        assert torch.equal(P.apply(op, x), Q.apply(op, x)), op


@pytest.mark.parametrize("j_old,j_new", [(0.0, 1e-3), (1e-3, 1e-2)])
def test_new_column_after_a_captured_graph(j_old, j_new):
    """sigma and whether sigma x is added are kernel arguments of the captured launches: a new
    column with another jitter on the same plan, x, y and RHS count must not replay them."""
    from hipgp_amd import _lib
    from hipgp_amd import plan as hp
    dims = (48, 40)
    col = lambda j: torch.tensor(_column("sqexp", dims, (1., .03), j), device=DEV, dtype=torch.float32)
    P = hp.ToeplitzPlan(dims, torch.float32, DEV)
    P.set_column(col(j_old))
    assert _sep(P)[0] == 1
    x = torch.randn(5, dims[0] * dims[1], device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    y = torch.empty_like(x)
    for _ in range(3):                                 # direct, captured, replayed
        P.apply(_lib.OP_K, x, out=y)
    P.set_column(col(j_new))
    assert _sep(P)[0] == 1
    F = hp.ToeplitzPlan(dims, torch.float32, DEV)
    F.set_column(col(j_new))
    ref = F.apply(_lib.OP_K, x)
    for rep in range(3):
        y.fill_(float("nan"))
        P.apply(_lib.OP_K, x, out=y)
        assert torch.equal(y, ref), rep


def test_device_scan_matches_host_detection():
    """the plan's device scan and hgp_separable_detect (host) agree on sigma and the residual"""
    from hipgp_amd import _lib
    dims = (96, 80)
    col = _column("sqexp", dims, (1., .05), 1e-3).astype(np.float32)
    P, Q, c = _plans(dims, torch.float32, col)
    out = (ctypes.c_double * 4)()
    _lib.check(_lib.lib().hgp_separable_detect(_lib.HGP_F32, dims[0], dims[1], col.ctypes.data_as(ctypes.c_void_p),
                                               0.0, out, None, None))
    sep, sigma, resid = _sep(P)
    assert sep == int(out[0]) == 1
    assert abs(sigma - out[1]) <= 1e-15 and abs(resid - out[2]) <= 1e-15 + 1e-6 * out[2]
