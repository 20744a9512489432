"""Banded product-form K matvec: an fp32 product-form plan whose factor columns have
tap radii r0, r1 <= 32 runs HGP_OP_K as two banded matrix products on the matrix cores.  Each case
is compared with the fp64 oracle on the plan's stored column and with the same plan under
HGP_BANDED=0 (the transform passes of DESIGN §20).

Bound (derived, not measured), elementwise, with n_a = 16 + 2 r_a (r_a rounded up to even):
  |y - y64| <= (n0 + n1 + 4) 2^-24 (|K| |x|) + 2^-24 ||t0||_1 ||t1||_1 max |x|
-- the fma chains of the two summations and the sigma x add, and the tap rule's truncation -- and in
the max norm the banded error is at most twice the HGP_BANDED=0 error on the same input."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ziggy_oracle as zo

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _column(dims, ell, jitter):
    grids = [np.linspace(-1, 1, m) for m in dims]
    return zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("sqexp", x, y, (1., ell)), jitter)


def _plan(dims, dt, c, banded=True):
    """a plan of the column c; banded=False: set under HGP_BANDED=0 (the knob is read by set_column)"""
    from hipgp_amd import plan as hp
    P = hp.ToeplitzPlan(dims, dt, DEV)
    if banded:
        P.set_column(c)
    else:
        with _env("HGP_BANDED", "0"):
            P.set_column(c)
    return P


def _radius(P):
    from hipgp_amd import _lib
    r = (ctypes.c_int * 2)(-7, -7)
    act = _lib.lib().hgp_plan_band_radius(P._h, r)
    assert act in (0, 1), act
    return act, (r[0], r[1])


def _host_radii(c, dims):
    """the host rule (hgp_band_radius) on the host detection's factors of the stored column"""
    from hipgp_amd import _lib
    col = np.ascontiguousarray(c.cpu().numpy())
    out = (ctypes.c_double * 4)()
    t0 = (ctypes.c_double * dims[0])()
    t1 = (ctypes.c_double * dims[1])()
    _lib.check(_lib.lib().hgp_separable_detect(_lib.HGP_F32 if col.dtype == np.float32 else _lib.HGP_F64, dims[0],
                                               dims[1], col.ctypes.data_as(ctypes.c_void_p), 0.0, out, t0, t1))
    assert out[0] == 1
    rs = []
    for t in (t0, t1):
        r = ctypes.c_int64(-1)
        _lib.check(_lib.lib().hgp_band_radius(len(t), t, ctypes.byref(r)))
        rs.append(r.value)
    l1 = [abs(t[0]) + 2 * float(np.sum(np.abs(np.array(t)[1:]))) for t in (t0, t1)]
    return tuple(rs), l1


def _check(dims, ell, jitter, nrhs, radii, x=None, seed=3):
    """one case: radii as stated and as the host rule gives, the elementwise bound against the oracle,
    the 2x max-norm comparison with HGP_BANDED=0.  Returns (banded y, HGP_BANDED=0 y, column)."""
    from hipgp_amd import _lib
    c = torch.tensor(_column(dims, ell, jitter), device=DEV, dtype=torch.float32)
    P, Q = _plan(dims, torch.float32, c), _plan(dims, torch.float32, c, banded=False)
    act, r = _radius(P)
    host_r, l1 = _host_radii(c, dims)
    assert act == 1 and r == radii == host_r, (act, r, radii, host_r)
    assert _radius(Q) == (0, radii)
    M = dims[0] * dims[1]
    if x is None:
        x = torch.randn(nrhs, M, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    yb = P.apply(_lib.OP_K, x)
    yt = Q.apply(_lib.OP_K, x)
    cn, xn = c.double().cpu().numpy(), x.double().cpu().numpy()
    ref = zo.ToeplitzOracle(cn, dims).matmul_K(xn)
    mag = zo.ToeplitzOracle(np.abs(cn), dims).matmul_K(np.abs(xn))
    n = [16 + 2 * ((ra + 1) // 2 * 2) for ra in r]
    bound = (n[0] + n[1] + 4) * U * mag + U * l1[0] * l1[1] * np.max(np.abs(xn))
    eb, et = np.abs(yb.double().cpu().numpy() - ref), np.abs(yt.double().cpu().numpy() - ref)
    print(f"{dims} r={r} B={x.shape[0]}: banded max err {eb.max():.3e} (bound used {np.max(eb / bound):.3f}), "
          f"HGP_BANDED=0 {et.max():.3e}")
    assert np.all(eb <= bound), float(np.max(eb / bound))
    assert eb.max() <= 2 * et.max(), (eb.max(), et.max())
    return yb, yt, c


#        dims        ell   jitter nrhs radii
CASES = [((48, 40), .035, 1e-3, 3, (4, 4)),        # the smallest
         ((50, 37), .07, 1e-3, 1, (9, 7)),         # no axis a multiple of 16, odd radii
         ((50, 37), .07, 1e-3, 3, (9, 7)),
         ((50, 37), .07, 1e-3, 9, (9, 7)),         # a partial last chunk
         ((96, 80), .05, 1e-3, 9, (13, 11)),       # r0 != r1
         ((64, 64), .185, 1e-3, 3, (32, 32)),      # r = HGP_BAND_RMAX
         ((20, 24), .25, 1e-3, 3, (13, 16)),       # r > m / 2: the band reaches both edges from every row
         ((256, 256), .01, 1e-3, 3, (7, 7)),       # several blocks on both axes
         ((48, 40), .03, 0.0, 3, (4, 3))]          # sigma = 0: no sigma x epilogue (nothing clamped)


@pytest.mark.parametrize("dims,ell,jitter,nrhs,radii", CASES,
                         ids=[f"{d[0]}x{d[1]}_r{r[0]}_{r[1]}_B{b}_j{j:g}" for d, _, j, b, r in CASES])
def test_banded_matvec(dims, ell, jitter, nrhs, radii):
    _check(dims, ell, jitter, nrhs, radii)


def test_radius_past_rmax_is_inactive_and_bit_equal():
    """the 64 x 64 grid with a slightly longer length scale: r = 33 takes the transform passes"""
    from hipgp_amd import _lib
    dims = (64, 64)
    c = torch.tensor(_column(dims, .19, 1e-3), device=DEV, dtype=torch.float32)
    P, Q = _plan(dims, torch.float32, c), _plan(dims, torch.float32, c, banded=False)
    assert _radius(P) == (0, (33, 33)) and _radius(Q) == (0, (33, 33))
    assert _host_radii(c, dims)[0] == (33, 33)
    x = torch.randn(3, dims[0] * dims[1], device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    assert torch.equal(P.apply(_lib.OP_K, x), Q.apply(_lib.OP_K, x))


def test_fp64_plan_is_inactive():
    from hipgp_amd import _lib
    dims = (48, 40)
    c = torch.tensor(_column(dims, .035, 1e-3), device=DEV, dtype=torch.float64)
    P, Q = _plan(dims, torch.float64, c), _plan(dims, torch.float64, c, banded=False)
    assert _radius(P)[0] == 0 and _radius(Q)[0] == 0
    x = torch.randn(3, dims[0] * dims[1], device=DEV, dtype=torch.float64,
                    generator=torch.Generator(device=DEV).manual_seed(4))
    assert torch.equal(P.apply(_lib.OP_K, x), Q.apply(_lib.OP_K, x))


@pytest.mark.parametrize("jitter,ell,radii", [(1e-3, .035, (4, 4)), (0.0, .03, (4, 3))], ids=["sigma", "nosigma"])
def test_unit_vectors_return_the_column_and_its_mirror(jitter, ell, radii):
    """x = e_0 gives the column, x = the last corner's unit vector its mirror image; outside the
    band (|di| > r0 or |dj| > r1) the dropped taps read exactly 0"""
    dims = (48, 40)
    M = dims[0] * dims[1]
    x = torch.zeros(2, M, device=DEV)
    x[0, 0] = 1
    x[1, M - 1] = 1
    yb, _, c = _check(dims, ell, jitter, 2, radii, x=x)
    y = yb.cpu().numpy().reshape(2, *dims)
    col = c.cpu().numpy().reshape(dims)
    out = np.ones(dims, bool)
    out[:radii[0] + 1, :radii[1] + 1] = False
    assert np.all(y[0][out] == 0) and np.all(y[1][::-1, ::-1][out] == 0)
    assert np.array_equal(y[0], y[1][::-1, ::-1])
    band = ~out
    # the stored column against t0[i] t1[j]: the product form's acceptance (4 units of max |c|), the
    # two taps' and the product's roundings, the sigma add
    assert np.max(np.abs(y[0][band] - col[band])) <= 8 * U * col.max()
    assert np.all(y[0][band] > 0)


def test_graph_replay_bitwise():
    """the second call is captured, later ones replay the graph: all equal the first bit for bit
    (17 RHS: chunks of 8 + 8 + 1 on both streams)"""
    from hipgp_amd import _lib
    dims = (96, 80)
    c = torch.tensor(_column(dims, .05, 1e-3), device=DEV, dtype=torch.float32)
    P = _plan(dims, torch.float32, c)
    assert _radius(P) == (1, (13, 11))
    x = torch.randn(17, dims[0] * dims[1], device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    first = P.apply(_lib.OP_K, x).clone()
    y = torch.empty_like(first)
    for rep in range(4):
        y.fill_(float("nan"))
        P.apply(_lib.OP_K, x, out=y)
        assert torch.equal(y, first), rep


@pytest.mark.parametrize("dims,old,new", [((48, 40), (.035, 1, (4, 4)), (.07, 1, (9, 7))),
                                          ((48, 40), (.07, 1, (9, 7)), (.035, 1, (4, 4))),
                                          ((64, 64), (.185, 1, (32, 32)), (.19, 0, (33, 33))),
                                          ((64, 64), (.19, 0, (33, 33)), (.185, 1, (32, 32)))],
                         ids=["wider", "narrower", "past_rmax", "back_under_rmax"])
def test_new_column_of_another_radius_after_a_captured_graph(dims, old, new):
    """the radii are kernel arguments of the captured launches and the taps a plan buffer: a new
    column on the same plan, x, y and RHS count must not replay them"""
    from hipgp_amd import _lib
    col = lambda ell: torch.tensor(_column(dims, ell, 1e-3), device=DEV, dtype=torch.float32)
    P = _plan(dims, torch.float32, col(old[0]))
    assert _radius(P) == old[1:]
    x = torch.randn(5, dims[0] * dims[1], device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    y = torch.empty_like(x)
    for _ in range(3):                                 # direct, captured, replayed
        P.apply(_lib.OP_K, x, out=y)
    P.set_column(col(new[0]))
    assert _radius(P) == new[1:]
    F = _plan(dims, torch.float32, col(new[0]))
    ref = F.apply(_lib.OP_K, x)
    for rep in range(3):
        y.fill_(float("nan"))
        P.apply(_lib.OP_K, x, out=y)
        assert torch.equal(y, ref), rep
