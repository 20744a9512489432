"""Fused banded K matvec: the two banded products of DESIGN §23 in one kernel with the
intermediate V in LDS.  Each case asserts that the default plan takes the fused kernel, that a plan
set under HGP_BAND_FUSED=0 does not, that the two results are equal bit for bit (both summations keep
their order), and the §23 elementwise bound against the fp64 oracle:
  |y - y64| <= (n0 + n1 + 4) 2^-24 (|K| |x|) + 2^-24 ||t0||_1 ||t1||_1 max |x|,  n_a = 16 + 2 r_a
(r_a rounded up to even).  Shapes are sized from hgp_band_fused_tile = {SEG, TW}."""
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


def _tile():
    from hipgp_amd import _lib
    t = (ctypes.c_int * 2)(0, 0)
    _lib.check(_lib.lib().hgp_band_fused_tile(t))
    return t[0], t[1]


def _column(dims, ell, jitter):
    grids = [np.linspace(-1, 1, m) for m in dims]
    return zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("sqexp", x, y, (1., ell)), jitter)


def _plan(dims, c, fused=True):
    """a plan of the column c; fused=False: set under HGP_BAND_FUSED=0 (read by set_column)"""
    from hipgp_amd import plan as hp
    P = hp.ToeplitzPlan(dims, torch.float32, DEV)
    _set(P, c, fused)
    return P


def _set(P, c, fused):
    if fused:
        P.set_column(c)
    else:
        with _env("HGP_BAND_FUSED", "0"):
            P.set_column(c)


def _radius(P):
    from hipgp_amd import _lib
    r = (ctypes.c_int * 2)(-7, -7)
    act = _lib.lib().hgp_plan_band_radius(P._h, r)
    assert act in (0, 1), act
    return act, (r[0], r[1])


def _is_fused(P):
    from hipgp_amd import _lib
    return _lib.lib().hgp_plan_band_fused(P._h)


def _host_rule(t):
    from hipgp_amd import _lib
    t = np.ascontiguousarray(t, dtype=np.float64)
    r = ctypes.c_int64(-1)
    _lib.check(_lib.lib().hgp_band_radius(t.size, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(r)))
    return r.value


def _ell_for_radius(m, r):
    """a length scale whose factor column on an m-point axis has tap radius r by the host rule: the
    middle of the scanned range that gives r"""
    h = 2.0 / (m - 1)
    j = np.arange(m, dtype=np.float64)
    hits = [q for q in np.arange(0.2, 7.0, 0.01) if _host_rule(np.exp(-0.5 * (j * h / (q * h)) ** 2)) == r]
    assert hits, (m, r)
    return float(hits[len(hits) // 2] * h)


def _host_radii(c, dims):
    """the host rule on the host detection's factors of the stored column, and their row sums"""
    from hipgp_amd import _lib
    col = np.ascontiguousarray(c.cpu().numpy())
    out = (ctypes.c_double * 4)()
    t0 = (ctypes.c_double * dims[0])()
    t1 = (ctypes.c_double * dims[1])()
    _lib.check(_lib.lib().hgp_separable_detect(_lib.HGP_F32, dims[0], dims[1], col.ctypes.data_as(ctypes.c_void_p), 0.0,
                                               out, t0, t1))
    assert out[0] == 1
    rs = tuple(_host_rule(np.array(t)) for t in (t0, t1))
    l1 = [abs(t[0]) + 2 * float(np.sum(np.abs(np.array(t)[1:]))) for t in (t0, t1)]
    return rs, l1


def _check(dims, ell, jitter, nrhs, x=None, seed=3, want=None):
    """one case: fused on the default plan, off under the knob, bit equality of the two, the §23
    bound.  Returns (fused y, column, radii)."""
    from hipgp_amd import _lib
    c = torch.tensor(_column(dims, ell, jitter), device=DEV, dtype=torch.float32)
    P, Q = _plan(dims, c), _plan(dims, c, fused=False)
    act, r = _radius(P)
    host_r, l1 = _host_radii(c, dims)
    assert act == 1 and r == host_r and _radius(Q) == (1, r), (act, r, host_r, _radius(Q))
    if want is not None:
        assert want(r), r
    assert _is_fused(P) == 1 and _is_fused(Q) == 0
    M = dims[0] * dims[1]
    if x is None:
        x = torch.randn(nrhs, M, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    yf = P.apply(_lib.OP_K, x)
    y2 = Q.apply(_lib.OP_K, x)
    assert torch.equal(yf, y2), float((yf - y2).abs().max())
    cn, xn = c.double().cpu().numpy(), x.double().cpu().numpy()
    ref = zo.ToeplitzOracle(cn, dims).matmul_K(xn)
    mag = zo.ToeplitzOracle(np.abs(cn), dims).matmul_K(np.abs(xn))
    n = [16 + 2 * ((ra + 1) // 2 * 2) for ra in r]
    bound = (n[0] + n[1] + 4) * U * mag + U * l1[0] * l1[1] * np.max(np.abs(xn))
    ef = np.abs(yf.double().cpu().numpy() - ref)
    print(f"{dims} r={r} B={x.shape[0]}: fused max err {ef.max():.3e} (bound used {np.max(ef / bound):.3f})")
    assert np.all(ef <= bound), float(np.max(ef / bound))
    return yf, c, r


def test_one_partial_block():
    _check((48, 40), .035, 1e-3, 3, want=lambda r: r == (4, 4))


def test_band_reaches_both_edges():
    _check((20, 24), .25, 1e-3, 3, want=lambda r: r == (13, 16))


def test_deepest_k_and_a_full_ring():
    _check((64, 64), .185, 1e-3, 3, want=lambda r: r == (32, 32))


@pytest.mark.parametrize("nrhs", [1, 3, 9])
def test_two_segments_and_two_strips(nrhs):
    SEG, TW = _tile()
    dims = (SEG + 17, TW + 9)
    _check(dims, _ell_for_radius(dims[1], 6), 1e-3, nrhs, want=lambda r: 5 <= min(r) and max(r) <= 32)


def test_exact_multiples():
    """a halo row or column index exactly on the grid edge"""
    SEG, TW = _tile()
    dims = (2 * SEG, TW)
    _check(dims, _ell_for_radius(dims[1], 5), 1e-3, 2, want=lambda r: 1 <= min(r) and max(r) <= 32)


def test_ring_wraps_within_and_across_segments():
    SEG, TW = _tile()
    dims = (3 * SEG + 5, 40)
    _check(dims, _ell_for_radius(dims[0], 32), 1e-3, 2, want=lambda r: r[0] == 32)


def test_no_sigma_epilogue():
    _check((48, 40), .03, 0.0, 3, want=lambda r: r == (4, 3))


def test_rhs_index_in_the_block_decomposition():
    _check((48, 40), .035, 1e-3, 33, want=lambda r: r == (4, 4))


def test_impulses_at_the_seams():
    """unit impulses on both sides of the segment and strip seams and at an interior point, one per
    right-hand side: the response patches are equal bit for bit, everything else is exactly 0"""
    SEG, TW = _tile()
    rn = 8
    dims = (SEG + 17 + 2 * rn, TW + 9 + 2 * rn)
    ell = _ell_for_radius(dims[0], rn)                               # axis 0 has the finer step
    pts = [(SEG - 1, TW - 1), (SEG, TW), (SEG - 1, TW), (SEG + 8 + rn, TW + 4 + rn)]
    M = dims[0] * dims[1]
    x = torch.zeros(len(pts), M, device=DEV)
    for q, (i, j) in enumerate(pts):
        x[q, i * dims[1] + j] = 1
    yf, _, r = _check(dims, ell, 1e-3, len(pts), x=x, want=lambda r: 1 <= min(r) and max(r) <= rn)
    i, j = pts[-1]
    assert min(i - SEG, dims[0] - 1 - i, j - TW, dims[1] - 1 - j) >= max(r)
    y = yf.cpu().numpy().reshape(len(pts), *dims)
    patches = []
    for q, (i, j) in enumerate(pts):
        assert i - r[0] >= 0 and i + r[0] < dims[0] and j - r[1] >= 0 and j + r[1] < dims[1]
        sl = (slice(i - r[0], i + r[0] + 1), slice(j - r[1], j + r[1] + 1))
        patches.append(y[q][sl].copy())
        rest = y[q].copy()
        rest[sl] = 0
        assert np.all(rest == 0), q
    assert patches[0][r[0], r[1]] > 0
    for q in range(1, len(pts)):
        assert np.array_equal(patches[q].view(np.uint32), patches[0].view(np.uint32)), q


def test_graph_replay_and_the_knob_on_the_same_plan():
    """direct, captured, replayed x3: all bit-equal; then the same plan, x and y under
    HGP_BAND_FUSED=0 must not replay the fused launch, and the same in reverse.

    The two paths are bit-equal by design, so the values cannot tell a stale replayed graph of the
    other path from a fresh launch: what separates the legs is hgp_plan_band_fused (the plan flag).
    set_column drops the captured graph in any case; the flag's place in the graph key is not
    observable through results."""
    from hipgp_amd import _lib
    SEG, TW = _tile()
    dims = (SEG + 17, 40)
    c = torch.tensor(_column(dims, _ell_for_radius(dims[0], 12), 1e-3), device=DEV, dtype=torch.float32)
    x = torch.randn(5, dims[0] * dims[1], device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    ref = {True: _plan(dims, c).apply(_lib.OP_K, x).clone(), False: _plan(dims, c, fused=False).apply(_lib.OP_K, x).clone()}
    assert torch.equal(ref[True], ref[False])
    P = _plan(dims, c)
    assert _radius(P)[0] == 1
    y = torch.empty_like(x)
    for leg, fused in enumerate((True, False, True)):
        if leg > 0:
            _set(P, c, fused)
        assert _is_fused(P) == (1 if fused else 0)
        for rep in range(5):                                         # direct, captured, replayed x3
            y.fill_(float("nan"))
            P.apply(_lib.OP_K, x, out=y)
            assert torch.equal(y, ref[fused]), (leg, rep)
