"""k_sep_pass at every half-length H = 2 ... 8192 it is instantiated for, as pass 0
(axis 1: strided rows of x in, V transposed at pitch round_up(m0, 32) out) and as pass 1 (axis 0:
pitched rows of V in, y out, + sigma x), in both dtypes; and the RHS-chunk arithmetic of run_sep /
run_band under HGP_WS_MB and HGP_STREAMS.  Cases and column: tests/sep_cases.py.

Every fp32 plan is set under HGP_BANDED=0, so that it runs k_sep_pass whatever its tap radii.

Bounds (set before any run):
  sweep     product-form error against the fp64 oracle on the stored column, max norm relative to
            max |ref|: <= 2x the general path's (HGP_SEPARABLE=0) in fp32, <= 10x in fp64 -- the rule
            of test_separable_gpu.py.  Cases listed in SPREAD miss that ratio with an error spread
            over the whole result; they are held to the transform depth instead:
            es <= 2 (log2 L_K[0] + log2 L_K[1]) u.
  impulses  each response is the shifted / mirrored stored column within
            2 (log2 L_K[0] + log2 L_K[1]) u max |c|: four transforms, each within log2(L) u of its
            largest value (test_jitter_recovered_and_unit_vector_gives_the_column with its own L).
  u = 2^-24 (fp32), 2^-53 (fp64)."""
import contextlib
import ctypes
import gc
import math
import os

import numpy as np
import pytest
import torch

import sep_cases as sc
from oracle import ziggy_oracle as zo

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": torch.float32, "f64": torch.float64}
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
RATIO = {"f32": 2.0, "f64": 10.0}
ALL = [(k, d) for k in ("f32", "f64") for d in sc.CASES[k]]
# 9 right-hand sides (chunks of 5 + 4 on the two streams) at one short and one long H per dtype
NINE = {("f32", (8, 4)), ("f32", (4200, 2)), ("f64", (8, 4)), ("f64", (2100, 3))}
# cases that miss the ratio rule, with the measured (es, eg): held to the transform-depth bound.
# None on an MI355X: the largest es / eg is 1.93 in fp32 (301 x 2: 6.77e-7 / 3.51e-7) and 0.70 in fp64
# (3 x 2100: 1.35e-15 / 1.93e-15)
SPREAD = {}


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _sep(P):
    from hipgp_amd import _lib
    s, r = ctypes.c_double(0), ctypes.c_double(0)
    return _lib.lib().hgp_plan_is_separable(P._h, ctypes.byref(s), ctypes.byref(r))


def _band(P):
    from hipgp_amd import _lib
    r = (ctypes.c_int * 2)(-7, -7)
    return _lib.lib().hgp_plan_band_radius(P._h, r), (r[0], r[1])


def _band_fused(P):
    from hipgp_amd import _lib
    return _lib.lib().hgp_plan_band_fused(P._h)


def _stored(kind, dims):
    return torch.tensor(sc.column(dims, np.float64), device=DEV).to(DT[kind])


def _sep_plan(kind, dims, c, **create_env):
    """a plan of c that runs k_sep_pass: set under HGP_BANDED=0; create_env around the constructor"""
    from hipgp_amd import plan as hp
    with _env(**create_env):
        P = hp.ToeplitzPlan(dims, DT[kind], DEV)
    with _env(HGP_BANDED="0"):
        ncl = P.set_column(c, count_clamped=True)
    return P, ncl


def _randn(kind, nrhs, M, seed):
    return torch.randn(nrhs, M, device=DEV, dtype=DT[kind], generator=torch.Generator(device=DEV).manual_seed(seed))


def _depth(P):
    return 2 * (math.log2(P.L_K[0]) + math.log2(P.L_K[1]))


@pytest.fixture(scope="module", params=ALL, ids=[f"{k}_{sc.case_id(d)}" for k, d in ALL])
def case(request):
    """the product-form plan, the HGP_SEPARABLE=0 plan and the fp64 oracle of one case, built once
    for the tests that use it"""
    from hipgp_amd import plan as hp
    kind, dims = request.param
    c = _stored(kind, dims)
    P, ncl = _sep_plan(kind, dims, c)
    Q = hp.ToeplitzPlan(dims, DT[kind], DEV)
    with _env(HGP_SEPARABLE="0"):
        Q.set_column(c)
    col64 = c.double().cpu().numpy()
    H = sc.half_lens(dims)
    assert tuple(P.L_K[:2]) == (2 * H[0], 2 * H[1])
    # pass 0 runs along axis 1 (H[1]) over the m0 rows, pass 1 along axis 0 (H[0]) over the m1 rows
    C = (sc.PAIRS[kind][H[1]], sc.PAIRS[kind][H[0]])
    return dict(kind=kind, dims=dims, c=c, P=P, Q=Q, ncl=ncl, col64=col64, O=zo.ToeplitzOracle(col64, dims), H=H, C=C)


def test_sweep_against_the_oracle(case):
    from hipgp_amd import _lib
    kind, dims, P, Q = case["kind"], case["dims"], case["P"], case["Q"]
    assert _sep(P) == 1 and _sep(Q) == 0
    assert _band(P)[0] == 0
    assert case["ncl"] == 0
    nrhs = 9 if (kind, dims) in NINE else 3
    x = _randn(kind, nrhs, dims[0] * dims[1], 3)
    ref = case["O"].matmul_K(x.double().cpu().numpy())
    sc_ = np.max(np.abs(ref))
    ds = np.abs(P.apply(_lib.OP_K, x).double().cpu().numpy() - ref).reshape(nrhs, *dims)
    dg = np.abs(Q.apply(_lib.OP_K, x).double().cpu().numpy() - ref)
    es, eg = float(ds.max() / sc_), float(dg.max() / sc_)
    at = np.unravel_index(np.argmax(ds), ds.shape)
    bound = _depth(P) * U[kind]
    print(f"{kind} {dims} B={nrhs} H={case['H']} C(pass 0, pass 1)={case['C']}: product form es {es:.3e} "
          f"({es / U[kind]:.2f} u, at rhs {at[0]} ({at[1]}, {at[2]})), general eg {eg:.3e} ({eg / U[kind]:.2f} u), "
          f"es / eg {es / eg:.2f}, depth bound {bound / U[kind]:.0f} u")
    if (kind, dims) in SPREAD:
        assert es <= bound, (es, eg, bound)
    else:
        assert es <= RATIO[kind] * eg, (es, eg)


def _impulse_sites(dims, C):
    m0, m1 = dims
    last = lambda m, c: ((m - 1) // (2 * c)) * (2 * c)          # first row of the last row block
    first = lambda m, c: min(2 * c, m) - 1                      # last row of the first block
    return [(0, 0), (m0 - 1, m1 - 1), (m0 - 1, 0), (last(m0, C[0]), last(m1, C[1])), (first(m0, C[0]), first(m1, C[1]))]


def test_impulses_at_the_masks(case):
    """unit impulses at the corners and at the row-block edges of either pass (blocks of 2C rows):
    the responses are the stored column shifted to the impulse and mirrored about it"""
    from hipgp_amd import _lib
    kind, dims, P = case["kind"], case["dims"], case["P"]
    m0, m1 = dims
    sites = _impulse_sites(dims, case["C"])
    x = torch.zeros(len(sites), m0 * m1, device=DEV, dtype=DT[kind])
    for q, (a, b) in enumerate(sites):
        x[q, a * m1 + b] = 1
    y = P.apply(_lib.OP_K, x).double().cpu().numpy().reshape(len(sites), m0, m1)
    col = case["col64"].reshape(dims)
    bound = _depth(P) * U[kind] * np.abs(col).max()
    i, j = np.arange(m0), np.arange(m1)
    errs = []
    for q, (a, b) in enumerate(sites):
        want = col[np.abs(i - a)[:, None], np.abs(j - b)[None, :]]
        errs.append(float(np.abs(y[q] - want).max()))
    mirror = float(np.abs(y[0] - y[1][::-1, ::-1]).max())
    print(f"{kind} {dims} H={case['H']} C={case['C']} impulses at {sites}: errors "
          f"{[round(e / U[kind], 2) for e in errs]} u, corner mirror {mirror / U[kind]:.2f} u, bound {bound / U[kind]:.1f} u")
    for q, e in enumerate(errs):
        assert e <= bound, (sites[q], e, bound)
    assert mirror <= bound, (mirror, bound)


# ---- nothing stored outside y -------------------------------------------------------------------
# the C = 64, C = 4 and C = 1 block shapes of either dtype, in either pass role
GUARD = [("f32", (4200, 2)), ("f32", (2, 4200)), ("f32", (2100, 3)), ("f32", (3, 2100)),
         ("f64", (2100, 3)), ("f64", (3, 2100)), ("f64", (1100, 5)), ("f64", (5, 1100))]


def _guarded_apply(P, x):
    """y = K x written into rows 1 ... B of a NaN-filled (B + 2)-row buffer"""
    from hipgp_amd import _lib
    B = x.shape[0]
    buf = torch.full((B + 2, x.shape[1]), float("nan"), device=DEV, dtype=x.dtype)
    P.apply(_lib.OP_K, x, out=buf[1:B + 1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[B + 1]).all())
    assert bool(torch.isfinite(buf[1:B + 1]).all())
    assert torch.equal(buf[1:B + 1], P.apply(_lib.OP_K, x))


@pytest.mark.parametrize("kind,dims", GUARD, ids=[f"{k}_{sc.case_id(d)}" for k, d in GUARD])
def test_nothing_stored_outside_y(kind, dims):
    H = sc.half_lens(dims)
    assert {sc.PAIRS[kind][h] for h in H} in ({1, 64}, {4, 64})
    P, _ = _sep_plan(kind, dims, _stored(kind, dims))
    assert _sep(P) == 1 and _band(P)[0] == 0
    _guarded_apply(P, _randn(kind, 3, dims[0] * dims[1], 7))


@pytest.mark.parametrize("fused", [False, True], ids=["run_band", "fused"])
def test_nothing_stored_outside_y_banded(fused):
    from hipgp_amd import plan as hp
    dims = (50, 37)
    grids = [np.linspace(-1, 1, m) for m in dims]
    col = zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("sqexp", x, y, (1., .07)), 1e-3)
    P = hp.ToeplitzPlan(dims, torch.float32, DEV)
    with _env(HGP_BAND_FUSED="1" if fused else "0"):
        P.set_column(torch.tensor(col, device=DEV, dtype=torch.float32))
    assert _band(P) == (1, (9, 7)) and _band_fused(P) == int(fused)
    _guarded_apply(P, _randn("f32", 3, dims[0] * dims[1], 7))


# ---- fp64 plans with an H = 8192 axis -----------------------------------------------------------
@pytest.mark.parametrize("dims", sc.FALLBACK_F64, ids=[sc.case_id(d) for d in sc.FALLBACK_F64])
def test_fp64_longest_lines_take_the_general_passes(dims):
    from hipgp_amd import _lib
    from hipgp_amd import plan as hp
    c = _stored("f64", dims)
    P, ncl = _sep_plan("f64", dims, c)
    Q = hp.ToeplitzPlan(dims, torch.float64, DEV)
    with _env(HGP_SEPARABLE="0"):
        Q.set_column(c)
    assert _sep(P) == 0 and _sep(Q) == 0 and ncl == 0
    x = _randn("f64", 2, dims[0] * dims[1], 5)
    y = P.apply(_lib.OP_K, x)
    assert torch.equal(y, Q.apply(_lib.OP_K, x))
    ref = zo.ToeplitzOracle(c.cpu().numpy(), dims).matmul_K(x.cpu().numpy())
    err = float(np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max())
    print(f"f64 {dims}: general passes, error {err:.3e}")
    assert err < 1e-10, err


# ---- chunking does not change a bit -------------------------------------------------------------
NRHS = 11
SETTINGS = ["ws0", "wsmid", "streams1"]
# HGP_WS_MB is whole MiB: at 150 x 37 and 600 x 11 one MiB already admits every right-hand side a
# stream gets (6 of 11), so the 2-3 per chunk of "wsmid" are reached at 9 x 2048 (256 KiB and 512 KiB
# per right-hand side) -- and for run_band at 256 x 256
CHUNK_SEP = [(k, d) for d in ((150, 37), (600, 11), (9, 2048)) for k in ("f32", "f64")]
#             dims       ell  radii
CHUNK_BAND = [((96, 80), .05, (13, 11)), ((256, 256), .01, (7, 7))]


def _setting(name, per):
    """(environment of the plan's creation, right-hand sides per chunk it admits) with `per` bytes of
    workspace per right-hand side: HGP_WS_MB=0 -> 1; 'wsmid' -> room for 3 on each of the 2 streams,
    in whole MiB (at least 1)"""
    if name == "ws0":
        return dict(HGP_WS_MB="0"), 1
    if name == "streams1":
        return dict(HGP_STREAMS="1"), min(NRHS, 8)
    mb = max(1, (3 * per * 2) >> 20)
    return dict(HGP_WS_MB=str(mb)), min((NRHS + 1) // 2, (mb << 20) // (per * 2))


def _three_calls_equal(P, x, ref):
    from hipgp_amd import _lib
    y = torch.empty_like(ref)
    for rep in range(3):                                   # direct, captured, replayed
        y.fill_(float("nan"))
        P.apply(_lib.OP_K, x, out=y)
        assert torch.equal(y, ref), rep


@pytest.fixture
def fresh_plans():
    """plans that read HGP_WS_MB / HGP_STREAMS must come from hgp_plan_create, not from the pool of
    idle plans, and must not enter it afterwards"""
    from hipgp_amd import plan as hp
    gc.collect()
    hp.release_pool()
    yield
    gc.collect()
    hp.release_pool()


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("kind,dims", CHUNK_SEP, ids=[f"{k}_{sc.case_id(d)}" for k, d in CHUNK_SEP])
def test_chunking_is_bitwise_neutral(kind, dims, setting, fresh_plans):
    from hipgp_amd import _lib
    c = _stored(kind, dims)
    x = _randn(kind, NRHS, dims[0] * dims[1], 11)
    D, _ = _sep_plan(kind, dims, c)
    ref = D.apply(_lib.OP_K, x).clone()
    per = dims[1] * ((dims[0] + 31) // 32 * 32) * (4 if kind == "f32" else 8)
    env, qc = _setting(setting, per)
    if setting == "wsmid" and dims == (9, 2048):
        assert qc in (2, 3), qc
    print(f"{kind} {dims} {setting}: {env}, {qc} right-hand sides per chunk of {NRHS}")
    S, _ = _sep_plan(kind, dims, c, **env)
    try:
        assert _sep(D) == 1 and _sep(S) == 1 and _band(D)[0] == 0 and _band(S)[0] == 0
        _three_calls_equal(S, x, ref)
    finally:
        del S, D


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("dims,ell,radii", CHUNK_BAND, ids=[sc.case_id(d) for d, _, _ in CHUNK_BAND])
def test_run_band_chunking_equals_the_fused_kernel(dims, ell, radii, setting, fresh_plans):
    """the two banded paths agree bit for bit -- under any chunking of run_band"""
    from hipgp_amd import _lib
    from hipgp_amd import plan as hp
    grids = [np.linspace(-1, 1, m) for m in dims]
    col = zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval("sqexp", x, y, (1., ell)), 1e-3)
    c = torch.tensor(col, device=DEV, dtype=torch.float32)
    x = _randn("f32", NRHS, dims[0] * dims[1], 11)
    F = hp.ToeplitzPlan(dims, torch.float32, DEV)
    F.set_column(c)
    ref = F.apply(_lib.OP_K, x).clone()
    env, qc = _setting(setting, dims[0] * dims[1] * 4)
    if setting == "wsmid" and dims == (256, 256):
        assert qc in (2, 3), qc
    print(f"run_band {dims} {setting}: {env}, {qc} right-hand sides per chunk of {NRHS}")
    with _env(**env):
        S = hp.ToeplitzPlan(dims, torch.float32, DEV)
    with _env(HGP_BAND_FUSED="0"):
        S.set_column(c)
    try:
        assert _band(F) == (1, radii) and _band_fused(F) == 1
        assert _band(S) == (1, radii) and _band_fused(S) == 0
        _three_calls_equal(S, x, ref)
    finally:
        del S, F
