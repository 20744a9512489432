"""The windowed line-integral Kuf products on the device (hgp_kuf_semi_{mc,sqexp}_{matvec,rmatvec}_win behind
`kuf.LineWindowPlan` and the four `kuf.kuf_semi_*_win` functions) and the model methods on them.

Line n is the segment from the origin to x_n, cut into plan.pieces[n] pieces; its window is the set of nodes
in the bounding box of some piece widened by rho on every axis.  THE MASK of a case is what the kernels
realise: the non-zero pattern of the transposed product with one-hot coefficients on a plan with the case's
lines, rho and pieces but ell = 10 and the two-node Monte-Carlo mean (the window depends on neither the kernel
nor the estimator, and that value, |x| times a mean of numbers near sig2, is never 0; with the case's own ell
a mean of few nodes underflows far from them, and a short line's analytic difference of two CDFs cancels in
fp32).  Torch restates the
predicate in fp64 from the inputs in the test dtype and must sandwich it:
    Chebyshev tube at rho (1 - 1e-5)  <=  mask  <=  union of the piece boxes widened by rho (1 + 1e-5).
The tube of a line is { u : min_a max_axis |u - a x| <= r, a in [0, 1] }; the lines x = 0 (element |x| * mean
= 0) and NaN have no window by definition and are left out of the lower set.  Every grid lies on [0, 1], so
every real line starts on the hull: the "window is empty because the line is far outside" case runs on the
same grids moved to [0.5, 1.5] (`test_lines_that_miss_the_grid_give_exact_zeros`).

Values, against the fp64 forward (`kuf.kuf_semi_mc` / `kuf.kuf_semi_sqexp` in fp64) times the mask, relative to
S = max over the other index of sum |K64| |w| (or |c|), by the rules of tests/test_kuf_win_gpu.py:
    fp64: |error| <= 1e-10 S;   fp32: <= 4 x the error of torch's own fp32 masked product + 1e-7 S.
Truncation, against the dense fp64 product: |dense - windowed| <= tol sig2 |x_n| sum |w| + 1e-10 S.
Each test prints its figures before it asserts."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# grid -> rho: 4 .. 9 steps of every axis (steps 1 / (m - 1))
GRIDS = {(300,): 0.02, (70, 90): 0.07, (20, 18, 33): 0.27}
# kernel, nu, estimator, npts
MODES = [("sqexp", None, "sqexp", 0), ("sqexp", None, "mc", 10), ("matern", 0.5, "mc", 33), ("matern", 2.5, "mc", 1)]
NOBS = (1, 67, 300)                    # 300 crosses the 256-line chunk of the gather
NWS = (1, 8, 9)                        # 9: a group of 8 rows and a tail group
SIG2 = 1.3
F64_BOUND = 1e-10
F32_FLOOR = 1e-7
SLACK = 1e-5
did = lambda d: "x".join(map(str, d))
mid = lambda m: f"{m[0]}{m[1] or ''}-{m[2]}{m[3] or ''}"
ALL = [(d, m, t) for d in GRIDS for m in MODES for t in ("f64", "f32")]
ALL_IDS = [f"{did(d)}-{mid(m)}-{t}" for d, m, t in ALL]


def _kern(kind, nu, dtype):
    import ziggy.kernels as zk
    return zk.SqExp(dtype=dtype) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dtype)


def _mesh(grids):
    return torch.stack([a.reshape(-1) for a in torch.meshgrid(*grids, indexing="ij")], dim=-1)


def _lines(d, rho, dtype):
    """300 lines' end points in dtype (CPU).  0: a long diagonal; 1: x = 0; 2: NaN; 3: along the last axis (the
    others exactly 0); 4: along the first; 5: shorter than rho (one piece); 6: the end outside the hull; 7: into
    the negative orthant (only the nodes near the origin); then random ends in [-0.2, 1.2]^d, every fifth short."""
    g = torch.Generator().manual_seed(7 + d)
    x = torch.rand(300, d, generator=g, dtype=torch.float64) * 1.4 - 0.2
    x[8::5] *= torch.rand(x[8::5].shape[0], 1, generator=g, dtype=torch.float64) * 0.2
    x[0] = 0.97
    x[1] = 0.
    x[2] = float("nan")
    x[3] = 0.
    x[3, -1] = 0.83
    x[4] = 0.
    x[4, 0] = 0.61
    x[5] = 0.4 * rho
    x[6] = 1.3
    x[6, 0] = 0.8
    x[7] = -0.6
    return x.to(dtype)


def _forward(c, x, grids, dtype):
    from hipgp_amd import kuf
    k = _kern(c["mode"][0], c["mode"][1], dtype)
    if c["mode"][2] == "sqexp":
        return kuf.kuf_semi_sqexp(k, grids, x, c["params"])
    return kuf.kuf_semi_mc(k, grids, x, c["params"], c["npts"], u=c["u"])


def _mv(c, plan, W):
    from hipgp_amd import kuf
    if c["mode"][2] == "sqexp":
        return kuf.kuf_semi_sqexp_matvec_win(plan, W)
    return kuf.kuf_semi_mc_matvec_win(plan, W, c["npts"], u=c["u"])


def _rmv(c, plan, C):
    from hipgp_amd import kuf
    if c["mode"][2] == "sqexp":
        return kuf.kuf_semi_sqexp_rmatvec_win(plan, C)
    return kuf.kuf_semi_mc_rmatvec_win(plan, C, c["npts"], u=c["u"])


def _plan(c, nobs, rho=None, x=None, wide=False):
    """The case's plan for its first nobs lines; wide: ell = 10, the plan the mask is read from."""
    from hipgp_amd import kuf
    x = c["x"] if x is None else x
    return kuf.LineWindowPlan(c["k"], c["grids"], x[:nobs], (SIG2, 10.) if wide else c["params"], 1e-6,
                              rho=c["rho"] if rho is None else rho)


def _one_hot_rows(c, plan):
    """The windowed matrix (nobs, M) in the case dtype: the transposed product with C = I."""
    n = plan.nobs
    return _rmv(c, plan, torch.eye(n, dtype=c["dtype"], device=DEV))


def _mask_rows(c, wide):
    """The mask (nobs, M) of a wide plan through the transposed product."""
    from hipgp_amd import kuf
    return kuf.kuf_semi_mc_rmatvec_win(wide, torch.eye(wide.nobs, dtype=c["dtype"], device=DEV), 2, u=c["u"]) != 0


@functools.lru_cache(maxsize=None)
def _case(dims, mode, tag):
    """Everything of one (grid, kernel and estimator, dtype): computed once, shared, never changed."""
    dtype = torch.float64 if tag == "f64" else torch.float32
    rho = GRIDS[dims]
    c = dict(dims=dims, mode=mode, dtype=dtype, rho=rho, npts=mode[3], params=(SIG2, rho / 2))
    c["k"] = _kern(mode[0], mode[1], dtype)
    c["grids"] = [torch.linspace(0, 1, m, dtype=torch.float64).to(dtype).to(DEV) for m in dims]
    c["x"] = _lines(len(dims), rho, dtype).to(DEV)
    c["u"] = torch.tensor([0.37], dtype=dtype, device=DEV)
    c["M"] = int(torch.tensor(dims).prod())
    g64, x64 = [g.double() for g in c["grids"]], c["x"].double()
    K64 = _forward(c, x64, g64, torch.float64)
    c["plan"] = _plan(c, 300)
    Kw = _one_hot_rows(c, c["plan"])
    c["Kw"], c["mask"] = Kw, _mask_rows(c, _plan(c, 300, wide=True))
    c["K64"] = torch.nan_to_num(K64, nan=0.)                           # x = 0 (sqexp) and NaN rows: not in any window
    c["KM"] = torch.where(c["mask"], c["K64"], torch.zeros_like(K64))
    c["Kfwd"] = _forward(c, c["x"], c["grids"], dtype)
    c["K32m"] = torch.where(c["mask"], torch.nan_to_num(c["Kfwd"], nan=0.), torch.zeros_like(c["Kfwd"]))
    g = torch.Generator().manual_seed(3)
    c["W"] = torch.randn(9, c["M"], generator=g, dtype=torch.float64).to(dtype).to(DEV)
    c["C"] = torch.randn(9, 300, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    return c


def _tube(x64, mesh64, r):
    """(nobs, M) bool in fp64: the node is within Chebyshev distance r of the segment {a x : a in [0, 1]}: the
    intervals {a : |u_k - a x_k| <= r} of the axes and [0, 1] have a common point."""
    u, xv = mesh64[None, :, :], x64[:, None, :]
    e0, e1 = (u - r) / xv, (u + r) / xv
    lo, hi = torch.minimum(e0, e1), torch.maximum(e0, e1)
    flat = (xv == 0).expand_as(lo)                                     # the axis does not move: all a or none
    ok0 = (u.abs() <= r).expand_as(lo)
    lo = torch.where(flat, torch.where(ok0, torch.full_like(lo, -1.), torch.full_like(lo, 2.)), lo)
    hi = torch.where(flat, torch.where(ok0, torch.full_like(hi, 2.), torch.full_like(hi, -1.)), hi)
    return lo.amax(dim=-1).clamp(min=0.) <= hi.amin(dim=-1).clamp(max=1.)


def _boxes(x, pieces, mesh64, r):
    """(nobs, M) bool: the node is in the box of some piece widened by r; the pieces' ends in x's dtype, as the
    kernels form them, the comparisons in fp64."""
    out = torch.zeros(x.shape[0], mesh64.shape[0], dtype=torch.bool, device=x.device)
    P = pieces.to(x.dtype)
    for p in range(int(pieces.max())):
        t0 = (torch.full_like(P, p) / P)[:, None]
        t1 = (torch.full_like(P, p + 1) / P)[:, None]
        e0, e1 = (x * t0).double()[:, None, :], (x * t1).double()[:, None, :]
        lo, hi = torch.minimum(e0, e1), torch.maximum(e0, e1)
        u = mesh64[None, :, :]
        inside = ((lo - u <= r) & (u - hi <= r)).all(dim=-1) & (p < pieces)[:, None]
        out |= inside
    return out


def _sandwich(c, x, plan, mask, rho):
    mesh64 = _mesh([g.double() for g in c["grids"]])
    x64 = x.double()
    real = ~(torch.isnan(x64).any(dim=1) | (x64 == 0).all(dim=1))
    inner = _tube(x64, mesh64, rho * (1 - SLACK)) & real[:, None]
    outer = _boxes(x, plan.pieces, mesh64, rho * (1 + SLACK)) & real[:, None]
    exact = _tube(x64, mesh64, rho) & real[:, None]
    return mask, inner, outer, exact


@pytest.mark.parametrize("dims,mode,tag", ALL, ids=ALL_IDS)
def test_the_mask_is_one_set_in_both_kernels_and_lies_between_tube_and_boxes(dims, mode, tag):
    from hipgp_amd import kuf
    c = _case(dims, mode, tag)
    mask, inner, outer, exact = _sandwich(c, c["x"], c["plan"], c["mask"], c["rho"])
    nin, nmask, nout, nex = int(inner.sum()), int(mask.sum()), int(outer.sum()), int(exact.sum())
    print(f"{did(dims)} {mid(mode)} {tag}: pairs tube(1-s) {nin}, mask {nmask}, boxes(1+s) {nout}, exact tube {nex} "
          f"of {mask.numel()}; pieces {int(c['plan'].pieces.min())}..{int(c['plan'].pieces.max())}")
    assert bool((inner <= mask).all()), "a pair of the tube is missing from the window"
    assert bool((mask <= outer).all()), "the window holds a pair outside every widened piece box"
    assert 0 < nin <= nmask < mask.numel()
    assert int(mask[1].sum()) == 0 and int(mask[2].sum()) == 0          # x = 0 and NaN
    assert int(c["plan"].pieces[5]) == 1 and int(mask[5].sum()) > 0     # shorter than rho: one piece
    assert int(c["plan"].pieces[0]) > 1
    # the matvec with one-hot weights realises the same rows, bit for bit (the first 67 lines hold the special ones)
    p67, w67 = _plan(c, 67), _plan(c, 67, wide=True)
    rows, wrows = (torch.empty(67, c["M"], dtype=c["dtype"], device=DEV) for _ in range(2))
    for a in range(0, c["M"], 1024):
        b = min(a + 1024, c["M"])
        W = torch.zeros(b - a, c["M"], dtype=c["dtype"], device=DEV)
        W[torch.arange(b - a), torch.arange(a, b)] = 1
        rows[:, a:b] = _mv(c, p67, W)
        wrows[:, a:b] = kuf.kuf_semi_mc_matvec_win(w67, W, 2, u=c["u"])
    assert torch.equal(wrows != 0, mask[:67]), "the two kernels realise different sets"
    assert torch.equal(rows, c["Kw"][:67])
    assert bool(((c["Kw"] != 0) <= mask).all())
    # an in-window element is the dense forward's element, bit for bit
    assert torch.equal(c["Kw"][mask], c["Kfwd"][mask])


@pytest.mark.parametrize("dims,mode,tag", ALL, ids=ALL_IDS)
def test_matvec_win_matches_the_masked_forward(dims, mode, tag):
    c = _case(dims, mode, tag)
    worst = 0.
    for nobs in NOBS:
        plan = _plan(c, nobs)
        for nw in NWS:
            W = c["W"][:nw]
            ref = c["KM"][:nobs] @ W.double().t()
            S = (c["K64"][:nobs].abs() @ W.double().abs().t()).amax(dim=0, keepdim=True)
            bound = F64_BOUND
            if tag == "f32":
                e32 = float((((c["K32m"][:nobs] @ W.t()).double() - ref).abs() / S).max())
                bound = 4 * e32 + F32_FLOOR
            out = _mv(c, plan, W)
            err = float(((out.double() - ref).abs() / S).max())
            worst = max(worst, err / bound)
            print(f"mv {did(dims)} {mid(mode)} {tag} nobs {nobs} nw {nw}: err/S {err:.3e} bound {bound:.3e}")
            assert tuple(out.shape) == (nobs, nw) and err <= bound
            assert torch.equal(out, _mv(c, plan, W)), "two calls with equal arguments differ"
            if nobs >= 3:
                assert bool((out[1:3] == 0).all()), "x = 0 and NaN lines must give exact zeros"


@pytest.mark.parametrize("dims,mode,tag", ALL, ids=ALL_IDS)
def test_rmatvec_win_matches_the_masked_forward(dims, mode, tag):
    c = _case(dims, mode, tag)
    for nobs in NOBS:
        plan = _plan(c, nobs)
        for nc in NWS:
            C = c["C"][:nc, :nobs].contiguous()
            ref = C.double() @ c["KM"][:nobs]
            S = (C.double().abs() @ c["K64"][:nobs].abs()).amax(dim=1, keepdim=True)
            bound = F64_BOUND
            if tag == "f32":
                e32 = float((((C @ c["K32m"][:nobs]).double() - ref).abs() / S).max())
                bound = 4 * e32 + F32_FLOOR
            out = _rmv(c, plan, C)
            err = float(((out.double() - ref).abs() / S).max())
            print(f"rmv {did(dims)} {mid(mode)} {tag} nobs {nobs} nc {nc}: err/S {err:.3e} bound {bound:.3e}")
            assert tuple(out.shape) == (nc, c["M"]) and err <= bound
            assert torch.equal(out, _rmv(c, plan, C)), "two calls with equal arguments differ"


@pytest.mark.parametrize("dims,mode", [(d, m) for d in GRIDS for m in MODES], ids=lambda v: did(v) if len(v) < 4 else mid(v))
def test_the_two_products_are_transposes_fp64(dims, mode):
    c = _case(dims, mode, "f64")
    w, cc = c["W"][:1], c["C"][:1]
    f = _mv(c, c["plan"], w).reshape(-1)
    b = _rmv(c, c["plan"], cc).reshape(-1)
    lhs, rhs = float(cc.reshape(-1) @ f), float(b @ w.reshape(-1))
    scale = float(cc.abs().reshape(-1) @ (c["KM"].abs() @ w.abs().reshape(-1)))
    print(f"transpose {did(dims)} {mid(mode)}: <c, Kw> {lhs:.15e}  <K^T c, w> {rhs:.15e}  scale {scale:.3e}")
    assert abs(lhs - rhs) <= 1e-13 * scale


@pytest.mark.parametrize("tol", [1e-4, 1e-12], ids=lambda t: f"{t:.0e}")
@pytest.mark.parametrize("dims,mode", [(d, m) for d in GRIDS for m in MODES[:3]], ids=lambda v: did(v) if len(v) < 4 else mid(v))
def test_the_stated_truncation_bound_holds(dims, mode, tol):
    """ell is chosen so that support_radius(tol = 1e-12) is the grid's rho; the plan takes its radius from tol.
    The bound is stated for exact sums, so it is asserted in fp64, with the fp64 exactness rule for the sums' rounding."""
    from hipgp_amd import kuf
    tag = "f64"
    c = _case(dims, mode, tag)
    k = c["k"]
    ell = GRIDS[dims] / kuf.support_radius(_kern(mode[0], mode[1], torch.float64), (SIG2, 1.0), 1e-12)
    params = (SIG2, ell)
    x = c["x"][3:70].contiguous()
    plan = kuf.LineWindowPlan(k, c["grids"], x, params, tol)
    assert plan.rho == kuf.support_radius(k, params, tol)
    W, C = c["W"][:3], c["C"][:3, :67].contiguous()
    k64, g64, x64 = _kern(mode[0], mode[1], torch.float64), [g.double() for g in c["grids"]], x.double()
    if mode[2] == "sqexp":
        mvw, rmvw = kuf.kuf_semi_sqexp_matvec_win(plan, W), kuf.kuf_semi_sqexp_rmatvec_win(plan, C)
        K64 = kuf.kuf_semi_sqexp(k64, g64, x64, params)
    else:
        mvw = kuf.kuf_semi_mc_matvec_win(plan, W, c["npts"], u=c["u"])
        rmvw = kuf.kuf_semi_mc_rmatvec_win(plan, C, c["npts"], u=c["u"])
        K64 = kuf.kuf_semi_mc(k64, g64, x64, params, c["npts"], u=c["u"].double())
    xn = torch.linalg.vector_norm(x64, dim=1)
    mv, rmv = K64 @ W.double().t(), C.double() @ K64
    lim_mv = tol * SIG2 * xn[:, None] * W.double().abs().sum(dim=1)[None, :]
    lim_rmv = (tol * SIG2 * (C.double().abs() @ xn))[:, None]
    S_mv = (K64.abs() @ W.double().abs().t()).amax(dim=0, keepdim=True)
    S_rmv = (C.double().abs() @ K64.abs()).amax(dim=1, keepdim=True)
    rnd = F64_BOUND
    g_mv, g_rmv = (mvw.double() - mv).abs(), (rmvw.double() - rmv).abs()
    print(f"truncation {did(dims)} {mid(mode)} tol {tol:.0e} {tag}: rho {plan.rho:.4f}; matvec max gap {float(g_mv.max()):.3e} "
          f"(limit {float(lim_mv.max()):.3e}); rmatvec max gap {float(g_rmv.max()):.3e} (limit {float(lim_rmv.max()):.3e})")
    assert bool((g_mv <= lim_mv + rnd * S_mv).all())
    assert bool((g_rmv <= lim_rmv + rnd * S_rmv).all())


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_a_line_of_more_than_64_pieces_is_capped_and_still_a_superset(tag):
    """rho = 0.004 on the 300 grid: the long lines ask for up to 300 pieces and get 64 longer ones.  The
    sandwich is a statement about 1e-5 rho = 4e-8, under fp32's rounding of the ends, so fp32 is held to the
    two products realising one set and to the tube at rho (1 - 1e-3)."""
    from hipgp_amd import kuf
    c = _case((300,), MODES[1], tag)
    rho = 0.004
    plan = _plan(c, 300, rho=rho)
    assert int(plan.pieces.max()) == kuf.LINE_MAX_PIECES and float((c["x"][0].abs().max()) / rho) > 64
    Kw = _one_hot_rows(c, plan)
    wide = _plan(c, 300, rho=rho, wide=True)
    mask = _mask_rows(c, wide)
    s = SLACK if tag == "f64" else 1e-3
    mesh64 = _mesh([g.double() for g in c["grids"]])
    real = ~(torch.isnan(c["x"]).any(dim=1) | (c["x"] == 0).all(dim=1))
    inner = _tube(c["x"].double(), mesh64, rho * (1 - s)) & real[:, None]
    outer = _boxes(c["x"], plan.pieces, mesh64, rho * (1 + s)) & real[:, None]
    print(f"cap {tag}: pairs tube {int(inner.sum())}, mask {int(mask.sum())}, boxes {int(outer.sum())}")
    assert bool((inner <= mask).all()) and bool((mask <= outer).all())
    W = torch.eye(300, dtype=c["dtype"], device=DEV)
    assert torch.equal(_mv(c, plan, W), Kw) and torch.equal(kuf.kuf_semi_mc_matvec_win(wide, W, 2, u=c["u"]) != 0, mask)
    assert bool(((Kw != 0) <= mask).all())
    assert torch.equal(Kw[mask], c["Kfwd"][mask])


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("dims", list(GRIDS), ids=did)
def test_lines_that_miss_the_grid_give_exact_zeros(dims, tag):
    """The grids moved to [0.5, 1.5]: lines into the negative orthant, short lines and x = 0 stay farther than
    rho from the hull on some axis and have an empty window; the diagonal still crosses the grid."""
    from hipgp_amd import kuf
    c = _case(dims, MODES[2], tag)
    grids = [g + 0.5 for g in c["grids"]]
    x = c["x"][:8].clone()
    x[6] = 0.2
    plan = kuf.LineWindowPlan(c["k"], grids, x, c["params"], 1e-6, rho=c["rho"])
    out = kuf.kuf_semi_mc_matvec_win(plan, c["W"][:3].abs(), c["npts"], u=c["u"])
    assert bool((out[0] > 0).all())
    assert bool((out[[1, 2, 5, 6, 7]] == 0).all())
    back = kuf.kuf_semi_mc_rmatvec_win(plan, torch.eye(8, dtype=c["dtype"], device=DEV), c["npts"], u=c["u"])
    assert bool((back[[1, 2, 5, 6, 7]] == 0).all()) and bool((back[0] != 0).any())


def _raw(name, c, plan, rows, out_ptr, mc):
    from hipgp_amd import _lib
    from hipgp_amd.kuf import _grid_ptrs
    x = plan.x
    m, ptrs = _grid_ptrs(plan.grids)
    head = [_lib.dtype_code(x.dtype)] + ([plan.kind] if mc else []) + \
           [len(plan.grids), m, ptrs, ctypes.c_void_p(x.data_ptr()), x.shape[0], plan.sig2, plan.ell, plan.rho]
    if mc:
        head += [c["npts"], ctypes.c_void_p(c["u"].data_ptr())]
    _lib.check(getattr(_lib.lib(), name)(*head, ctypes.c_void_p(plan.pieces.data_ptr()), plan.pieces.shape[0],
                                         ctypes.c_void_p(rows.data_ptr()), rows.shape[0], ctypes.c_void_p(out_ptr),
                                         _lib.stream_ptr(x.device)))


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("mode", [MODES[0], MODES[2]], ids=mid)
@pytest.mark.parametrize("dims", list(GRIDS), ids=did)
def test_guard_rows_around_out_are_untouched(dims, mode, tag):
    c = _case(dims, mode, tag)
    mc = mode[2] == "mc"
    est = "mc" if mc else "sqexp"
    for nobs in (67, 300):
        plan = _plan(c, nobs)
        for nw in (1, 9):
            buf = torch.full((nobs + 2, nw), float("nan"), dtype=c["dtype"], device=DEV)
            _raw(f"hgp_kuf_semi_{est}_matvec_win", c, plan, c["W"][:nw].contiguous(), buf[1:].data_ptr(), mc)
            torch.cuda.synchronize()
            assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())
            assert torch.equal(buf[1:-1], _mv(c, plan, c["W"][:nw]))
            buf = torch.full((nw + 2, c["M"]), float("nan"), dtype=c["dtype"], device=DEV)
            _raw(f"hgp_kuf_semi_{est}_rmatvec_win", c, plan, c["C"][:nw, :nobs].contiguous(), buf[1:].data_ptr(), mc)
            torch.cuda.synchronize()
            assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())
            assert torch.equal(buf[1:-1], _rmv(c, plan, c["C"][:nw, :nobs].contiguous()))


def test_no_lines_bad_piece_counts_and_declines():
    from hipgp_amd import _lib, kuf
    c = _case((70, 90), MODES[0], "f64")
    empty = _plan(c, 0)
    out = kuf.kuf_semi_sqexp_rmatvec_win(empty, torch.zeros(3, 0, dtype=c["dtype"], device=DEV))
    assert tuple(out.shape) == (3, c["M"]) and bool((out == 0).all())
    assert tuple(kuf.kuf_semi_sqexp_matvec_win(empty, c["W"][:2]).shape) == (0, 2)
    # piece counts outside 1 .. 64 are clamped in the kernels: the two products still agree, nothing faults
    plan = _plan(c, 67)
    good = plan.pieces.clone()
    plan.pieces = torch.where(torch.arange(67, device=DEV) % 2 == 0, torch.full_like(good, -5), torch.full_like(good, 1000))
    Kw = _one_hot_rows(c, plan)
    W = torch.zeros(2048, c["M"], dtype=c["dtype"], device=DEV)
    W[torch.arange(2048), torch.arange(2048)] = 1
    rows = kuf.kuf_semi_sqexp_matvec_win(plan, W)
    assert torch.equal(rows, Kw[:, :2048])
    # a piece array of the wrong length is refused before any launch
    plan.pieces = good[:10].contiguous()
    with pytest.raises(_lib.HipgpError, match="pieces"):
        kuf.kuf_semi_sqexp_matvec_win(plan, c["W"][:1])
    with pytest.raises(_lib.HipgpError, match="pieces"):
        kuf.kuf_semi_sqexp_rmatvec_win(plan, c["C"][:1, :67])
    # analytic entries are SqExp's alone
    cm = _case((70, 90), MODES[2], "f64")
    assert kuf.kuf_semi_sqexp_matvec_win(cm["plan"], cm["W"][:1]) is None
    assert kuf.kuf_semi_sqexp_rmatvec_win(cm["plan"], cm["C"][:1]) is None


# ---- the model: 32 x 32 x 16 grid on [0, 1], SqExp, fp64, 100 lines ------------------------------------------
T_MODEL = 1e-12


@functools.lru_cache(maxsize=None)
def _model_case():
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    dt = torch.float64
    grids = [torch.linspace(0, 1, m, dtype=dt) for m in (32, 32, 16)]
    torch.manual_seed(5)
    mod = hg.MeanFieldToeplitzGP(zk.SqExp(dtype=dt), grids, num_obs=100, sig2_init=1., ell_init=.03, noise2_init=.05,
                                 learn_kernel=False, dtype=dt)
    g = torch.Generator(device="cpu").manual_seed(11)
    with torch.no_grad():
        mod.global_theta2.copy_(-(torch.rand(mod.Mprime, 1, generator=g, dtype=dt) * 4 + .5))
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=dt))
    mod = mod.cuda_params(0)
    x = (torch.rand(100, 3, generator=g, dtype=dt) * 1.1 + 0.02).to(DEV)
    sd = (torch.rand(100, 1, generator=g, dtype=dt) * .4 + .1).to(DEV)
    y = (torch.sin(3 * x[:, :1]) * torch.linalg.vector_norm(x, dim=1, keepdim=True)
         + sd * torch.randn(100, 1, generator=g, dtype=dt).to(DEV))
    return mod, x, y, sd


class _knob:
    def __init__(self, mod, t):
        self.mod, self.t = mod, t

    def __enter__(self):
        self.mod.kuf_line_support_tol = self.t

    def __exit__(self, *a):
        self.mod.kuf_line_support_tol = None


def _spy(monkeypatch, names):
    from hipgp_amd import kuf
    calls = []
    for nm in names:
        real = getattr(kuf, nm)
        monkeypatch.setattr(kuf, nm, (lambda real, nm: lambda *a, **k: calls.append((nm, a)) or real(*a, **k))(real, nm))
    return calls


DENSE = ("kuf_semi_sqexp_matvec", "kuf_semi_sqexp_rmatvec", "kuf_semi_mc_matvec", "kuf_semi_mc_rmatvec")
WIN = ("kuf_semi_sqexp_matvec_win", "kuf_semi_sqexp_rmatvec_win", "kuf_semi_mc_matvec_win", "kuf_semi_mc_rmatvec_win")


@pytest.mark.parametrize("est", ["analytic", "mc-biased"])
def test_predict_mean_with_a_line_tolerance_is_within_the_stated_bound(est, monkeypatch):
    from hipgp_amd import kuf
    mod, x, _, _ = _model_case()
    alpha = mod.mean_weights()
    sig2 = float(mod.get_kernel_params()[0])
    u = torch.tensor([0.25], dtype=torch.float64, device=DEV)
    kw = dict(weights=alpha, integrated_obs=True, semi_integrated_estimator=est, semi_integrated_samps=7, mc_offset=u)
    calls = _spy(monkeypatch, DENSE + WIN)
    mu = mod.predict_mean(x, **kw)
    assert [c[0] for c in calls] == [DENSE[0] if est == "analytic" else DENSE[2]], "the knob unset: the dense product"
    del calls[:]
    with _knob(mod, T_MODEL):
        mu_t = mod.predict_mean(x, **kw)
    assert [c[0] for c in calls] == [WIN[0] if est == "analytic" else WIN[2]]
    xn = torch.linalg.vector_norm(x, dim=1).cpu()
    limit = T_MODEL * sig2 * xn * float(alpha.abs().sum()) + F64_BOUND * float(mu.abs().max())
    gap = (mu_t - mu).abs().reshape(-1)
    rho = kuf.support_radius(mod.kernel, mod.get_kernel_params(), T_MODEL)
    print(f"predict_mean {est} line tol {T_MODEL:.0e}: rho {rho:.4f} ({rho * 31:.1f} steps); max gap {float(gap.max()):.3e}, "
          f"limit {float(limit.max()):.3e}; max|mu| {float(mu.abs().max()):.3e}")
    assert tuple(mu_t.shape) == (100, 1) and bool((gap <= limit).all())
    # unset: bit-equal to the dense function's own result
    if est == "analytic":
        dense = kuf.kuf_semi_sqexp_matvec(mod.kernel, mod.xgrids, x, mod.get_kernel_params(), alpha)
    else:
        dense = kuf.kuf_semi_mc_matvec(mod.kernel, mod.xgrids, x, mod.get_kernel_params(), 7, u=u, W=alpha)
    assert torch.equal(mu, dense.reshape(-1, 1).cpu())
    # the point knob still refuses line integrals
    with pytest.raises(NotImplementedError, match="tube"):
        try:
            mod.kuf_support_tol = 1e-6
            mod.predict_mean(x, **kw)
        finally:
            mod.kuf_support_tol = None


def test_fit_mean_with_a_line_tolerance_solves_the_dense_system_to_the_derived_bound(monkeypatch):
    """beta of the windowed fit in the DENSE system: |b - A beta| <= tol_cg |b| + |dA| |beta| + |db| with
    dA = Kuf^T D Kuf - KufM^T D KufM and db = (Kuf - KufM)^T D y formed here from the dense forward and the
    windowed matrix (one-hot transposed product on the same radius); K is applied by the model's own operator."""
    from hipgp_amd import kuf
    mod, x, y, sd = _model_case()
    params = mod.get_kernel_params()
    tol_cg = 1e-9
    calls = _spy(monkeypatch, DENSE + WIN)
    dense_fit = mod.fit_mean(x, y, noise_std=sd, integrated_obs=True, tol=tol_cg, maxiter=3000, update=False)
    assert calls and all(c[0] in DENSE[:2] for c in calls), "the knob unset: the dense products"
    del calls[:]
    with _knob(mod, T_MODEL):
        fit = mod.fit_mean(x, y, noise_std=sd, integrated_obs=True, tol=tol_cg, maxiter=3000, update=False)
    assert calls and all(c[0] in WIN[:2] for c in calls)
    assert len({id(c[1][0]) for c in calls}) == 1, "one plan for the whole call"
    Kuf = kuf.kuf_semi_sqexp(mod.kernel, mod.xgrids, x, params)
    plan = kuf.LineWindowPlan(mod.kernel, mod.xgrids, x, params, T_MODEL)
    KufM = kuf.kuf_semi_sqexp_rmatvec_win(plan, torch.eye(100, dtype=torch.float64, device=DEV))
    iv, yv = (1 / sd ** 2).reshape(-1), y.reshape(-1)
    T = mod.toeplitz()
    T.set_batch_shape((1,))
    beta = fit.weights.reshape(1, -1)
    Ab = T._matmul_by_K(beta.contiguous()).reshape(-1) + Kuf.t() @ (iv * (Kuf @ beta.reshape(-1)))
    b = Kuf.t() @ (iv * yv)
    res = float(torch.linalg.vector_norm(b - Ab))
    E = Kuf - KufM
    Q, _ = torch.linalg.qr(torch.cat([Kuf, KufM], dim=0).t())
    EQ, KQ, MQ = E @ Q, Kuf @ Q, KufM @ Q
    Bq = EQ.t() @ (iv[:, None] * KQ) + MQ.t() @ (iv[:, None] * EQ)
    ndA = float(torch.linalg.eigvalsh(.5 * (Bq + Bq.t())).abs().max())
    ndb = float(torch.linalg.vector_norm(E.t() @ (iv * yv)))
    nb, nbeta = float(torch.linalg.vector_norm(b)), float(torch.linalg.vector_norm(beta))
    limit = tol_cg * nb + ndA * nbeta + ndb
    away = float((fit.qm - dense_fit.qm).abs().max() / dense_fit.qm.abs().max())
    print(f"fit_mean line tol {T_MODEL:.0e}: {fit.iters} iterations (dense {dense_fit.iters}), relres {fit.relres:.2e}; "
          f"|b - A beta| {res:.3e}, limit {limit:.3e} = tol|b| {tol_cg * nb:.3e} + |dA||beta| {ndA * nbeta:.3e} + |db| "
          f"{ndb:.3e}; dropped pairs {int((KufM == 0).sum())} of {KufM.numel()}; mean vs dense mean {away:.3e}")
    assert fit.relres < tol_cg and fit.iters < 3000
    assert res <= limit
    assert int((KufM == 0).sum()) > 0
    back = mod.fit_mean(x, y, noise_std=sd, integrated_obs=True, tol=tol_cg, maxiter=3000, update=False)
    assert torch.equal(back.weights, dense_fit.weights) and back.iters == dense_fit.iters
    with pytest.raises(NotImplementedError, match="tube"):
        try:
            mod.kuf_support_tol = 1e-6
            mod.fit_mean(x, y, noise_std=sd, integrated_obs=True, update=False)
        finally:
            mod.kuf_support_tol = None


def test_predict_line_samples_with_a_line_tolerance_moves_by_no_more_than_the_bound(monkeypatch):
    mod, x, _, _ = _model_case()
    g = torch.Generator().manual_seed(2)
    dt = torch.float64
    kw = dict(nfeat=64, eps=torch.randn(2, mod.Mprime, generator=g, dtype=dt),
              features=(torch.randn(64, 3, generator=g, dtype=dt) * 5, torch.rand(64, generator=g, dtype=dt)),
              prior_w=torch.randn(2, 64, generator=g, dtype=dt), nugget_eps=torch.randn(2, mod.M, generator=g, dtype=dt))
    calls = _spy(monkeypatch, DENSE + WIN)
    s0 = mod.predict_line_samples(x, 2, **kw)
    assert [c[0] for c in calls] == [DENSE[0]]
    del calls[:]
    with _knob(mod, T_MODEL):
        st = mod.predict_line_samples(x, 2, **kw)
    assert [c[0] for c in calls] == [WIN[0]]
    alpha = calls[0][1][1]                                             # the rows the product was given: (2, M)
    sig2 = float(mod.get_kernel_params()[0])
    xn = torch.linalg.vector_norm(x, dim=1).cpu()
    limit = T_MODEL * sig2 * alpha.abs().sum(dim=1).cpu()[:, None] * xn[None, :] + F64_BOUND * float(s0.abs().max())
    gap = (st - s0).abs()
    print(f"predict_line_samples line tol {T_MODEL:.0e}: max gap {float(gap.max()):.3e}, limit {float(limit.max()):.3e}")
    assert tuple(st.shape) == (2, 100) and bool((gap <= limit).all())
