"""The windowed Kuf products on the device (hgp_kuf_grid_matvec_win / hgp_kuf_grid_rmatvec_win behind
`kuf.WindowPlan`, `kuf.kuf_grid_matvec_win`, `kuf.kuf_grid_rmatvec_win`) and the model methods on them.

The window of a plan is the set of pairs (n, j) with |x[n, a] - g_a[j_a]| <= rho on every axis, in the
tensor dtype with rho rounded once to it.  The reference is the MASKED dense matrix in fp64: K64 =
kernel(x, mesh) as `tests/test_kuf_rmatvec_gpu.py::_torch_K` forms it, times the mask of that predicate
computed by torch from the inputs in the test dtype, as the kernels see them.

Exactness, against the masked reference: every error of an output is measured relative to S = max over the
other index of sum |K64| |w| (or |c|), under the bounds of the dense products' tests:
  fp64: |error| <= 1e-10 S;   fp32: <= 4 x the error of torch's own fp32 masked product + 1e-7 S.
Truncation, against the unmasked fp64 product: |windowed - dense| <= tol sig2 sum |w| + the bound above.
Each test prints its figures before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

KERNELS = [("sqexp", None), ("matern", 0.5), ("matern", 2.5)]
# grid -> the radius aimed at: between 4 and 9 steps of every axis (steps 2 / (m - 1))
GRIDS = {(300,): 0.0535, (70, 90): 0.2, (20, 18, 33): 0.5}
NOBS = (1, 67, 200)
NWS = (1, 3, 9)                        # 9: a group of 8 rows and a tail group
TOL = 1e-6
SIG2 = 1.3
F64_BOUND = 1e-10
F32_FLOOR = 1e-7
ADJ_F64_BOUND = 1e-12
kid = lambda k: f"{k[0]}{k[1] or ''}"
did = lambda d: "x".join(map(str, d))


def _kern(kind, nu, dtype):
    import ziggy.kernels as zk
    return zk.SqExp(dtype=dtype) if kind == "sqexp" else zk.Matern(nu=nu, dtype=dtype)


def _ell_for(kern, rho):
    """ell with support_radius(kernel, (SIG2, ell), TOL) = rho up to rounding: the radius is linear in ell."""
    from hipgp_amd import kuf
    return rho / kuf.support_radius(_kern(*kern, torch.float64), (SIG2, 1.0), TOL)


def _mesh(grids):
    return torch.stack([a.reshape(-1) for a in torch.meshgrid(*grids, indexing="ij")], dim=-1)


def _mask(x, grids, rho):
    """The predicate, by torch in x's dtype: (nobs, M) bool."""
    r = torch.tensor(rho, dtype=x.dtype, device=x.device)
    return ((x[:, None, :] - _mesh(grids)[None, :, :]).abs() <= r).all(dim=-1)


def _points(grids, rho, dtype, layout):
    """200 points in dtype on the CPU and the indices of the special ones.  "mixed": a node first (so
    that nobs = 1 is a node), the grid's corners, a point exactly rho from a node on every axis and its
    neighbour one ulp farther on the last axis, points outside the hull within and beyond rho, the rest
    uniform in [-1.1, 1.1]^d.  "onebin": all 200 strictly inside one cell, so one bin holds them all."""
    d = len(grids)
    g = torch.Generator(device="cpu").manual_seed(7)
    if layout == "onebin":
        lo = torch.stack([gr[len(gr) // 2] for gr in grids])
        hi = torch.stack([gr[len(gr) // 2 + 1] for gr in grids])
        u = torch.rand(200, d, generator=g, dtype=torch.float64) * 0.9 + 0.05
        return (lo.double() + (hi - lo).double() * u).to(dtype), {}
    r = torch.tensor(rho, dtype=dtype)
    node = torch.stack([gr[len(gr) // 3] for gr in grids])
    rows, special = [node], {"node": 0}
    rows += [torch.stack([gr[0] for gr in grids]), torch.stack([gr[-1] for gr in grids]),
             torch.stack([gr[0] if a % 2 == 0 else gr[-1] for a, gr in enumerate(grids)])]
    special["corners"] = (1, 2, 3)
    exact, at = [], []
    for gr in grids:                      # a node i with fl((g[i] + rho) - g[i]) == rho in dtype
        for i in sorted(range(len(gr)), key=lambda i: abs(i - len(gr) // 2)):
            xa = gr[i] + r
            if bool(xa - gr[i] == r) and bool(torch.nextafter(xa, xa + 1) - gr[i] > r):
                exact.append(xa)
                at.append(i)
                break
    assert len(exact) == d, "no node lies exactly rho from a representable point"
    exact = torch.stack(exact)
    beyond = exact.clone()
    beyond[-1] = torch.nextafter(exact[-1], exact[-1] + 1)
    special["exact"], special["beyond"], special["exact_node"] = len(rows), len(rows) + 1, tuple(at)
    rows += [exact, beyond]
    near, allnear, far, farneg = node.clone(), node.clone(), node.clone(), node.clone()
    near[0] = 1 + r / 2
    allnear[:] = 1 + r / 2
    far[-1] = 1 + 2 * r
    farneg[0] = -1 - 2 * r
    special["outside_within"] = (len(rows), len(rows) + 1)
    special["outside_beyond"] = (len(rows) + 2, len(rows) + 3)
    rows += [near, allnear, far, farneg]
    x = torch.stack(rows).to(dtype)
    rest = (torch.rand(200 - len(rows), d, generator=g, dtype=torch.float64) * 2.2 - 1.1).to(dtype)
    return torch.cat([x, rest], dim=0), special


def _weights(n, M, dtype, positive=False):
    g = torch.Generator(device="cpu").manual_seed(11 + M)
    mag = torch.rand(n, M, generator=g, dtype=dtype) + 0.5
    if positive:
        return mag.to(DEV)
    sign = (torch.randint(0, 2, (n, M), generator=g, dtype=torch.int64) * 2 - 1).to(dtype)
    return (sign * mag).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(dims, kern, tag, layout="mixed"):
    """Inputs in the test dtype, the plan, the fp64 dense and masked matrices on those same values and
    (fp32) torch's own fp32 masked matrix; computed once and shared, never changed."""
    from hipgp_amd import kuf
    dtype = torch.float64 if tag == "f64" else torch.float32
    ell = _ell_for(kern, GRIDS[dims])
    params = (SIG2, ell)
    k = _kern(*kern, dtype)
    rho = kuf.support_radius(k, params, TOL)
    cpu_grids = [torch.linspace(-1, 1, m, dtype=dtype) for m in dims]
    for gr in cpu_grids:                  # the radius spans 4 to 9 steps of every axis
        assert 4 <= rho / float(gr[1] - gr[0]) <= 9, (dims, rho)
    xc, special = _points(cpu_grids, rho, dtype, layout)
    grids = [gr.to(DEV) for gr in cpu_grids]
    x = xc.to(DEV)
    K64 = _kern(*kern, torch.float64).forward(x.double(), _mesh([gr.double() for gr in grids]), params=params)
    mask = _mask(x, grids, rho)
    K32m = None
    if tag == "f32":
        K32m = k.forward(x, _mesh(grids), params=params) * mask
    M = int(np.prod(dims))
    return dict(dims=dims, dtype=dtype, k=k, params=params, rho=rho, grids=grids, x=x, K64=K64, mask=mask,
                KM=K64 * mask, K32m=K32m, special=special, M=M, W=_weights(max(NWS), M, dtype),
                C=_weights(max(NWS), 200, dtype))


def _plan(c, nobs, rho=None):
    from hipgp_amd import kuf
    return kuf.WindowPlan(c["k"], c["grids"], c["x"][:nobs], c["params"], TOL, rho=rho)


def _mv_bound(c, nobs, nw, tag, K=None, K32=None):
    """(ref, S, bound) of the product of rows [:nobs] of K (default: the masked matrix) with W[:nw]."""
    K = c["KM"] if K is None else K
    W = c["W"][:nw]
    ref = K[:nobs] @ W.double().t()
    S = (c["K64"][:nobs].abs() @ W.double().abs().t()).amax(dim=0, keepdim=True)          # (1, nw)
    if tag == "f64":
        return ref, S, F64_BOUND, None
    K32 = c["K32m"] if K32 is None else K32
    e32 = float((((K32[:nobs] @ W.t()).double() - ref).abs() / S).max())
    return ref, S, 4 * e32 + F32_FLOOR, e32


def _rmv_bound(c, nobs, nc, tag, K=None, K32=None):
    K = c["KM"] if K is None else K
    C = c["C"][:nc, :nobs]
    ref = C.double() @ K[:nobs]
    S = (C.double().abs() @ c["K64"][:nobs].abs()).amax(dim=1, keepdim=True)              # (nc, 1)
    if tag == "f64":
        return ref, S, F64_BOUND, None
    K32 = c["K32m"] if K32 is None else K32
    e32 = float((((C @ K32[:nobs]).double() - ref).abs() / S).max())
    return ref, S, 4 * e32 + F32_FLOOR, e32


ALL = [(d, k, t) for d in GRIDS for k in KERNELS for t in ("f64", "f32")]
ALL_IDS = [f"{did(d)}-{kid(k)}-{t}" for d, k, t in ALL]


@pytest.mark.parametrize("layout", ["mixed", "onebin"])
@pytest.mark.parametrize("dims,kern,tag", ALL, ids=ALL_IDS)
def test_the_mask_is_non_trivial_and_the_points_are_what_they_claim(dims, kern, tag, layout):
    """Between 1 % and 60 % of the pairs are in the window for every nobs, and the special points sit
    where the other tests need them (checked on the CPU copy of the mask)."""
    c = _case(dims, kern, tag, layout)
    mask = c["mask"].cpu()
    for nobs in NOBS:
        frac = float(mask[:nobs].double().mean())
        print(f"{did(dims)} {kid(kern)} {tag} {layout} nobs={nobs}: {100 * frac:.2f} % of the pairs in the window")
        assert 0.01 <= frac <= 0.60
    if layout == "onebin":
        order, start = _plan(c, 200).bins()
        counts = (start[1:] - start[:-1]).cpu()
        assert int(counts.max()) == 200 and int((counts > 0).sum()) == 1, "the 200 points are not in one bin"
        assert sorted(order.cpu().tolist()) == list(range(200))
        return
    sp = c["special"]
    node = 0
    for i, m in zip(sp["exact_node"], dims):
        node = node * m + i
    assert bool(mask[sp["exact"], node]) and not bool(mask[sp["beyond"], node]), "the <= of the predicate is not hit"
    assert all(bool(mask[n].any()) for n in sp["corners"] + sp["outside_within"] + (sp["node"],))
    assert not any(bool(mask[n].any()) for n in sp["outside_beyond"])


@pytest.mark.parametrize("dims,kern,tag", ALL, ids=ALL_IDS)
def test_matvec_win_matches_the_masked_dense_product(dims, kern, tag):
    from hipgp_amd import kuf
    worst = 0.0
    for layout in ("mixed", "onebin"):
        c = _case(dims, kern, tag, layout)
        for nobs in NOBS:
            plan = _plan(c, nobs)
            assert plan.rho == c["rho"] and plan.nobs == nobs and plan.M == c["M"]
            for nw in NWS:
                ref, S, bound, e32 = _mv_bound(c, nobs, nw, tag)
                out = kuf.kuf_grid_matvec_win(plan, c["W"][:nw])
                assert tuple(out.shape) == (nobs, nw) and out.dtype == c["dtype"]
                assert torch.equal(out, kuf.kuf_grid_matvec_win(plan, c["W"][:nw])), "second call differs"
                e = float(((out.double() - ref).abs() / S).max())
                worst = max(worst, e)
                print(f"matvec_win {did(dims)} {kid(kern)} {tag} {layout} nobs={nobs} nw={nw}: |error|/S = {e:.3e}"
                      + ("" if e32 is None else f" (torch fp32: {e32:.3e})"))
                assert e <= bound, (dims, kern, tag, layout, nobs, nw, e, bound)
                if layout == "mixed" and nobs > 1:       # beyond rho from the hull: an empty window, exact zeros
                    for n in c["special"]["outside_beyond"]:
                        assert bool((out[n] == 0).all())
    print(f"matvec_win {did(dims)} {kid(kern)} {tag}: worst |error|/S = {worst:.3e}")


@pytest.mark.parametrize("dims,kern,tag", ALL, ids=ALL_IDS)
def test_rmatvec_win_matches_the_masked_dense_product(dims, kern, tag):
    from hipgp_amd import kuf
    worst = 0.0
    for layout in ("mixed", "onebin"):
        c = _case(dims, kern, tag, layout)
        for nobs in NOBS:
            plan = _plan(c, nobs)
            for nc in NWS:
                ref, S, bound, e32 = _rmv_bound(c, nobs, nc, tag)
                C = c["C"][:nc, :nobs]
                out = kuf.kuf_grid_rmatvec_win(plan, C)
                assert tuple(out.shape) == (nc, c["M"]) and out.dtype == c["dtype"]
                assert torch.equal(out, kuf.kuf_grid_rmatvec_win(plan, C)), "second call differs"
                e = float(((out.double() - ref).abs() / S).max())
                worst = max(worst, e)
                print(f"rmatvec_win {did(dims)} {kid(kern)} {tag} {layout} nobs={nobs} nc={nc}: |error|/S = {e:.3e}"
                      + ("" if e32 is None else f" (torch fp32: {e32:.3e})"))
                assert e <= bound, (dims, kern, tag, layout, nobs, nc, e, bound)
                untouched = ~c["mask"][:nobs].any(dim=0)                 # mesh points no observation reaches
                assert bool((out[:, untouched] == 0).all())
    print(f"rmatvec_win {did(dims)} {kid(kern)} {tag}: worst |error|/S = {worst:.3e}")


@pytest.mark.parametrize("dims,kern,tag", ALL, ids=ALL_IDS)
def test_the_stated_truncation_bound_holds(dims, kern, tag):
    """|windowed - dense fp64| <= tol sig2 sum |w| plus the exactness bound, and the transpose twin."""
    from hipgp_amd import kuf
    c = _case(dims, kern, tag)
    nobs = 200
    plan = _plan(c, nobs)
    for nw in NWS:
        W, C = c["W"][:nw], c["C"][:nw]
        _, S, bound, _ = _mv_bound(c, nobs, nw, tag)
        dense = c["K64"] @ W.double().t()
        gap = (kuf.kuf_grid_matvec_win(plan, W).double() - dense).abs()
        limit = TOL * SIG2 * W.double().abs().sum(dim=1)[None, :] + bound * S
        print(f"truncation matvec {did(dims)} {kid(kern)} {tag} nw={nw}: worst gap / limit = {float((gap / limit).max()):.3e}, "
              f"worst gap / (tol sig2 sum|w|) = {float((gap / (limit - bound * S)).max()):.3e}")
        assert bool((gap <= limit).all())
        _, S, bound, _ = _rmv_bound(c, nobs, nw, tag)
        dense = C.double() @ c["K64"]
        gap = (kuf.kuf_grid_rmatvec_win(plan, C).double() - dense).abs()
        limit = TOL * SIG2 * C.double().abs().sum(dim=1)[:, None] + bound * S
        print(f"truncation rmatvec {did(dims)} {kid(kern)} {tag} nc={nw}: worst gap / limit = {float((gap / limit).max()):.3e}")
        assert bool((gap <= limit).all())


@pytest.mark.parametrize("dims,kern,tag", ALL, ids=ALL_IDS)
def test_a_radius_over_the_whole_grid_gives_the_unmasked_product(dims, kern, tag):
    """rho = 4 exceeds every |x - u| here (points in [-1.2, 1.2], grid [-1, 1]): the exactness bound
    against the dense matrix itself."""
    from hipgp_amd import kuf
    c = _case(dims, kern, tag)
    nobs = 67
    plan = _plan(c, nobs, rho=4.0)
    assert bool(_mask(c["x"][:nobs], c["grids"], 4.0).all())
    K32 = None if tag == "f64" else c["k"].forward(c["x"], _mesh(c["grids"]), params=c["params"])
    for nw in NWS:
        ref, S, bound, _ = _mv_bound(c, nobs, nw, tag, K=c["K64"], K32=K32)
        e = float(((kuf.kuf_grid_matvec_win(plan, c["W"][:nw]).double() - ref).abs() / S).max())
        ref, S, rbound, _ = _rmv_bound(c, nobs, nw, tag, K=c["K64"], K32=K32)
        er = float(((kuf.kuf_grid_rmatvec_win(plan, c["C"][:nw, :nobs]).double() - ref).abs() / S).max())
        print(f"whole grid {did(dims)} {kid(kern)} {tag} n={nw}: matvec |error|/S = {e:.3e} (bound {bound:.3e}), "
              f"rmatvec {er:.3e} (bound {rbound:.3e})")
        assert e <= bound and er <= rbound


@pytest.mark.parametrize("dims,kern", [(d, k) for d in GRIDS for k in KERNELS],
                         ids=[f"{did(d)}-{kid(k)}" for d in GRIDS for k in KERNELS])
def test_the_two_products_are_transposes_fp64(dims, kern):
    """<c, matvec_win(w)> = <rmatvec_win(c), w> to 1e-12 relative, both sides accumulated in fp64 (positive
    w and c: nothing cancels, so relative to the value itself)."""
    from hipgp_amd import kuf
    for layout in ("mixed", "onebin"):
        c = _case(dims, kern, "f64", layout)
        for nobs in NOBS:
            plan = _plan(c, nobs)
            w = _weights(1, c["M"], torch.float64, positive=True)
            cc = _weights(1, nobs, torch.float64, positive=True)
            left = float(torch.sum(kuf.kuf_grid_matvec_win(plan, w)[:, 0] * cc[0]))
            right = float(torch.sum(kuf.kuf_grid_rmatvec_win(plan, cc)[0] * w[0]))
            gap = abs(left - right) / abs(left)
            print(f"transpose {did(dims)} {kid(kern)} {layout} nobs={nobs}: <c, Kw> = {left:.15e}, relative gap {gap:.3e}")
            assert left > 0 and gap <= ADJ_F64_BOUND


@pytest.mark.parametrize("dims,kern,tag", ALL, ids=ALL_IDS)
def test_one_hot_coefficients_give_exactly_the_masks_rows(dims, kern, tag):
    """C = I over 67 observations: the non-zero entries of row n are the window of observation n, exactly
    (the point exactly rho from a node keeps it, its neighbour one ulp farther loses it), and the
    values are those the matvec sees: the same row from one-hot weights on a few mesh points."""
    from hipgp_amd import kuf
    c = _case(dims, kern, tag)
    nobs = 67
    plan = _plan(c, nobs)
    out = kuf.kuf_grid_rmatvec_win(plan, torch.eye(nobs, dtype=c["dtype"], device=DEV))
    assert torch.equal(out != 0, c["mask"][:nobs])
    assert bool((out >= 0).all())
    cols = torch.unique(torch.nonzero(c["mask"][:nobs])[:, 1])[:: max(1, c["M"] // 40)][:9]
    W = torch.zeros(len(cols), c["M"], dtype=c["dtype"], device=DEV)
    W[torch.arange(len(cols)), cols] = 1
    assert torch.equal(kuf.kuf_grid_matvec_win(plan, W), out[:, cols]), "the two products differ in an element value"


def _raw(entry, plan, A, out_ptr):
    """The C entry on the plan's arguments with the given output address."""
    from hipgp_amd import _lib, kuf
    x = plan.x
    m, ptrs = kuf._grid_ptrs(plan.grids)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    head = (_lib.dtype_code(x.dtype), plan.kind, len(plan.grids), m, ptrs, vp(x), x.shape[0], plan.sig2, plan.ell,
            plan.rho, vp(A), A.shape[0])
    if entry == "matvec":
        return _lib.lib().hgp_kuf_grid_matvec_win(*head, ctypes.c_void_p(out_ptr), _lib.stream_ptr(x.device))
    order, start = plan.bins()
    return _lib.lib().hgp_kuf_grid_rmatvec_win(*head, vp(order), vp(start), ctypes.c_void_p(out_ptr),
                                               _lib.stream_ptr(x.device))


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("dims", list(GRIDS), ids=did)
def test_guard_rows_around_out_are_untouched(dims, tag):
    from hipgp_amd import kuf
    c = _case(dims, KERNELS[0], tag)
    nobs = 67
    plan = _plan(c, nobs)
    for nw in NWS:
        W, C = c["W"][:nw].contiguous(), c["C"][:nw, :nobs].contiguous()
        buf = torch.full((nobs + 2, nw), float("nan"), dtype=c["dtype"], device=DEV)
        assert _raw("matvec", plan, W, buf[1].data_ptr()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())
        assert torch.equal(buf[1:-1], kuf.kuf_grid_matvec_win(plan, W))
        buf = torch.full((nw + 2, c["M"]), float("nan"), dtype=c["dtype"], device=DEV)
        assert _raw("rmatvec", plan, C, buf[1].data_ptr()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())
        assert torch.equal(buf[1:-1], kuf.kuf_grid_rmatvec_win(plan, C))


def test_empty_products_declines_and_plan_reuse():
    from hipgp_amd import kuf
    c = _case((70, 90), KERNELS[0], "f32")
    M = c["M"]
    plan0 = _plan(c, 0)
    assert tuple(kuf.kuf_grid_matvec_win(plan0, c["W"][:2]).shape) == (0, 2)
    empty = kuf.kuf_grid_rmatvec_win(plan0, c["C"][:2, :0])                    # an empty sum is zero
    assert tuple(empty.shape) == (2, M) and bool((empty == 0).all())
    plan = _plan(c, 67)
    assert tuple(kuf.kuf_grid_matvec_win(plan, c["W"][:0]).shape) == (67, 0)
    assert tuple(kuf.kuf_grid_rmatvec_win(plan, c["C"][:0, :67]).shape) == (0, M)
    assert tuple(kuf.kuf_grid_matvec_win(plan, c["W"][0]).shape) == (67, 1)    # an (M,) vector is one row
    assert tuple(kuf.kuf_grid_rmatvec_win(plan, c["C"][0, :67]).shape) == (1, M)
    with pytest.raises(ValueError):
        kuf.kuf_grid_matvec_win(plan, c["W"][:2, :-1])
    with pytest.raises(ValueError):
        kuf.kuf_grid_rmatvec_win(plan, c["C"][:2, :66])
    w = c["W"][:1].clone().requires_grad_(True)
    assert kuf.kuf_grid_matvec_win(plan, w) is None
    # what WindowPlan.make declines: Gneiting, a vector ell, a graph to ell, a tolerance outside (0, 1)
    import ziggy.kernels as zk
    x, grids = c["x"][:67], c["grids"]
    assert kuf.WindowPlan.make(zk.Gneiting(dtype=torch.float32), grids, x, c["params"], TOL) is None
    assert kuf.WindowPlan.make(c["k"], grids, x, (1.0, torch.tensor([.2, .3], device=DEV)), TOL) is None
    assert kuf.WindowPlan.make(c["k"], grids, x, (1.0, torch.tensor(0.3, device=DEV, requires_grad=True)), TOL) is None
    assert kuf.WindowPlan.make(c["k"], grids, x, c["params"], 0.0) is None
    assert kuf.WindowPlan.make(c["k"], grids, x, c["params"], 1.0) is None
    assert kuf.WindowPlan.make(c["k"], grids, x, c["params"], TOL) is not None
    # one plan for three C: the bits of three fresh plans
    for i in range(3):
        C = (c["C"][:3, :67] * (i + 1)).contiguous()
        assert torch.equal(kuf.kuf_grid_rmatvec_win(plan, C), kuf.kuf_grid_rmatvec_win(_plan(c, 67), C))


# ---- the model: 64 x 64 grid, SqExp ell = 0.05, fp64, 300 observations --------------------------------
MODEL_TOLS = (1e-4, 1e-12)


@functools.lru_cache(maxsize=None)
def _model_case():
    import ziggy.hipgp as hg
    import ziggy.kernels as zk
    dt = torch.float64
    grids = [torch.linspace(-1, 1, 64, dtype=dt) for _ in range(2)]
    torch.manual_seed(5)
    mod = hg.MeanFieldToeplitzGP(zk.SqExp(dtype=dt), grids, num_obs=300, sig2_init=1., ell_init=.05, noise2_init=.05,
                                 learn_kernel=False, dtype=dt)
    g = torch.Generator(device="cpu").manual_seed(11)
    with torch.no_grad():
        mod.global_theta2.copy_(-(torch.rand(mod.Mprime, 1, generator=g, dtype=dt) * 4 + .5))
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=dt))
    mod = mod.cuda_params(0)
    x = (torch.rand(300, 2, generator=g, dtype=dt) * 2.2 - 1.1).to(DEV)
    sd = (torch.rand(300, 1, generator=g, dtype=dt) * .4 + .1).to(DEV)
    y = torch.sin(3 * x[:, :1]) * torch.cos(2 * x[:, 1:2]) + sd * torch.randn(300, 1, generator=g, dtype=dt).to(DEV)
    return mod, x, y, sd


@pytest.mark.parametrize("t", MODEL_TOLS, ids=lambda t: f"{t:.0e}")
def test_predict_mean_with_a_support_tolerance_is_within_the_stated_bound(t):
    from hipgp_amd import kuf
    mod, x, _, _ = _model_case()
    alpha = mod.mean_weights()
    sig2 = float(mod.get_kernel_params()[0])
    try:
        mod.kuf_support_tol = t
        mu_t = mod.predict_mean(x, weights=alpha)
    finally:
        mod.kuf_support_tol = None
    mu = mod.predict_mean(x, weights=alpha)
    limit = t * sig2 * float(alpha.abs().sum())
    gap = float((mu_t - mu).abs().max())
    rho = kuf.support_radius(mod.kernel, mod.get_kernel_params(), t)
    print(f"predict_mean support_tol={t:.0e}: rho = {rho:.4f} ({rho * 63 / 2:.1f} steps), max gap {gap:.3e}, "
          f"limit t sig2 sum|alpha| = {limit:.3e}, max|mu| = {float(mu.abs().max()):.3e}")
    assert tuple(mu_t.shape) == (300, 1) and mu_t.device.type == "cpu"
    assert gap <= limit
    if t == 1e-4:
        assert gap > 0, "the windowed product was not taken"
    # the knob unset: the dense fused product, bit for bit
    dense = kuf.kuf_grid_matvec(mod.kernel, mod.xgrids, x, mod.get_kernel_params(), alpha)
    assert torch.equal(mu, dense.reshape(-1, 1).cpu())
    with pytest.raises(NotImplementedError, match="tube"):
        try:
            mod.kuf_support_tol = t
            mod.predict_mean(x, weights=alpha, integrated_obs=True)
        finally:
            mod.kuf_support_tol = None
    # predict_samples takes the tolerance as an argument and windows its Kuf product alone
    kw = dict(nfeat=64, generator=None, eps=torch.zeros(2, mod.Mprime, dtype=torch.float64),
              features=(torch.ones(64, 2, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)),
              prior_w=torch.zeros(2, 64, dtype=torch.float64), nugget_eps=torch.zeros(2, mod.M, dtype=torch.float64))
    calls = []
    real = kuf.kuf_grid_matvec_win
    try:
        kuf.kuf_grid_matvec_win = lambda plan, W: calls.append(plan.tol) or real(plan, W)
        s0 = mod.predict_samples(x, 2, **kw)
        assert calls == []
        st = mod.predict_samples(x, 2, support_tol=t, **kw)
        assert calls == [t]
    finally:
        kuf.kuf_grid_matvec_win = real
    print(f"predict_samples support_tol={t:.0e}: max gap to the dense draws {float((st - s0).abs().max()):.3e}")
    assert tuple(st.shape) == tuple(s0.shape) == (2, 300)
    with pytest.raises(NotImplementedError):
        mod.predict_samples(x, 2, support_tol=t, integrated_obs=True, **kw)


@functools.lru_cache(maxsize=None)
def _dense_system():
    """The dense fp64 operator pieces of the model case: K from the model's own K operator applied to the
    identity in pieces, Kuf by the torch kernel, iv, y."""
    mod, x, y, sd = _model_case()
    with torch.no_grad():
        T = mod.toeplitz()
        M = mod.M
        eye = torch.eye(M, dtype=torch.float64, device=DEV)
        T.set_batch_shape((256,))
        K = torch.cat([T._matmul_by_K(eye[a:a + 256].contiguous()).reshape(256, M) for a in range(0, M, 256)], dim=0)
        Kuf = mod.kernel.forward(x, mod.xinduce.to(DEV), params=mod.get_kernel_params())
        iv = (1 / sd ** 2).reshape(-1)
    return K, Kuf, iv, y.reshape(-1)


@functools.lru_cache(maxsize=None)
def _dense_fit():
    """`fit_mean` of the model case with every knob unset: computed once, shared, never changed."""
    mod, x, y, sd = _model_case()
    assert mod.kuf_support_tol is None
    return mod.fit_mean(x, y, noise_std=sd, tol=1e-10, maxiter=4000, update=False)


@pytest.mark.parametrize("t", MODEL_TOLS, ids=lambda t: f"{t:.0e}")
def test_fit_mean_with_a_support_tolerance_solves_the_dense_system_to_the_derived_bound(t):
    """beta of the windowed fit in the DENSE system: b - A beta = (b_w - A_w beta) + (b - b_w) - (A - A_w) beta, so
    |b - A beta| <= tol_cg |b| + |dA| |beta| + |db| with dA, db formed here from the dense and the masked Kuf
    (|dA| the spectral norm).  Also printed, not asserted: how far the windowed fit's mean lies from the dense
    fit's (it scales with the condition number)."""
    from hipgp_amd import kuf
    mod, x, y, sd = _model_case()
    K, Kuf, iv, yv = _dense_system()
    tol_cg = 1e-10
    rho = kuf.support_radius(mod.kernel, mod.get_kernel_params(), t)
    KufM = Kuf * _mask(x, [g.to(DEV) for g in mod.xgrids], rho)
    A = K + Kuf.t() @ (iv[:, None] * Kuf)
    b = Kuf.t() @ (iv * yv)
    E = Kuf - KufM                                       # exact: the dropped entries
    dA = E.t() @ (iv[:, None] * Kuf) + KufM.t() @ (iv[:, None] * E)      # = Kuf^T D Kuf - KufM^T D KufM, nothing cancels
    db = E.t() @ (iv * yv)
    dense_fit = _dense_fit()
    try:
        mod.kuf_support_tol = t
        fit = mod.fit_mean(x, y, noise_std=sd, tol=tol_cg, maxiter=4000, update=False)
    finally:
        mod.kuf_support_tol = None
    beta = fit.weights.reshape(-1)
    res = float(torch.linalg.vector_norm(b - A @ beta))
    nb, nbeta = float(torch.linalg.vector_norm(b)), float(torch.linalg.vector_norm(beta))
    # |dA| (spectral) without an M x M decomposition: the range of the symmetric dA lies in the span of the
    # rows of [Kuf; KufM], so with Q an orthonormal basis of it (M x 600) |dA| = |Q^T dA Q|, a 600 x 600
    # symmetric eigenproblem; 30 steps of the power method on dA itself give a lower estimate that the
    # figure must not fall under
    Q, _ = torch.linalg.qr(torch.cat([Kuf, KufM], dim=0).t())
    Bq = Q.t() @ dA @ Q
    ndA = float(torch.linalg.eigvalsh(.5 * (Bq + Bq.t())).abs().max())
    v = torch.ones(dA.shape[0], dtype=dA.dtype, device=DEV)
    for _ in range(30):
        v = dA @ v
        v = v / torch.linalg.vector_norm(v)
    assert ndA >= 0.999 * float(torch.linalg.vector_norm(dA @ v)), "the 600 x 600 eigenvalues miss |dA|"
    ndb = float(torch.linalg.vector_norm(db))
    limit = tol_cg * nb + ndA * nbeta + ndb
    away = float((fit.qm - dense_fit.qm).abs().max() / dense_fit.qm.abs().max())
    print(f"fit_mean support_tol={t:.0e}: {fit.iters} iterations (dense {dense_fit.iters}), relres {fit.relres:.2e}; "
          f"|b - A beta| = {res:.3e}, limit {limit:.3e} = tol|b| {tol_cg * nb:.3e} + |dA||beta| {ndA * nbeta:.3e} + "
          f"|db| {ndb:.3e}; windowed mean vs dense mean: max gap / max|qm| = {away:.3e}")
    assert fit.relres < tol_cg and fit.iters < 4000
    assert res <= limit
    assert not torch.equal(fit.weights, dense_fit.weights), "the windowed products were not taken"
    if t == MODEL_TOLS[0]:      # the knobs unset again: the dense fit's bits
        back = mod.fit_mean(x, y, noise_std=sd, tol=tol_cg, maxiter=4000, update=False)
        assert torch.equal(back.weights, dense_fit.weights) and torch.equal(back.qm, dense_fit.qm)
        assert back.iters == dense_fit.iters
    with pytest.raises(NotImplementedError, match="tube"):
        try:
            mod.kuf_support_tol = t
            mod.fit_mean(x, y, noise_std=sd, integrated_obs=True, update=False)
        finally:
            mod.kuf_support_tol = None
