"""SqExp with one length scale per axis on the device (the hgp_kuf_grid*_ard entries behind `kuf.kuf_grid`,
`kuf_grid_matvec` / `kuf_grid_rmatvec`, `WindowPlan` / `kuf_grid_matvec_win` / `kuf_grid_rmatvec_win` and
`kuf_grid_ad`, and the model on top of them) against the fp64 torch expression of `kernels.py:73-79` with
the vector ell, K64 = sig2 exp(-sum_a ((x_a - u_a) / ell_a)^2 / 2).

Shapes: the smallest that cross the kernels' seams (64 points a wave and runs of 256 in the dense products,
tiles of 256 mesh points and 256 staged observations in the gather, lanes across the last axis in the
forward window): grids 70, 37 x 70, 5 x 9 x 70 on [-1, 1], 1 / 65 / 300 points in [-1.2, 1.2], 1 and 3 rows.

Every error of a product is measured relative to S = sum |K64| |w| of the fp64 reference, the largest over the
outputs of a weight / coefficient row as tests/test_kuf_win_gpu.py takes it (so an output that underflows
does not set the scale).
  fp64: |error| <= 1e-10 S.
  fp32: |error| <= (4 e32 + 1e-7) S, e32 the worst |error| / S of torch's own fp32 evaluation of the same
        quantity over the case's 300 points (one figure per case).
The windowed products are checked against the fp64 product masked with the per-axis predicate formed here,
|x_a - g_a[j_a]| <= rho[a] in x's dtype, and against the unmasked product to t sig2 sum |w| more.
The scalar-replication check compares bits; the hgp_kuf_grid_grad_ard sums with equal ell have the scalar
entry's sig2 sum bit for bit and per-axis sums that add up to its ell sum to the backward's bound (the
scalar entry forms K s / ell, the new one K q_a / ell_a per axis).
Each test prints its figures before it asserts."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIG2 = 1.3
# per-axis length scales with clearly different windows: at t = 1e-3 about 4 nodes of 37 against 13 of 70
CASES = {(70,): (0.04,), (37, 70): (0.03, 0.05), (5, 9, 70): (0.2, 0.08, 0.04)}
DIMS = list(CASES)
NOBS = (1, 65, 300)
NROWS = (1, 3)
TOLS = (2.0 ** -24, 1e-3)
F64_BOUND = 1e-10
F32_FLOOR = 1e-7
ADJ_F64_BOUND = 1e-12          # tests/test_kuf_win_gpu.py
GUARD = 3
did = lambda d: "x".join(map(str, d))
ALL = [(d, t) for d in DIMS for t in ("f64", "f32")]
ALL_IDS = [f"{did(d)}-{t}" for d, t in ALL]


def _sqexp(dtype):
    import ziggy.kernels as zk
    return zk.SqExp(dtype=dtype, ard=True)     # declared per-axis: a plain SqExp declines a vector ell


def _mesh(grids):
    return torch.stack([g.reshape(-1) for g in torch.meshgrid(*grids, indexing="ij")], dim=-1)


def _expr(x, grids, ell, dtype):
    """kernels.py:73-79 with a vector ell, in `dtype`: sig2 exp(-sum_a ((x_a - u_a) / ell_a)^2 / 2)"""
    e = torch.tensor(ell, dtype=dtype, device=x.device)
    u = _mesh([g.to(dtype) for g in grids])
    d = (x.to(dtype)[:, None, :] - u[None, :, :]) / e
    return torch.tensor(SIG2, dtype=dtype, device=x.device) * torch.exp(-torch.sum(d * d, dim=-1) / 2)


def _mask(x, grids, rho):
    """the window's predicate per axis, in x's dtype with each rho[a] rounded once to it"""
    nobs = x.shape[0]
    m = torch.ones((nobs,) + tuple(g.numel() for g in grids), dtype=torch.bool, device=x.device)
    for a, g in enumerate(grids):
        ok = (x[:, a, None] - g[None, :]).abs() <= torch.tensor(rho[a], dtype=x.dtype, device=x.device)
        m = m & ok.reshape((nobs,) + tuple(g.numel() if b == a else 1 for b in range(len(grids))))
    return m.reshape(nobs, -1)


def _weights(n, M, dtype, positive=False):
    g = torch.Generator(device="cpu").manual_seed(11 + M)
    mag = torch.rand(n, M, generator=g, dtype=dtype) + 0.5
    if positive:
        return mag.to(DEV)
    sign = (torch.randint(0, 2, (n, M), generator=g, dtype=torch.int64) * 2 - 1).to(dtype)
    return (sign * mag).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(dims, tag):
    """Inputs in the test dtype, the fp64 matrix on those same values and (fp32) torch's own fp32 matrix;
    computed once and shared, never changed."""
    from hipgp_amd import kuf
    dtype = torch.float64 if tag == "f64" else torch.float32
    ell = list(CASES[dims])
    k = _sqexp(dtype)
    grids = [torch.linspace(-1, 1, m, dtype=dtype).to(DEV) for m in dims]
    g = torch.Generator(device="cpu").manual_seed(5)
    x = (torch.rand(max(NOBS), len(dims), generator=g, dtype=torch.float64) * 2.4 - 1.2).to(dtype)
    x[3] = torch.stack([gr.cpu()[gr.numel() // 3] for gr in grids])            # one point on a node: r = 0
    x = x.to(DEV)
    K64 = _expr(x, grids, ell, torch.float64)
    K32 = _expr(x, grids, ell, torch.float32) if tag == "f32" else None
    M = int(np.prod(dims))
    c = dict(dims=dims, tag=tag, dtype=dtype, k=k, ell=ell, params=(SIG2, ell), grids=grids, x=x, K64=K64, K32=K32,
             M=M, W=_weights(max(NROWS), M, dtype), C=_weights(max(NROWS), max(NOBS), dtype), win={})
    for t in TOLS:
        rho = kuf.support_radius(k, c["params"], t)
        mask = _mask(x, grids, rho)
        c["win"][t] = dict(rho=rho, mask=mask, KM=K64 * mask, K32m=None if K32 is None else K32 * mask)
    return c


def _bound(c, ref_fn, K, K32, axis, nobs=None):
    """(ref, S, relative bound, e32): ref_fn(K) the fp64 product (axis 0: its first nobs rows), S the matching
    sum |K64| |w|, its largest along `axis` (the outputs of one weight / coefficient row), the fp32 figure
    from torch's fp32 product over all of the case's points."""
    cut = (lambda v: v[:nobs]) if axis == 0 and nobs is not None else (lambda v: v)
    ref_all, S_all = ref_fn(K.double()), ref_fn(c["K64"].abs(), absw=True)
    ref, S = cut(ref_all), cut(S_all).amax(dim=axis, keepdim=True)
    if c["tag"] == "f64":
        return ref, S, F64_BOUND, None
    t32 = ref_fn(K32, f32=True).double()
    e32 = float(((t32 - ref_all).abs() / S_all.amax(dim=axis, keepdim=True)).max())
    return ref, S, 4 * e32 + F32_FLOOR, e32


def _mv_ref(c, nw):
    W = c["W"][:nw]

    def f(K, absw=False, f32=False):
        Wd = W if f32 else W.double()
        return K @ (Wd.abs() if absw else Wd).t()
    return f


def _rmv_ref(c, nc, nobs):
    C = c["C"][:nc, :nobs]

    def f(K, absw=False, f32=False):
        Cd = C if f32 else C.double()
        return (Cd.abs() if absw else Cd) @ K[:nobs]
    return f


def _assert_close(what, out, ref, S, bound, e32=None):
    err = (out.double() - ref).abs()
    worst = float((err / S).max())
    print(f"{what}: worst |error| / S = {worst:.3e}, bound {bound:.3e}" + ("" if e32 is None else f" (torch fp32 {e32:.3e})"))
    assert bool(torch.isfinite(out).all())
    assert bool((err <= bound * S).all()), (what, worst, bound)


# ---- 5. the inputs: the mask keeps between 1 % and 60 % of the pairs ----------------------------------
@pytest.mark.parametrize("dims,tag", ALL, ids=ALL_IDS)
def test_the_windows_are_neither_trivial_nor_everything(dims, tag):
    c = _case(dims, tag)
    for t in TOLS:
        w = c["win"][t]
        share = float(w["mask"].double().mean())
        per_point = w["mask"].sum(dim=1)
        width = [2 * r / (2.0 / (m - 1)) for r, m in zip(w["rho"], dims)]
        print(f"{did(dims)} {tag} t={t:.2e}: rho = {w['rho']}, window widths in nodes {width}, "
              f"mask share {share:.4f}, empty windows {int((per_point == 0).sum())}, largest {int(per_point.max())}")
        assert 0.01 <= share <= 0.60
        assert len(set(round(v, 1) for v in width)) == len(dims), "the axes' windows differ in width"


# ---- 1. kuf_grid ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,tag", ALL, ids=ALL_IDS)
def test_kuf_grid_vs_the_expression(dims, tag):
    """Element by element against S = the largest element of K64 (a one-hot w: sum |K64| |w| is the element)."""
    from hipgp_amd import kuf
    c = _case(dims, tag)
    for nobs in NOBS:
        K = kuf.kuf_grid(c["k"], c["grids"], c["x"][:nobs], c["params"])
        assert K is not None and tuple(K.shape) == (nobs, c["M"]) and K.dtype == c["dtype"]
        S = c["K64"][:nobs].amax().reshape(1, 1)
        if tag == "f64":
            bound, e32 = F64_BOUND, None
        else:
            e32 = float((c["K32"].double() - c["K64"]).abs().max() / c["K64"].amax())
            bound = 4 * e32 + F32_FLOOR
        _assert_close(f"kuf_grid {did(dims)} {tag} nobs={nobs}", K, c["K64"][:nobs], S, bound, e32)
        assert torch.equal(K, kuf.kuf_grid(c["k"], c["grids"], c["x"][:nobs], c["params"]))
        # ell as a tensor is read as its values
        ell_t = torch.tensor(c["ell"], dtype=c["dtype"], device=DEV)
        assert torch.equal(K, kuf.kuf_grid(c["k"], c["grids"], c["x"][:nobs], (SIG2, ell_t)))


# ---- 2. the dense products ------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,tag", ALL, ids=ALL_IDS)
def test_dense_products_vs_the_expression(dims, tag):
    from hipgp_amd import kuf
    c = _case(dims, tag)
    for nr in NROWS:
        for nobs in NOBS:
            ref, S, bound, e32 = _bound(c, _mv_ref(c, nr), c["K64"], c["K32"], 0, nobs)
            for nsplit in (0, 3):
                out = kuf.kuf_grid_matvec(c["k"], c["grids"], c["x"][:nobs], c["params"], c["W"][:nr], nsplit=nsplit)
                _assert_close(f"matvec {did(dims)} {tag} nobs={nobs} nw={nr} nsplit={nsplit}", out, ref, S, bound, e32)
        for nobs in NOBS:
            ref, S, bound, e32 = _bound(c, _rmv_ref(c, nr, nobs), c["K64"], c["K32"], 1)
            for nsplit in (0, 2):
                out = kuf.kuf_grid_rmatvec(c["k"], c["grids"], c["x"][:nobs], c["params"], c["C"][:nr, :nobs],
                                           nsplit=nsplit)
                _assert_close(f"rmatvec {did(dims)} {tag} nobs={nobs} nc={nr} nsplit={nsplit}", out, ref, S, bound, e32)


# ---- 3. / 4. the windowed pair ----------------------------------------------------------------------------
def _plan(c, nobs, t, **kw):
    from hipgp_amd import kuf
    return kuf.WindowPlan(c["k"], c["grids"], c["x"][:nobs], c["params"], t, **kw)


@pytest.mark.parametrize("dims,tag", ALL, ids=ALL_IDS)
def test_windowed_products_vs_the_masked_and_the_dense_product(dims, tag):
    from hipgp_amd import kuf
    c = _case(dims, tag)
    for t in TOLS:
        w = c["win"][t]
        for nobs in NOBS:
            plan = _plan(c, nobs, t)
            assert plan.rho == w["rho"] and plan.ell == c["ell"]
            for nr in NROWS:
                ref, S, bound, e32 = _bound(c, _mv_ref(c, nr), w["KM"], w["K32m"], 0, nobs)
                out = kuf.kuf_grid_matvec_win(plan, c["W"][:nr])
                _assert_close(f"matvec_win {did(dims)} {tag} t={t:.1e} nobs={nobs} nw={nr}", out, ref, S, bound, e32)
                dense = _mv_ref(c, nr)(c["K64"])[:nobs]
                trunc = t * SIG2 * c["W"][:nr].double().abs().sum(dim=1)[None, :]
                gap = (out.double() - dense).abs()
                print(f"  truncation: worst |windowed - dense| = {float(gap.max()):.3e}, bound t sig2 sum|w| = "
                      f"{float(trunc.min()):.3e}")
                assert bool((gap <= trunc + bound * S).all())
                ref, S, bound, e32 = _bound(c, _rmv_ref(c, nr, nobs), w["KM"], w["K32m"], 1)
                out = kuf.kuf_grid_rmatvec_win(plan, c["C"][:nr, :nobs])
                _assert_close(f"rmatvec_win {did(dims)} {tag} t={t:.1e} nobs={nobs} nc={nr}", out, ref, S, bound, e32)
                dense = _rmv_ref(c, nr, nobs)(c["K64"])
                trunc = t * SIG2 * c["C"][:nr, :nobs].double().abs().sum(dim=1)[:, None]
                assert bool(((out.double() - dense).abs() <= trunc + bound * S).all())


# ---- 6. one-hot rows, transposes ---------------------------------------------------------------------------
@pytest.mark.parametrize("dims,tag", ALL, ids=ALL_IDS)
def test_one_hot_rows_give_the_masked_rows_of_kuf_grid(dims, tag):
    from hipgp_amd import kuf
    c = _case(dims, tag)
    t = TOLS[0]
    nobs = 65
    plan = _plan(c, nobs, t)
    K = kuf.kuf_grid(c["k"], c["grids"], c["x"][:nobs], c["params"])
    zero = torch.zeros((), dtype=c["dtype"], device=DEV)
    seen = 0
    for n0 in range(0, nobs, 3):
        rows = list(range(n0, min(n0 + 3, nobs)))
        C = torch.zeros(len(rows), nobs, dtype=c["dtype"], device=DEV)
        for s, n in enumerate(rows):
            C[s, n] = 1
        out = kuf.kuf_grid_rmatvec_win(plan, C)
        want = torch.where(c["win"][t]["mask"][rows], K[rows], zero)
        assert torch.equal(out, want), (dims, tag, rows)
        seen += int((want != 0).sum())
    assert seen > 0


@pytest.mark.parametrize("dims", DIMS, ids=did)
def test_the_two_windowed_products_are_transposes_fp64(dims):
    from hipgp_amd import kuf
    c = _case(dims, "f64")
    for t in TOLS:
        for nobs in NOBS:
            plan = _plan(c, nobs, t)
            w = _weights(1, c["M"], torch.float64, positive=True)
            cc = _weights(1, nobs, torch.float64, positive=True)
            left = float(torch.sum(kuf.kuf_grid_matvec_win(plan, w)[:, 0] * cc[0]))
            right = float(torch.sum(kuf.kuf_grid_rmatvec_win(plan, cc)[0] * w[0]))
            gap = abs(left - right) / abs(left) if left != 0 else abs(right)
            print(f"transpose {did(dims)} t={t:.1e} nobs={nobs}: <c, Kw> = {left:.15e}, relative gap {gap:.3e}")
            assert gap <= ADJ_F64_BOUND
            assert left > 0 or not bool(c["win"][t]["mask"][:nobs].any())


# ---- 7. equal ell on every axis: the scalar entries' bits -------------------------------------------------
@pytest.mark.parametrize("dims,tag", ALL, ids=ALL_IDS)
def test_replicated_ell_gives_the_scalar_entries_bits(dims, tag):
    from hipgp_amd import kuf
    c = _case(dims, tag)
    k, grids, d = c["k"], c["grids"], len(dims)
    e, t = 0.05, TOLS[0]
    sc, rep = (SIG2, e), (SIG2, [e] * d)
    rho = kuf.support_radius(k, sc, t)
    assert kuf.support_radius(k, rep, t) == [rho] * d
    for nobs in NOBS:
        x = c["x"][:nobs]
        assert torch.equal(kuf.kuf_grid(k, grids, x, sc), kuf.kuf_grid(k, grids, x, rep))
        ps, pr = kuf.WindowPlan(k, grids, x, sc, t), kuf.WindowPlan(k, grids, x, rep, t)
        assert isinstance(ps.ell, float) and isinstance(pr.ell, list)
        for nr in NROWS:
            W, C = c["W"][:nr], c["C"][:nr, :nobs]
            for ns in (0, 3):
                assert torch.equal(kuf.kuf_grid_matvec(k, grids, x, sc, W, nsplit=ns),
                                   kuf.kuf_grid_matvec(k, grids, x, rep, W, nsplit=ns))
                assert torch.equal(kuf.kuf_grid_rmatvec(k, grids, x, sc, C, nsplit=ns),
                                   kuf.kuf_grid_rmatvec(k, grids, x, rep, C, nsplit=ns))
            assert torch.equal(kuf.kuf_grid_matvec_win(ps, W), kuf.kuf_grid_matvec_win(pr, W))
            assert torch.equal(kuf.kuf_grid_rmatvec_win(ps, C), kuf.kuf_grid_rmatvec_win(pr, C))
        # the backward: the sig2 sum bit for bit; the per-axis sums add up to the scalar entry's ell sum
        G = _weights(nobs, c["M"], c["dtype"])
        g2 = _raw_grad(c, x, e, G, ard=False)
        ga = _raw_grad(c, x, [e] * d, G, ard=True)
        K64 = _expr(x, grids, [e] * d, torch.float64)
        u = _mesh([gr.double() for gr in grids])
        s = (((x.double()[:, None, :] - u[None]) / e) ** 2).sum(-1)
        S = float((G.double().abs() * K64 * s / e).sum())
        gap = abs(float(ga[1:].double().sum()) - float(g2[1])) / S
        print(f"grad {did(dims)} {tag} nobs={nobs}: scalar {g2.tolist()}, per axis {ga.tolist()}, |sum - scalar| / S = {gap:.3e}")
        assert torch.equal(ga[0], g2[0])
        assert gap <= (F64_BOUND if tag == "f64" else 1e-5)


def _raw_grad(c, x, ell, G, ard):
    from hipgp_amd import _lib, kuf
    m, ptrs = kuf._grid_ptrs(c["grids"])
    xc = x.contiguous()
    args = (_lib.KERN_SQEXP, len(c["grids"]), m, ptrs, ctypes.c_void_p(xc.data_ptr()), xc.shape[0], SIG2)
    if ard:
        return kuf._grad_call(_lib.lib().hgp_kuf_grid_grad_ard, xc, G.contiguous(), *args, kuf._dvec(ell),
                              nsum=1 + len(ell))
    return kuf._grad_call(_lib.lib().hgp_kuf_grid_grad, xc, G.contiguous(), *args, ell)


# ---- 8. guard rows, reruns ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,tag", ALL, ids=ALL_IDS)
def test_guard_rows_stay_untouched_and_reruns_repeat_the_bits(dims, tag):
    from hipgp_amd import _lib, kuf
    c = _case(dims, tag)
    L, dt, M, d = _lib.lib(), c["dtype"], c["M"], len(dims)
    t = TOLS[1]
    code, st = _lib.dtype_code(dt), _lib.stream_ptr(torch.device(DEV))
    m, ptrs = kuf._grid_ptrs(c["grids"])
    ell, rho = kuf._dvec(c["ell"]), kuf._dvec(c["win"][t]["rho"])
    vp = lambda tns: ctypes.c_void_p(tns.data_ptr())
    for nobs in (65, 300):
        x = c["x"][:nobs].contiguous()
        plan = _plan(c, nobs, t)
        order, start = plan.bins()
        W, C = c["W"].contiguous(), c["C"][:, :nobs].contiguous()
        G = _weights(nobs, M, dt)
        nr = W.shape[0]
        head = (code, _lib.KERN_SQEXP, d, m, ptrs, vp(x), nobs, SIG2, ell)
        calls = {
            "grid": ((nobs, M), lambda o: L.hgp_kuf_grid_ard(*head, vp(o), st),
                     lambda: kuf.kuf_grid(c["k"], c["grids"], x, c["params"])),
            "matvec": ((nobs, nr), lambda o: L.hgp_kuf_grid_matvec_ard(*head, vp(W), nr, 3, vp(o), st),
                       lambda: kuf.kuf_grid_matvec(c["k"], c["grids"], x, c["params"], W, nsplit=3)),
            "rmatvec": ((nr, M), lambda o: L.hgp_kuf_grid_rmatvec_ard(*head, vp(C), nr, 2, vp(o), st),
                        lambda: kuf.kuf_grid_rmatvec(c["k"], c["grids"], x, c["params"], C, nsplit=2)),
            "matvec_win": ((nobs, nr), lambda o: L.hgp_kuf_grid_matvec_win_ard(*head, rho, vp(W), nr, vp(o), st),
                           lambda: kuf.kuf_grid_matvec_win(plan, W)),
            "rmatvec_win": ((nr, M), lambda o: L.hgp_kuf_grid_rmatvec_win_ard(*head, rho, vp(C), nr, vp(order),
                                                                              vp(start), vp(o), st),
                            lambda: kuf.kuf_grid_rmatvec_win(plan, C)),
            "grad": ((1, 1 + d), lambda o: L.hgp_kuf_grid_grad_ard(*head, vp(G), vp(o), st),
                     lambda: _raw_grad(c, x, c["ell"], G, ard=True).reshape(1, -1)),
        }
        for name, (shape, raw, wrapped) in calls.items():
            buf = torch.full((shape[0] + 2 * GUARD, shape[1]), float("nan"), dtype=dt, device=DEV)
            _lib.check(raw(buf[GUARD:]))
            torch.cuda.synchronize()
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), (name, "guard rows")
            assert bool(torch.isfinite(buf[GUARD:-GUARD]).all()), name
            assert torch.equal(buf[GUARD:-GUARD], wrapped()), (name, "a rerun differs")


# ---- 9. the backward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,tag", ALL, ids=ALL_IDS)
def test_backward_vs_autograd_of_the_expression(dims, tag):
    """The 1 + D sums for a random G against fp64 torch autograd, under the bound rule of
    tests/test_kuf_grad_gpu.py: relative to S = sum |G o dK/dtheta|; fp64 1e-10, fp32 4 x torch's own fp32
    autograd plus 1e-5 S."""
    from hipgp_amd import kuf
    c = _case(dims, tag)
    d = len(dims)
    for nobs in (65, 300):
        x = c["x"][:nobs]
        G = _weights(nobs, c["M"], c["dtype"])

        def auto(dtype):
            s2 = torch.tensor(SIG2, dtype=dtype, device=DEV, requires_grad=True)
            el = torch.tensor(c["ell"], dtype=dtype, device=DEV, requires_grad=True)
            u = _mesh([g.to(dtype) for g in c["grids"]])
            dv = (x.to(dtype)[:, None, :] - u[None, :, :]) / el
            K = s2 * torch.exp(-torch.sum(dv * dv, dim=-1) / 2)
            (K * G.to(dtype)).sum().backward()
            absK = (K.detach() * G.to(dtype).abs()).double()
            S = torch.cat([(absK / SIG2).sum()[None], (absK[:, :, None] * (dv.detach().double() ** 2)).sum((0, 1))
                           / torch.tensor(c["ell"], dtype=torch.float64, device=DEV)])
            return torch.cat([s2.grad[None], el.grad]).double(), S
        ref, S = auto(torch.float64)
        s2 = torch.tensor(SIG2, dtype=c["dtype"], device=DEV, requires_grad=True)
        el = torch.tensor(c["ell"], dtype=c["dtype"], device=DEV, requires_grad=True)
        K = kuf.kuf_grid_ad(c["k"], c["grids"], x, (s2, el))
        assert K is not None and type(K.grad_fn).__name__ == "_KufADBackward"
        assert torch.equal(K.detach(), kuf.kuf_grid(c["k"], c["grids"], x, c["params"]))
        K.backward(G)
        assert tuple(el.grad.shape) == (d,) and s2.grad.dim() == 0
        mine = torch.cat([s2.grad[None], el.grad]).double()
        e = ((mine - ref).abs() / S).cpu().numpy()
        if tag == "f64":
            print(f"grad {did(dims)} f64 nobs={nobs}: err / S = {e}")
            assert np.all(e <= F64_BOUND), e
        else:
            e32 = ((auto(torch.float32)[0] - ref).abs() / S).cpu().numpy()
            print(f"grad {did(dims)} f32 nobs={nobs}: err / S = {e}, torch fp32 {e32}")
            assert np.all(e <= 4 * e32 + 1e-5), (e, e32)


# ---- 10. the model: 24 x 40 grid, fp64, ell = (0.3, 0.12), 50 observations ---------------------------------
MDIMS, MELL, MNOBS, MAXITER = (24, 40), (0.3, 0.12), 50, 400
MODEL_GAP_F64_MEASURED = 8.7e-9        # tests/test_kuf_matvec_gpu.py: predict_mean against predict, limit 10 x
GAP_BATCH_SOLVE_F64_MEASURED = 9.0e-9  # tests/test_fit_mean_gpu.py: fit_mean against batch_solve, limit 10 x


def _model(family, learn=False):
    import ziggy.hipgp as hg
    dt = torch.float64
    grids = [torch.linspace(-1, 1, m, dtype=dt) for m in MDIMS]
    torch.manual_seed(5)
    kw = dict(num_obs=MNOBS, sig2_init=1., ell_init=list(MELL), noise2_init=.05, learn_kernel=learn, dtype=dt)
    g = torch.Generator().manual_seed(11)
    if family == "block":
        mod = hg.BlockToeplitzGP(_sqexp(dt), grids, block_sizes=[2, 2], **kw)
        with torch.no_grad():
            A = torch.randn(mod.num_blocks, mod.block_size, mod.block_size, generator=g, dtype=dt) * .5
            mod.global_theta2.copy_(-.5 * (A.matmul(A.transpose(1, 2)) + torch.eye(mod.block_size, dtype=dt)))
    else:
        mod = hg.MeanFieldToeplitzGP(_sqexp(dt), grids, **kw)
        with torch.no_grad():
            mod.global_theta2.copy_(-(torch.rand(mod.Mprime, 1, generator=g, dtype=dt) * 4 + .5))
    with torch.no_grad():
        mod.global_theta1.copy_(torch.randn(mod.Mprime, 1, generator=g, dtype=dt))
    return mod.cuda_params(0)


def _data():
    g = torch.Generator().manual_seed(6)
    x = torch.rand(MNOBS, 2, generator=g, dtype=torch.float64) * 2.2 - 1.1
    y = torch.sin(3 * x[:, :1]) * torch.cos(5 * x[:, 1:]) + .1 * torch.randn(MNOBS, 1, generator=g, dtype=torch.float64)
    return x.to(DEV), y.to(DEV)


def _gap(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_model_prediction_routes(family):
    import copy
    from hipgp_amd import _lib
    mod = _model(family)
    x, y = _data()
    assert tuple(mod.ell.shape) == (2,)
    with torch.no_grad():
        T = mod.toeplitz()
        s, r = ctypes.c_double(0), ctypes.c_double(0)
        sep = _lib.lib().hgp_plan_is_separable(T._plan._h, ctypes.byref(s), ctypes.byref(r))
        print(f"{family}: hgp_plan_is_separable = {sep} (scale {s.value}, residual {r.value})")
        assert sep == 1
        mu_ref, sd_ref = mod.predict(x, maxiter_cg=MAXITER, fused=False, streamed=False)
        for kw in (dict(fused=True), dict(streamed=True)):
            mu_f, sd_f = mod.predict(x, maxiter_cg=MAXITER, **kw)
            assert _gap(mu_f, mu_ref) <= 10 * MODEL_GAP_F64_MEASURED and _gap(sd_f, sd_ref) <= 10 * MODEL_GAP_F64_MEASURED
        mu = mod.predict_mean(x, maxiter_cg=MAXITER)
        g = _gap(mu, mu_ref)
        print(f"{family}: predict_mean against predict: relative gap {g:.3e} (limit {10 * MODEL_GAP_F64_MEASURED:.1e})")
        assert g <= 10 * MODEL_GAP_F64_MEASURED
        # the windowed mean: within t sig2 sum |alpha| of the dense one
        alpha = mod.mean_weights(maxiter_cg=MAXITER)
        dense = mod.predict_mean(x, weights=alpha)
        mod.kuf_support_tol = 1e-6
        win = mod.predict_mean(x, weights=alpha)
        mod.kuf_support_tol = None
        lim = 1e-6 * float(mod.sig2) * float(alpha.abs().sum()) + F64_BOUND * float(alpha.abs().sum())
        gap = float((win - dense).abs().max())
        print(f"{family}: windowed predict_mean: max gap {gap:.3e}, bound {lim:.3e}")
        assert gap <= lim
        # draws with the randomness passed in repeat
        F = 256
        gen = torch.Generator().manual_seed(3)
        from hipgp_amd import rff
        feats = rff.spectral_features(mod.kernel, mod.get_kernel_params(), 2, F, generator=gen)
        rnd = dict(eps=torch.randn(2, mod.Mprime, generator=gen, dtype=torch.float64), features=feats,
                   prior_w=torch.randn(2, F, generator=gen, dtype=torch.float64),
                   nugget_eps=torch.randn(2, mod.M, generator=gen, dtype=torch.float64))
        d1 = mod.predict_samples(x, 2, nfeat=F, maxiter_cg=MAXITER, **rnd)
        d2 = mod.predict_samples(x, 2, nfeat=F, maxiter_cg=MAXITER, **rnd)
        assert tuple(d1.shape) == (2, MNOBS) and bool(torch.isfinite(d1).all()) and torch.equal(d1, d2)
        dd = mod.predict_draws(x, 2, eps=rnd["eps"], maxiter_cg=MAXITER)
        assert tuple(dd.shape) == (2, MNOBS) and bool(torch.isfinite(dd).all())
        for call in (lambda: mod.predict(x, integrated_obs=True), lambda: mod.predict_mean(x, integrated_obs=True),
                     lambda: mod.fit_mean(x, y, integrated_obs=True), lambda: mod._make_grams(x, integrated_obs=True)):
            with pytest.raises(NotImplementedError, match="one length scale per axis"):
                call()
    # fit_mean against batch_solve
    sd = torch.full((MNOBS, 1), 0.2, dtype=torch.float64, device=DEV)
    dense_mod = copy.deepcopy(mod)
    dense_mod.batch_solve(x, y, noise_std=sd, maxiter_cg=200)
    fit = mod.fit_mean(x, y, noise_std=sd, tol=1e-10, maxiter=2000)
    qm = mod.standard_variational_params()[0].detach()
    qd = dense_mod.standard_variational_params()[0].detach()
    g = _gap(qm, qd)
    print(f"{family}: fit_mean {fit.iters} iterations, relres {fit.relres:.2e}; against batch_solve: relative gap {g:.3e} "
          f"(limit {10 * GAP_BATCH_SOLVE_F64_MEASURED:.1e})")
    assert fit.relres < 1e-10 and fit.iters < 2000
    assert g <= 10 * GAP_BATCH_SOLVE_F64_MEASURED


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_model_learns_every_length_scale(family):
    """elbo_and_grad(learn_kernel=True): a (2,) gradient for log_ell, the same with `kuf_grad` on and off to
    the fp64 tolerance of tests/test_kuf_grad_gpu.py for that pair, 1e-6 relative plus 1e-9 (the ELBO itself
    to 1e-6 relative).  Both PCGs run to their break test (maxiter_cg = 400): K at ell = (0.3, 0.12) on this
    grid is ill conditioned, and 50 iterations stop two roundings-apart inputs 2e-4 apart in the ELBO
    (measured: -36.38952 against -36.38204, the gradients 0.3 to 2 % apart)."""
    x, y = _data()
    grads = {}
    for knob in (False, True):
        mod = _model(family, learn=True)
        mod.kuf_grad = knob
        Knm = mod._make_grams(x)[0]
        assert (type(Knm.grad_fn).__name__ == "_KufADBackward") == knob
        for route in (dict(), dict(fused=True), dict(streamed=True)):
            mod.zero_grad()
            elbo = mod.elbo_and_grad(x, y, maxiter_cg=MAXITER, **route)
            elbo.backward()
            g = torch.cat([mod.log_sig2.grad.reshape(1), mod.log_ell.grad]).double().cpu().numpy()
            assert tuple(mod.log_ell.grad.shape) == (2,) and np.all(np.isfinite(g)) and np.all(g[1:] != 0)
            grads[(knob, tuple(route))] = (float(elbo.detach()), g)
    for route in ((), ("fused",), ("streamed",)):
        (e0, g0), (e1, g1) = grads[(False, route)], grads[(True, route)]
        print(f"{family} {route or 'materialised'}: elbo {e0!r} / {e1!r}, grads off {g0}, on {g1}")
        assert abs(e0 - e1) <= 1e-6 * abs(e0)
        assert np.all(np.abs(g1 - g0) <= 1e-6 * np.abs(g0) + 1e-9), (g0, g1)
