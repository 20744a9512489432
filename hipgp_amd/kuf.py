"""Cross covariances on the inducing grid: point observations (hgp_kuf_grid) and line-integral
observations (hgp_kuf_semi_mc / hgp_kuf_semi_sqexp / hgp_knn_doubly_diag).

`svi_gp._make_grams` (`svi_gp.py:48-76`) evaluates Knm = kernel(xbatch, xinduce) through the
(B, M, D) broadcast of `kernels.py:78,149`; this computes the same values with one fused HIP
kernel straight into the (B, M) layout the PCG reads.  Used when the kernel is SqExp or
Matern(nu in {1/2, 3/2, 5/2}) with a scalar length scale and no gradient is needed; other
kernels (or kernel-hyper-parameter learning) evaluate the torch kernel on the device.  A SqExp
declared with `ard=True` also takes one length scale per axis for point observations
(`kernels.py:73-79`: ell "a scalar, or a tensor that matches the dimension of data"), through the
hgp_kuf_grid*_ard entries: `kuf_grid`, the two products, their windowed twins (one radius per axis)
and `kuf_grid_ad`.  Without that declaration a vector ell is declined as before, and the
line-integral functions decline it always.

Kernel-hyper-parameter learning has fused twins, `kuf_grid_ad` / `kuf_semi_mc_ad` /
`kuf_semi_sqexp_ad`: the same forward, and the gradient with respect to (sig2, ell) by
hgp_kuf_*_grad, which recomputes K instead of keeping the broadcast for autograd
(`SviGP._make_grams` uses them when the model's `kuf_grad` knob is on).

Products with Knm that never store it, `kuf_grid_matvec` / `kuf_semi_mc_matvec` /
`kuf_semi_sqexp_matvec` (hgp_kuf_*_matvec): Knm @ W^T for a few weight rows W, what the posterior
mean and draws at many points need once K^-1 R v is solved (`ToeplitzInducingGP.predict_mean`).
Their transposes, `kuf_grid_rmatvec` / `kuf_semi_mc_rmatvec` / `kuf_semi_sqexp_rmatvec`
(hgp_kuf_*_rmatvec): C @ Knm for a few coefficient rows C, the other half of the matrix-free
operator K + Knm^T diag(iv) Knm behind `ToeplitzInducingGP.fit_mean`.

The point-observation pair of those also over a window, for kernels far shorter than the grid:
`support_radius` (the truncation rule), `WindowPlan`, `kuf_grid_matvec_win` / `kuf_grid_rmatvec_win`
(hgp_kuf_grid_matvec_win / hgp_kuf_grid_rmatvec_win), within tol * sig2 * sum |w| of the dense ones.
The line-integral pairs over the window of a line, a tube around its segment: `LineWindowPlan`,
`kuf_semi_mc_matvec_win` / `kuf_semi_mc_rmatvec_win`, `kuf_semi_sqexp_matvec_win` /
`kuf_semi_sqexp_rmatvec_win` (hgp_kuf_semi_*_win).
"""
import ctypes

import torch

from . import _lib
from ._lib import check, lib


def kernel_kind(kernel, gneiting=False):
    """HGP_KERN_* code of a ziggy kernel object, or None when the fused kernel does not apply."""
    from hipgp_amd.ziggy import kernels as zk
    if isinstance(kernel, zk.SqExp):
        return _lib.KERN_SQEXP
    if gneiting and isinstance(kernel, zk.Gneiting):
        return _lib.KERN_GNEITING
    if isinstance(kernel, zk.Matern):
        return {0.5: _lib.KERN_MATERN12, 1.5: _lib.KERN_MATERN32, 2.5: _lib.KERN_MATERN52}.get(kernel.nu)
    return None


def _scalar(v):
    if torch.is_tensor(v):
        if v.numel() != 1:
            return None
        return float(v.detach().reshape(()).item())
    return float(v)


def _ell_form(v, D):
    """0 for a scalar ell (a number, or a tensor of one element), 1 for one length scale per axis (a 1-D
    tensor or a sequence of length D), else None; no value is read."""
    if torch.is_tensor(v):
        return 0 if v.numel() == 1 else 1 if v.dim() == 1 and v.numel() == D else None
    if isinstance(v, (list, tuple)):
        return 1 if len(v) == D else None
    return 0


def _ell_arg(v, D):
    """ell as the fused kernels take it: a float for a scalar (number, or tensor of one element), a
    list of D floats for a 1-D tensor or sequence of length D (one length scale per axis), else None."""
    form = _ell_form(v, D)
    if form is None:
        return None
    if form == 0:
        return _scalar(v)
    return [float(e) for e in (v.detach().cpu().tolist() if torch.is_tensor(v) else v)]


def _is_ard(el):
    return isinstance(el, list)


def _takes_ard(kernel):
    """True for a SqExp declared with one length scale per axis (`SqExp(ard=True)`): the only kernel
    for which a vector ell is read as per-axis scales; every other kernel declines a vector."""
    from hipgp_amd.ziggy import kernels as zk
    return isinstance(kernel, zk.SqExp) and bool(getattr(kernel, "ard", False))


def _dvec(vals):
    """host doubles for a `const double*` argument"""
    return (ctypes.c_double * len(vals))(*vals)


def _gate(kernel, xgrids, x, params, gneiting=False, ard=False, graph=False):
    """The HGP_KERN_* code, or None where the fused kernels decline: a kernel without a fused forward
    (`gneiting`: the Monte-Carlo line integral also takes Gneiting), a CPU tensor, x not (nobs, D <= 3)
    in fp32 / fp64, a non-scalar sig2, an ell that is neither a scalar nor -- with `ard` (the point
    functions), for a SqExp declared with ard=True -- one value per axis, a graph to x, and a graph to
    sig2 or ell unless that graph is the point (`graph`: the `_ad` functions)."""
    kind = kernel_kind(kernel, gneiting=gneiting)
    if kind is None or x.device.type != "cuda" or x.dim() != 2 or x.shape[1] != len(xgrids):
        return None
    if x.dtype not in (torch.float32, torch.float64) or len(xgrids) > 3:
        return None
    sig2, ell = params
    if torch.is_grad_enabled() and any(torch.is_tensor(p) and p.requires_grad
                                       for p in ((x,) if graph else (sig2, ell, x))):
        return None
    if torch.is_tensor(sig2) and sig2.numel() != 1:
        return None
    form = _ell_form(ell, len(xgrids))
    if form is None:
        return None
    if form == 1 and not (ard and _takes_ard(kernel)):
        return None
    return kind


def _grid_call_args(kernel, xgrids, x, params, gneiting=False, ard=False):
    """(kind, s2, el, grids, xc, M) for the fused grid kernels, or None when they do not apply (`_gate`).
    el is a float, or a list of one float per axis for a vector ell."""
    kind = _gate(kernel, xgrids, x, params, gneiting=gneiting, ard=ard)
    if kind is None:
        return None
    grids = [g.to(device=x.device, dtype=x.dtype).contiguous() for g in xgrids]
    M = 1
    for g in grids:
        M *= g.numel()
    return kind, _scalar(params[0]), _ell_arg(params[1], len(grids)), grids, x.detach().contiguous(), M


def _grid_ptrs(grids):
    m = (ctypes.c_int64 * len(grids))(*[g.numel() for g in grids])
    ptrs = (ctypes.c_void_p * len(grids))(*[g.data_ptr() for g in grids])
    return m, ptrs


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _offset_draw(u, dtype, x):
    """The Monte-Carlo offset as the entries take it, one element on x's device in x's dtype: the given
    `u`, or one torch.rand(1) draw in the kernel's dtype exactly as the reference (`kernels.py:28-29`).
    Called after every way of declining, so that a declined call consumes nothing."""
    if u is None:
        u = torch.rand(1, dtype=dtype, device=x.device)
    return u.detach().to(device=x.device, dtype=x.dtype).reshape(1).contiguous()


def _kuf_head(x, grids, s2, el, pre=(), rho=None, mc=None):
    """(ard, head) of one hgp_kuf_* entry: head is what follows dtype, `pre` (the entry's kind, or kind and
    kp, if it takes them), ndim, m, grids, x, nobs, sig2, ell, [rho], [npts, u] with mc = (npts, u).  A list
    ell (and rho) goes as host doubles and `ard` says that the entry named *_ard reads them."""
    m, ptrs = _grid_ptrs(grids)
    ard = _is_ard(el)
    head = [*pre, len(grids), m, ptrs, _ptr(x), x.shape[0], s2, _dvec(el) if ard else el]
    if rho is not None:
        head.append(_dvec(rho) if ard else rho)
    if mc is not None:
        head += (int(mc[0]), _ptr(mc[1]))
    return ard, head


def _kuf_call(name, out, x, grids, s2, el, *tail, **head):
    """Run one hgp_kuf_* entry (`name`, or name_ard for a list ell): dtype, `_kuf_head`, the entry's own
    `tail` as ctypes values, then `out` and the stream.  Returns `out`."""
    ard, args = _kuf_head(x, grids, s2, el, **head)
    check(getattr(lib(), name + "_ard" if ard else name)(_lib.dtype_code(x.dtype), *args, *tail, _ptr(out),
                                                         _lib.stream_ptr(x.device)))
    return out


def kuf_grid(kernel, xgrids, x, params):
    """Knm (nobs, M) for observations x (nobs, D) against the C-order mesh of xgrids, or None
    when the fused path does not apply (caller then evaluates the torch kernel)."""
    a = _grid_call_args(kernel, xgrids, x, params, ard=True)
    if a is None:
        return None
    kind, s2, el, grids, xc, M = a
    out = torch.empty((x.shape[0], M), dtype=x.dtype, device=x.device)
    return _kuf_call("hgp_kuf_grid", out, xc, grids, s2, el, pre=(kind,))


def kuf_semi_mc(kernel, xgrids, x, params, npts, u=None):
    """Line-integral Knm (nobs, M) by the reference's biased Monte-Carlo estimator
    (`Kernel.k_semi_mc` `kernels.py:19-39`, as `svi_gp.py:61-64` uses it), or None when the
    fused path does not apply.  Consumes one torch.rand(1) draw exactly as the reference, or
    uses the given offset draw `u` (a 1-element tensor in [0, 1))."""
    a = _grid_call_args(kernel, xgrids, x, params, gneiting=True)
    if a is None:
        return None
    kind, s2, el, grids, xc, M = a
    out = torch.empty((x.shape[0], M), dtype=x.dtype, device=x.device)
    return _kuf_call("hgp_kuf_semi_mc", out, xc, grids, s2, el,
                     pre=(kind, float(getattr(kernel, "alpha", 1.))), mc=(npts, _offset_draw(u, kernel.dtype, x)))


def kuf_semi_sqexp(kernel, xgrids, x, params):
    """Analytic SqExp line-integral Knm (nobs, M) (`SqExp.k_semi` `kernels.py:80-85` ->
    `semi_integrated_sqe` `:223-237`), or None when the fused path does not apply."""
    a = _grid_call_args(kernel, xgrids, x, params)
    if a is None or a[0] != _lib.KERN_SQEXP:
        return None
    kind, s2, el, grids, xc, M = a
    out = torch.empty((x.shape[0], M), dtype=x.dtype, device=x.device)
    return _kuf_call("hgp_kuf_semi_sqexp", out, xc, grids, s2, el)


# ---- products with the cross covariances, Knm never stored (hgp_kuf_*_matvec) -------------------

def _matvec_weights(W, x, M):
    """W as contiguous (nw, M) rows on x's device in x's dtype, or None where the product declines
    (W carries a graph that the kernel would drop)."""
    if torch.is_grad_enabled() and W.requires_grad:
        return None
    W = W.detach()
    if W.dim() == 1:
        W = W[None, :]
    if W.dim() != 2 or W.shape[1] != M:
        raise ValueError(f"W must be (nw, M) or (M,) with M = {M}, got {tuple(W.shape)}")
    return W.to(device=x.device, dtype=x.dtype).contiguous()


def kuf_grid_matvec(kernel, xgrids, x, params, W, nsplit=0):
    """kuf_grid(...) @ W^T as an (nobs, nw) tensor without the (nobs, M) matrix
    (hgp_kuf_grid_matvec): W is (nw, M) or (M,).  nsplit: slices of the grid summed apart (0: the
    library's choice).  None under the rules by which `kuf_grid` declines."""
    a = _grid_call_args(kernel, xgrids, x, params, ard=True)
    if a is None:
        return None
    kind, s2, el, grids, xc, M = a
    Wc = _matvec_weights(W, x, M)
    if Wc is None:
        return None
    out = torch.empty((x.shape[0], Wc.shape[0]), dtype=x.dtype, device=x.device)
    return _kuf_call("hgp_kuf_grid_matvec", out, xc, grids, s2, el, _ptr(Wc), Wc.shape[0], int(nsplit), pre=(kind,))


def kuf_semi_mc_matvec(kernel, xgrids, x, params, npts, u=None, W=None, nsplit=0):
    """kuf_semi_mc(...) @ W^T as an (nobs, nw) tensor without the (nobs, M) matrix
    (hgp_kuf_semi_mc_matvec); the offset draw `u` as in `kuf_semi_mc`."""
    a = _grid_call_args(kernel, xgrids, x, params, gneiting=True)
    if a is None:
        return None
    kind, s2, el, grids, xc, M = a
    if W is None:
        raise TypeError("kuf_semi_mc_matvec needs the weight rows W")
    Wc = _matvec_weights(W, x, M)
    if Wc is None:
        return None
    out = torch.empty((x.shape[0], Wc.shape[0]), dtype=x.dtype, device=x.device)
    return _kuf_call("hgp_kuf_semi_mc_matvec", out, xc, grids, s2, el, _ptr(Wc), Wc.shape[0], int(nsplit),
                     pre=(kind, float(getattr(kernel, "alpha", 1.))), mc=(npts, _offset_draw(u, kernel.dtype, x)))


def kuf_semi_sqexp_matvec(kernel, xgrids, x, params, W, nsplit=0):
    """kuf_semi_sqexp(...) @ W^T as an (nobs, nw) tensor without the (nobs, M) matrix
    (hgp_kuf_semi_sqexp_matvec); SqExp only, like the forward."""
    a = _grid_call_args(kernel, xgrids, x, params)
    if a is None or a[0] != _lib.KERN_SQEXP:
        return None
    kind, s2, el, grids, xc, M = a
    Wc = _matvec_weights(W, x, M)
    if Wc is None:
        return None
    out = torch.empty((x.shape[0], Wc.shape[0]), dtype=x.dtype, device=x.device)
    return _kuf_call("hgp_kuf_semi_sqexp_matvec", out, xc, grids, s2, el, _ptr(Wc), Wc.shape[0], int(nsplit))


# ---- products with the transposed cross covariances, Knm never stored (hgp_kuf_*_rmatvec) -------

def _rmatvec_coefs(C, x):
    """C as contiguous (nc, nobs) rows on x's device in x's dtype, or None where the product
    declines (C carries a graph that the kernel would drop)."""
    if torch.is_grad_enabled() and C.requires_grad:
        return None
    C = C.detach()
    if C.dim() == 1:
        C = C[None, :]
    if C.dim() != 2 or C.shape[1] != x.shape[0]:
        raise ValueError(f"C must be (nc, nobs) or (nobs,) with nobs = {x.shape[0]}, got {tuple(C.shape)}")
    return C.to(device=x.device, dtype=x.dtype).contiguous()


def kuf_grid_rmatvec(kernel, xgrids, x, params, C, nsplit=0):
    """C @ kuf_grid(...) as an (nc, M) tensor without the (nobs, M) matrix (hgp_kuf_grid_rmatvec):
    C is (nc, nobs) or (nobs,).  nsplit: slices of the observations summed apart (0: the library's
    choice).  None under the rules by which `kuf_grid` declines."""
    a = _grid_call_args(kernel, xgrids, x, params, ard=True)
    if a is None:
        return None
    kind, s2, el, grids, xc, M = a
    Cc = _rmatvec_coefs(C, x)
    if Cc is None:
        return None
    out = torch.empty((Cc.shape[0], M), dtype=x.dtype, device=x.device)
    return _kuf_call("hgp_kuf_grid_rmatvec", out, xc, grids, s2, el, _ptr(Cc), Cc.shape[0], int(nsplit), pre=(kind,))


def kuf_semi_mc_rmatvec(kernel, xgrids, x, params, npts, u=None, C=None, nsplit=0):
    """C @ kuf_semi_mc(...) as an (nc, M) tensor without the (nobs, M) matrix
    (hgp_kuf_semi_mc_rmatvec); the offset draw `u` as in `kuf_semi_mc`."""
    a = _grid_call_args(kernel, xgrids, x, params, gneiting=True)
    if a is None:
        return None
    kind, s2, el, grids, xc, M = a
    if C is None:
        raise TypeError("kuf_semi_mc_rmatvec needs the coefficient rows C")
    Cc = _rmatvec_coefs(C, x)
    if Cc is None:
        return None
    out = torch.empty((Cc.shape[0], M), dtype=x.dtype, device=x.device)
    return _kuf_call("hgp_kuf_semi_mc_rmatvec", out, xc, grids, s2, el, _ptr(Cc), Cc.shape[0], int(nsplit),
                     pre=(kind, float(getattr(kernel, "alpha", 1.))), mc=(npts, _offset_draw(u, kernel.dtype, x)))


def kuf_semi_sqexp_rmatvec(kernel, xgrids, x, params, C, nsplit=0):
    """C @ kuf_semi_sqexp(...) as an (nc, M) tensor without the (nobs, M) matrix
    (hgp_kuf_semi_sqexp_rmatvec); SqExp only, like the forward."""
    a = _grid_call_args(kernel, xgrids, x, params)
    if a is None or a[0] != _lib.KERN_SQEXP:
        return None
    kind, s2, el, grids, xc, M = a
    Cc = _rmatvec_coefs(C, x)
    if Cc is None:
        return None
    out = torch.empty((Cc.shape[0], M), dtype=x.dtype, device=x.device)
    return _kuf_call("hgp_kuf_semi_sqexp_rmatvec", out, xc, grids, s2, el, _ptr(Cc), Cc.shape[0], int(nsplit))


# ---- the same two products over a window: kernels far shorter than the grid ----------------------
# A point only sees the nodes within the kernel's reach.  `support_radius` is the truncation rule,
# `WindowPlan` holds what the two products share for one set of points, `kuf_grid_matvec_win` /
# `kuf_grid_rmatvec_win` are the products (hgp_kuf_grid_matvec_win / hgp_kuf_grid_rmatvec_win).  Per
# output the windowed product is within tol * sig2 * sum |w| (or sum |c|) of the dense one.

def _kern_unit64(kind, r, el):
    """k(r) / sig2 in fp64 by the formulas of the device's `kern_eval`."""
    import math
    if kind == _lib.KERN_SQEXP:
        dv = r / el
        return math.exp(-(dv * dv) / 2)
    if kind == _lib.KERN_MATERN12:
        return math.exp(-r / el)
    if kind == _lib.KERN_MATERN32:
        dp = 1.7320508075688772935 * r / el
        return (1 + dp) * math.exp(-dp)
    dp = 2.2360679774997896964 * r / el
    return (1 + dp + (5. / 3.) * (r * r) / (el * el)) * math.exp(-dp)


def support_radius(kernel, params, tol):
    """The smallest distance rho (a float, fp64) with k(r) <= tol * sig2 for every r >= rho, or
    None where no rule applies: Gneiting or a kernel without a fused forward, a vector `ell` with
    a kernel other than a SqExp declared with ard=True, `tol` outside (0, 1).  SqExp in closed form, ell * sqrt(2 ln(1 / tol))
    (moved up by at most a few ulps so that the fp64 formula itself is <= tol there); Matern 1/2, 3/2,
    5/2, all decreasing in r, by bisection on the fp64 formula.

    `SqExp(ard=True)` with a vector `ell` (a 1-D tensor or a sequence, one length scale per axis): a list,
    rho[a] = ell[a] * sqrt(2 ln(1 / tol)), each moved up as the scalar is, so that axis a's factor
    exp(-(rho[a] / ell[a])^2 / 2) alone is <= tol.  The window is then the box |x_a - u_a| <= rho[a]
    on every axis, and the bound is the scalar one: a pair outside has an axis with
    (d_a / ell[a])^2 > 2 ln(1 / tol), the other factors are <= 1, hence k < tol * sig2, and a
    windowed product is within tol * sig2 * sum |w| of the dense one per output."""
    import math
    kind = kernel_kind(kernel)
    if kind is None or tol is None:
        return None
    tol = float(tol)
    if not (0. < tol < 1.):
        return None
    sig2, ell = params
    if torch.is_tensor(ell) and ell.numel() != 1 or isinstance(ell, (list, tuple)):
        el = _ell_arg(ell, ell.numel() if torch.is_tensor(ell) else len(ell))
        if not _takes_ard(kernel) or _scalar(sig2) is None or not _is_ard(el):
            return None
        if not all(e > 0 and math.isfinite(e) for e in el):
            return None
        return [support_radius(kernel, (sig2, e), tol) for e in el]
    s2, el = _scalar(sig2), _scalar(ell)
    if s2 is None or el is None or not (el > 0) or not math.isfinite(el):
        return None
    if kind == _lib.KERN_SQEXP:
        rho = el * math.sqrt(2 * math.log(1 / tol))
        for _ in range(4):
            if _kern_unit64(kind, rho, el) <= tol:
                break
            rho = math.nextafter(rho, math.inf)
        return rho
    lo, hi = 0., el
    while _kern_unit64(kind, hi, el) > tol:
        lo, hi = hi, 2 * hi
    for _ in range(200):                  # k(lo) > tol >= k(hi) throughout
        mid = .5 * (lo + hi)
        if not (lo < mid < hi):
            break
        if _kern_unit64(kind, mid, el) <= tol:
            hi = mid
        else:
            lo = mid
    return hi


def win_bins(dims):
    """(tile, nbins) per axis as hgp_kuf_grid_rmatvec_win assumes them (hgp_kuf_win_bins): along
    axis a a tile has tile[a] mesh points and a bin tile[a] cells; nbins[a] = m[a] // tile[a] + 1."""
    nd = len(dims)
    m = (ctypes.c_int64 * nd)(*[int(v) for v in dims])
    tile, nbins = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    check(lib().hgp_kuf_win_bins(nd, m, tile, nbins))
    return list(tile)[:nd], list(nbins)[:nd]


class WindowPlan:
    """What the windowed products share for one set of points x against one grid: the radius rho
    (`support_radius(kernel, params, tol)`, or the given `rho`), the contiguous grids and x, and
    the observations sorted by bin (`order`, `bin_start`; built on the first transposed product).
    Build it once and use it for any number of products; x, the grids and the kernel parameters
    are read here and must not change while the plan is in use.

    Pair (n, j) is in the window iff |x[n, a] - g_a[j_a]| <= rho on every axis a, evaluated in
    x's dtype with rho rounded once to that dtype.  `SqExp(ard=True)` with a vector ell: `ell` and `rho` are
    lists, one value per axis, and the predicate reads rho[a] on axis a (a scalar `rho` given with a
    vector ell stands on every axis).  The constructor raises ValueError where the windowed products
    do not apply; `WindowPlan.make` returns None there instead."""

    def __init__(self, kernel, xgrids, x, params, tol, rho=None):
        a = _grid_call_args(kernel, xgrids, x, params, ard=True)
        if rho is None:
            rho = support_radius(kernel, params, tol)
        if a is not None and rho is not None and _is_ard(a[2]):
            rho = [float(r) for r in rho] if isinstance(rho, (list, tuple)) else [float(rho)] * len(a[2])
            ok = len(rho) == len(a[2]) and all(r >= 0 and r != float("inf") for r in rho)
        else:
            ok = a is not None and rho is not None and not isinstance(rho, (list, tuple)) and \
                float(rho) >= 0 and float(rho) != float("inf")
        if not ok:
            raise ValueError("the windowed Kuf products do not apply: they take SqExp / Matern(1/2, 3/2, 5/2) with a "
                             "scalar ell (SqExp(ard=True) also one ell per axis), a tolerance in (0, 1), device points "
                             "(nobs, D <= 3) in fp32 / fp64 and no graph to x, sig2 or ell")
        self.kind, self.sig2, self.ell, self.grids, self.x, self.M = a
        self.rho, self.tol = rho if _is_ard(self.ell) else float(rho), tol
        self.dims = [g.numel() for g in self.grids]
        self._bins = None

    @classmethod
    def make(cls, kernel, xgrids, x, params, tol, rho=None):
        """The plan, or None where `support_radius` or the fused grid kernels decline."""
        try:
            return cls(kernel, xgrids, x, params, tol, rho=rho)
        except ValueError:
            return None

    @property
    def nobs(self):
        return self.x.shape[0]

    def bins(self):
        """(order, bin_start): the observations sorted stably by bin, and the bins' offsets in that
        list (total bins + 1), both int64 on the device.  The bin of x on axis a is (number of
        nodes <= x_a) // tile[a]; bins are numbered in C order over the axes."""
        if self._bins is None:
            tile, nbins = win_bins(self.dims)
            b = torch.zeros(self.nobs, dtype=torch.int64, device=self.x.device)
            total = 1
            for a, g in enumerate(self.grids):
                cell = torch.searchsorted(g, self.x[:, a].contiguous(), right=True).clamp_(0, g.numel())
                b = b * nbins[a] + torch.div(cell, tile[a], rounding_mode="floor")
                total *= nbins[a]
            order = torch.sort(b, stable=True).indices.contiguous()
            start = torch.zeros(total + 1, dtype=torch.int64, device=self.x.device)
            start[1:] = torch.cumsum(torch.bincount(b, minlength=total), 0)
            self._bins = (order, start)
        return self._bins


def kuf_grid_matvec_win(plan, W):
    """The windowed kuf_grid(...) @ W^T, (nobs, nw), for the plan's points (hgp_kuf_grid_matvec_win):
    W is (nw, M) or (M,).  Within plan.tol * sig2 * sum_j |W[s, j]| of `kuf_grid_matvec` per output;
    a point with an empty window gives exact zeros.  None where W carries a graph."""
    x = plan.x
    Wc = _matvec_weights(W, x, plan.M)
    if Wc is None:
        return None
    out = torch.empty((x.shape[0], Wc.shape[0]), dtype=x.dtype, device=x.device)
    return _kuf_call("hgp_kuf_grid_matvec_win", out, x, plan.grids, plan.sig2, plan.ell, _ptr(Wc), Wc.shape[0],
                     pre=(plan.kind,), rho=plan.rho)


def kuf_grid_rmatvec_win(plan, C):
    """The windowed C @ kuf_grid(...), (nc, M), for the plan's points (hgp_kuf_grid_rmatvec_win): C is
    (nc, nobs) or (nobs,).  The exact transpose of `kuf_grid_matvec_win` on the same plan (the same
    pairs, the same element values); within plan.tol * sig2 * sum_n |C[s, n]| of `kuf_grid_rmatvec`
    per output.  No observations: zeros.  None where C carries a graph."""
    x = plan.x
    Cc = _rmatvec_coefs(C, x)
    if Cc is None:
        return None
    out = torch.empty((Cc.shape[0], plan.M), dtype=x.dtype, device=x.device)
    order, start = plan.bins() if x.shape[0] > 0 else (None, None)
    return _kuf_call("hgp_kuf_grid_rmatvec_win", out, x, plan.grids, plan.sig2, plan.ell, _ptr(Cc), Cc.shape[0],
                     _ptr(order), _ptr(start), pre=(plan.kind,), rho=plan.rho)


# ---- the two line-integral products over the window of a line: a tube around its segment --------
# Line n is the segment from the origin to x_n.  It is cut into pieces[n] equal pieces; a node is in
# the line's window iff it lies in the bounding box of some piece widened by rho on every axis, which
# holds every node within Chebyshev distance rho of the segment.  Per output the windowed product is
# within tol * sig2 * |x_n| * sum |w| (transposed: tol * sig2 * sum_n |c_n| |x_n|) of the dense one.

LINE_MAX_PIECES = 64


def line_pieces(x, rho):
    """Pieces per line, int32 (nobs,): about one per rho of the line's largest |x_a|, at least 1 and
    at most LINE_MAX_PIECES (longer pieces beyond: a larger window, still a superset of the tube).
    x = 0 and NaN rows get 1."""
    xa = x.detach().abs().amax(dim=1).double()
    p = torch.ceil(xa / float(rho)) if float(rho) > 0 else torch.full_like(xa, float(LINE_MAX_PIECES))
    p = torch.nan_to_num(p, nan=1., posinf=float(LINE_MAX_PIECES))
    return p.clamp_(1, LINE_MAX_PIECES).to(torch.int32).contiguous()


class LineWindowPlan:
    """What the windowed line-integral products share for one set of lines x against one grid: the
    radius rho (`support_radius(kernel, params, tol)`, or the given `rho`), the contiguous grids and
    x, and the pieces per line (`line_pieces`), computed once so that both products read the same
    numbers.  x, the grids and the kernel parameters must not change while the plan is in use.  The
    constructor raises ValueError where the products do not apply; `make` returns None there."""

    def __init__(self, kernel, xgrids, x, params, tol, rho=None):
        a = _grid_call_args(kernel, xgrids, x, params) if torch.is_tensor(x) and xgrids is not None else None
        if rho is None and a is not None:
            rho = support_radius(kernel, params, tol)
        if a is None or rho is None or not (float(rho) >= 0) or float(rho) == float("inf"):
            raise ValueError("the windowed line-integral Kuf products do not apply: they take SqExp / Matern(1/2, "
                             "3/2, 5/2) with a scalar ell, a tolerance in (0, 1), device lines (nobs, D <= 3) in "
                             "fp32 / fp64 and no graph to x, sig2 or ell")
        self.kind, self.sig2, self.ell, self.grids, self.x, self.M = a
        self.kernel_dtype = getattr(kernel, "dtype", x.dtype)
        self.rho, self.tol = float(rho), tol
        self.dims = [g.numel() for g in self.grids]
        self.pieces = line_pieces(self.x, self.rho)

    @classmethod
    def make(cls, kernel, xgrids, x, params, tol, rho=None):
        """The plan, or None where `support_radius` or the fused grid kernels decline."""
        try:
            return cls(kernel, xgrids, x, params, tol, rho=rho)
        except ValueError:
            return None

    @property
    def nobs(self):
        return self.x.shape[0]


def _line_win_call(plan, name, rows, out, npts=None, u=None):
    """One hgp_kuf_semi_*_win entry: `rows` are the weight or coefficient rows."""
    mc = {} if npts is None else dict(pre=(plan.kind,), mc=(npts, _offset_draw(u, plan.kernel_dtype, plan.x)))
    return _kuf_call(name, out, plan.x, plan.grids, plan.sig2, plan.ell, _ptr(plan.pieces), plan.pieces.shape[0],
                     _ptr(rows), rows.shape[0], rho=plan.rho, **mc)


def kuf_semi_mc_matvec_win(plan, W, npts, u=None):
    """The windowed kuf_semi_mc(...) @ W^T, (nobs, nw), for the plan's lines
    (hgp_kuf_semi_mc_matvec_win): W is (nw, M) or (M,), the offset draw `u` as in `kuf_semi_mc`.
    Within plan.tol * sig2 * |x_n| * sum_j |W[s, j]| of `kuf_semi_mc_matvec` per output; a line with
    an empty window (x = 0 included) gives exact zeros.  None where W carries a graph."""
    Wc = _matvec_weights(W, plan.x, plan.M)
    if Wc is None:
        return None
    out = torch.empty((plan.nobs, Wc.shape[0]), dtype=plan.x.dtype, device=plan.x.device)
    return _line_win_call(plan, "hgp_kuf_semi_mc_matvec_win", Wc, out, npts=npts, u=u)


def kuf_semi_sqexp_matvec_win(plan, W):
    """The windowed kuf_semi_sqexp(...) @ W^T (hgp_kuf_semi_sqexp_matvec_win); SqExp only (None
    otherwise).  A line with x = 0 gives zeros where the dense product gives NaN."""
    if plan.kind != _lib.KERN_SQEXP:
        return None
    Wc = _matvec_weights(W, plan.x, plan.M)
    if Wc is None:
        return None
    out = torch.empty((plan.nobs, Wc.shape[0]), dtype=plan.x.dtype, device=plan.x.device)
    return _line_win_call(plan, "hgp_kuf_semi_sqexp_matvec_win", Wc, out)


def kuf_semi_mc_rmatvec_win(plan, C, npts, u=None):
    """The windowed C @ kuf_semi_mc(...), (nc, M), for the plan's lines (hgp_kuf_semi_mc_rmatvec_win):
    the exact transpose of `kuf_semi_mc_matvec_win` on the same plan and offset (the same pairs, the
    same element values); within plan.tol * sig2 * sum_n |C[s, n]| |x_n| of the dense product per
    output.  No lines: zeros.  None where C carries a graph."""
    Cc = _rmatvec_coefs(C, plan.x)
    if Cc is None:
        return None
    out = torch.empty((Cc.shape[0], plan.M), dtype=plan.x.dtype, device=plan.x.device)
    return _line_win_call(plan, "hgp_kuf_semi_mc_rmatvec_win", Cc, out, npts=npts, u=u)


def kuf_semi_sqexp_rmatvec_win(plan, C):
    """The windowed C @ kuf_semi_sqexp(...) (hgp_kuf_semi_sqexp_rmatvec_win), the exact transpose of
    `kuf_semi_sqexp_matvec_win`; SqExp only (None otherwise)."""
    if plan.kind != _lib.KERN_SQEXP:
        return None
    Cc = _rmatvec_coefs(C, plan.x)
    if Cc is None:
        return None
    out = torch.empty((Cc.shape[0], plan.M), dtype=plan.x.dtype, device=plan.x.device)
    return _line_win_call(plan, "hgp_kuf_semi_sqexp_rmatvec_win", Cc, out)


def knn_doubly_diag(table, x, params):
    """Knn_diag (nobs,) of line-integral observations by the reference's table interpolation
    (`KernelDoublyDiagInterpolator.forward` `kernels.py:200-220`); table: device tensor (3, N)
    = distance grid, knn, slopes in x.dtype."""
    _lib.require_device_tensor(x, "x")
    sig2, ell = params
    s2, el = _scalar(sig2), _scalar(ell)
    if s2 is None or el is None:
        raise _lib.HipgpError("k_doubly_diag: sig2 / ell must be scalars")
    xc = x.detach().contiguous()
    tab = table.to(device=x.device, dtype=x.dtype).contiguous()
    out = torch.empty((x.shape[0],), dtype=x.dtype, device=x.device)
    check(lib().hgp_knn_doubly_diag(_lib.dtype_code(x.dtype), x.shape[1], ctypes.c_void_p(xc.data_ptr()), x.shape[0],
                                    s2, el, ctypes.c_void_p(tab.data_ptr()), tab.shape[1],
                                    ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr(x.device)))
    return out


# ---- the same cross covariances with a graph to (sig2, ell): kernel hyper-parameter learning ----
# The forward is the fused kernel above; the backward is two scalar sums over (nobs, M) with K
# recomputed in the kernel (hgp_kuf_*_grad), so nothing of the (nobs, M, D) broadcast that torch's
# autograd of `kernels.py:73-79, 145-158, 19-39, 80-85, 223-237` saves is ever allocated.

class _KufAD(torch.autograd.Function):
    """out = fwd(sig2, ell) (the plain fused forward on the detached scalars); the backward hands
    the upstream gradient to bwd(sig2, ell, G) -> grad2 = (sum G dK/dsig2, sum G dK/dell).  Only
    the detached scalars are kept on ctx; x, the grids and the MC offset live in the closures.
    A vector ell (`kuf_grid_ad` with SqExp) is kept as a list of floats and bwd returns
    (sum G dK/dsig2, sum G dK/dell_a per axis); the ell gradient then has ell's shape."""

    @staticmethod
    def forward(ctx, sig2, ell, fwd, bwd):
        ctx.s2, ctx.bwd = _scalar(sig2), bwd
        ctx.el = _ell_arg(ell, ell.numel() if torch.is_tensor(ell) else len(ell) if isinstance(ell, (list, tuple)) else 1)
        ctx.like = [(p.shape, p.dtype) if torch.is_tensor(p) else None for p in (sig2, ell)]
        return fwd(ctx.s2, ctx.el)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        grad2 = ctx.bwd(ctx.s2, ctx.el, G.contiguous())
        parts = (grad2[:1], grad2[1:])
        out = [parts[i].to(ctx.like[i][1]).reshape(ctx.like[i][0]) if ctx.needs_input_grad[i] else None
               for i in range(2)]
        return out[0], out[1], None, None


def _ad_route(kernel, xgrids, x, params, ard=False):
    """None: the `_ad` function declines (caller evaluates the torch kernel); False: no
    hyper-parameter gradient is asked for (the plain forward serves); else the HGP_KERN_* code.
    ard: a 1-D ell tensor with one entry per axis passes for a SqExp declared with ard=True (the point
    function alone)."""
    if xgrids is None or not torch.is_tensor(x):
        return None
    kind = _gate(kernel, xgrids, x, params, ard=ard, graph=True)     # no Gneiting: its gradient is NaN at r = 0
    if kind is None:
        return None
    if not (torch.is_grad_enabled() and any(torch.is_tensor(p) and p.requires_grad for p in params)):
        return False
    return kind


def _grad_call(entry, x, G, *args, nsum=2):
    """Run one hgp_kuf_*_grad entry: args are everything between dtype and g; nsum values come back."""
    grad2 = torch.empty(nsum, dtype=x.dtype, device=x.device)
    check(entry(_lib.dtype_code(x.dtype), *args, ctypes.c_void_p(G.data_ptr()), ctypes.c_void_p(grad2.data_ptr()),
                _lib.stream_ptr(x.device)))
    return grad2


def _ad_inputs(xgrids, x):
    grids = [g.to(device=x.device, dtype=x.dtype).contiguous() for g in xgrids]
    return grids, x.detach().contiguous()


def kuf_grid_ad(kernel, xgrids, x, params):
    """`kuf_grid` that carries the autograd graph to sig2 / ell: the same forward values, the
    backward by hgp_kuf_grid_grad.  `SqExp(ard=True)` also with a 1-D ell of one entry per axis (backward by
    hgp_kuf_grid_grad_ard; the ell gradient has ell's shape).  None when it does not apply: x requires
    grad, any other non-scalar ell, Gneiting or another kernel without a fused forward, a CPU tensor,
    more than 3 dims."""
    kind = _ad_route(kernel, xgrids, x, params, ard=True)
    if kind is None:
        return None
    if kind is False:
        return kuf_grid(kernel, xgrids, x, params)
    grids, xc = _ad_inputs(xgrids, x)

    def bwd(s2, el, G):
        ard, head = _kuf_head(xc, grids, s2, el, pre=(kind,))
        return _grad_call(lib().hgp_kuf_grid_grad_ard if ard else lib().hgp_kuf_grid_grad, xc, G, *head,
                          nsum=1 + len(el) if ard else 2)
    return _KufAD.apply(params[0], params[1], lambda s2, el: kuf_grid(kernel, grids, xc, (s2, el)), bwd)


def kuf_semi_mc_ad(kernel, xgrids, x, params, npts, u=None):
    """`kuf_semi_mc` with the graph to sig2 / ell (backward: hgp_kuf_semi_mc_grad on the offset
    draw the forward used; drawn here exactly as `kuf_semi_mc` draws it when not given)."""
    kind = _ad_route(kernel, xgrids, x, params)
    if kind is None:
        return None
    if kind is False:
        return kuf_semi_mc(kernel, xgrids, x, params, npts, u=u)
    grids, xc = _ad_inputs(xgrids, x)
    uc = _offset_draw(u, kernel.dtype, x)

    def bwd(s2, el, G):
        return _grad_call(lib().hgp_kuf_semi_mc_grad, xc, G,
                          *_kuf_head(xc, grids, s2, el, pre=(kind, 1.), mc=(npts, uc))[1])
    return _KufAD.apply(params[0], params[1],
                        lambda s2, el: kuf_semi_mc(kernel, grids, xc, (s2, el), npts, u=uc), bwd)


def kuf_semi_sqexp_ad(kernel, xgrids, x, params):
    """`kuf_semi_sqexp` with the graph to sig2 / ell (backward: hgp_kuf_semi_sqexp_grad)."""
    kind = _ad_route(kernel, xgrids, x, params)
    if kind is None or kind is not False and kind != _lib.KERN_SQEXP:
        return None
    if kind is False:
        return kuf_semi_sqexp(kernel, xgrids, x, params)
    grids, xc = _ad_inputs(xgrids, x)

    def bwd(s2, el, G):
        return _grad_call(lib().hgp_kuf_semi_sqexp_grad, xc, G, *_kuf_head(xc, grids, s2, el)[1])
    return _KufAD.apply(params[0], params[1], lambda s2, el: kuf_semi_sqexp(kernel, grids, xc, (s2, el)), bwd)


def knn_doubly_diag_ad(table, x, params):
    """`knn_doubly_diag` in plain torch, the reference's own formula
    (`KernelDoublyDiagInterpolator.forward` `kernels.py:199-218`), so that Knn_diag carries the
    graph to sig2 / ell; nobs values, any device.  table: (3, N) = distance grid, knn, slopes."""
    sig2, ell = params
    grid, knn, slopes = table.to(device=x.device, dtype=x.dtype)
    dists = torch.sqrt(torch.sum((x / ell) ** 2, dim=-1))
    lo = torch.sum(dists[:, None] > grid, -1) - 1            # -1 wraps to the last entry, as the reference
    ivals = knn[lo] + slopes[lo] * (dists - grid[lo])
    return ell * ell * sig2 * ivals
