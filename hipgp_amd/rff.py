"""Random Fourier features of the stationary kernels, and products with them that never store them.

A draw of the prior at any points is f(x) = sqrt(2 sig2 / F) sum_f w_f cos(omega_f . x + b_f) with
omega from the kernel's spectral density, b uniform on [0, 2 pi) and w standard normal
(`spectral_features` draws (omega, b)); its covariance is k(x, y) up to an O(F^-1/2) error.
`rff_matvec` (hgp_rff_matvec) evaluates scale * W cos(...) at explicit points or on the mesh of the
inducing grids for a few weight rows W: the (points, F) feature matrix, 16 GB at 1024^2 mesh points
and F = 4096, is never built.  `ToeplitzInducingGP.predict_samples` is the caller.

The line integral of the same draw from the origin to x, |x| int_0^1 f(a x) da, has a closed form per
feature, |x| cos(b + T / 2) sinc(T / 2) with T = omega . x (`line_features` in torch);
`rff_line_matvec` (hgp_rff_line_matvec) is the product with those, again without storing them, and
`ToeplitzInducingGP.predict_line_samples` its caller.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import check, lib
from .kuf import _ell_arg, _grid_ptrs, _takes_ard

TWO_PI = 2 * math.pi


def spectral_features(kernel, params, ndim, nfeat, generator=None, device=None, dtype=torch.float64):
    """(omega (nfeat, ndim), phase (nfeat)) in radians for kernel(params): omega from the spectral
    density of the kernel as `hipgp_amd/ziggy/kernels.py` parametrises it, phase ~ U[0, 2 pi).

    SqExp: omega ~ N(0, I / ell^2); declared with ard=True and given one ell per axis (a 1-D tensor or sequence of ndim values,
    `kernels.py:73-79`) omega_a ~ N(0, 1 / ell_a^2), the same normal draws divided axis by axis.  Matern nu in {1/2, 3/2, 5/2}: the multivariate t with 2 nu
    degrees of freedom, omega = z / ell * sqrt(2 nu / chi2_{2 nu}) with z ~ N(0, I) (the chi-square
    as the sum of 2 nu squared normals).  Drawn in fp64 with `generator` (on its device; the
    default generator of the CPU when None), then moved to `device` and rounded to `dtype`.
    Gneiting (no closed-form sampler of its spectrum), a vector ell with Matern and any other
    non-scalar ell raise."""
    from hipgp_amd.ziggy import kernels as zk
    name = type(kernel).__name__
    if not isinstance(kernel, (zk.SqExp, zk.Matern)):
        raise NotImplementedError(f"spectral_features: no spectral sampler for the {name} kernel "
                                  "(SqExp and Matern nu in {1/2, 3/2, 5/2} only)")
    ndim, nfeat = int(ndim), int(nfeat)
    ell = _ell_arg(params[1], ndim)
    if ell is None or (isinstance(ell, list) and not _takes_ard(kernel)):
        raise NotImplementedError(f"spectral_features: the {name} kernel needs a scalar ell (SqExp(ard=True) also "
                                  f"takes one ell per axis, {ndim} values)")
    gdev = generator.device if generator is not None else torch.device("cpu")
    kw = dict(generator=generator, dtype=torch.float64, device=gdev)
    omega = torch.randn((nfeat, ndim), **kw)
    omega = omega / (torch.tensor(ell, dtype=torch.float64, device=gdev) if isinstance(ell, list) else ell)
    if isinstance(kernel, zk.Matern):
        dof = int(round(2 * kernel.nu))
        chi2 = torch.sum(torch.randn((nfeat, dof), **kw) ** 2, dim=1, keepdim=True)
        omega = omega * torch.sqrt(dof / chi2)
    phase = torch.rand((nfeat,), **kw) * TWO_PI
    device = gdev if device is None else device
    return omega.to(device=device, dtype=dtype), phase.to(device=device, dtype=dtype)


def rff_matvec(omega, phase, W, x=None, xgrids=None, scale=1.0, transposed=False, out=None, beta=0.0, nsplit=0):
    """scale * cos(p omega^T + phase) W^T without the (points, nfeat) features (hgp_rff_matvec).

    The points p are the rows of x (nobs, ndim), or, with xgrids, the C-order mesh of the grids
    (coordinates read from the grids; no (M, ndim) tensor is built).  omega (nfeat, ndim) and phase
    (nfeat) are in radians; they are divided by 2 pi in fp64 here and rounded to the dtype, the form
    the kernel takes.  W: (nw, nfeat) or (nfeat,).  The result is (npoints, nw), or (nw, npoints)
    with transposed=True; with `out` and beta it is accumulated in place, out = beta * out + product
    (beta = 0: out is only written).  None for CPU tensors (the caller takes a torch route)."""
    if (x is None) == (xgrids is None):
        raise TypeError("rff_matvec takes either x or xgrids")
    ref = x if x is not None else xgrids[0]
    if ref.device.type != "cuda" or ref.dtype not in (torch.float32, torch.float64):
        return None
    dev, dt = ref.device, ref.dtype
    W = W.detach()
    if W.dim() == 1:
        W = W[None, :]
    nfeat = omega.shape[0]
    if W.dim() != 2 or W.shape[1] != nfeat or phase.numel() != nfeat:
        raise ValueError(f"W must be (nw, nfeat) and phase (nfeat,) with nfeat = {nfeat}, got {tuple(W.shape)} "
                         f"and {tuple(phase.shape)}")
    Wc = W.to(device=dev, dtype=dt).contiguous()
    om = (omega.detach().to(device=dev, dtype=torch.float64) / TWO_PI).to(dt).contiguous()
    ph = (phase.detach().to(device=dev, dtype=torch.float64).reshape(-1) / TWO_PI).to(dt).contiguous()
    if x is not None:
        if x.dim() != 2 or x.shape[1] != om.shape[1] or not 1 <= x.shape[1] <= 3:
            raise ValueError(f"x must be (nobs, ndim) with ndim = {om.shape[1]} in 1..3, got {tuple(x.shape)}")
        xc = x.detach().contiguous()
        ndim, npoints = x.shape[1], x.shape[0]
        m, ptrs, xp = None, None, ctypes.c_void_p(xc.data_ptr())
    else:
        if len(xgrids) != om.shape[1] or not 1 <= len(xgrids) <= 3:
            raise ValueError(f"{len(xgrids)} grids for features of {om.shape[1]} dimensions (1..3)")
        grids = [g.to(device=dev, dtype=dt).contiguous() for g in xgrids]
        ndim, npoints = len(grids), 1
        for g in grids:
            npoints *= g.numel()
        (m, ptrs), xp = _grid_ptrs(grids), None
    shape = (Wc.shape[0], npoints) if transposed else (npoints, Wc.shape[0])
    if out is None:
        if beta != 0:
            raise ValueError("beta != 0 needs the tensor to accumulate into (out)")
        out = torch.empty(shape, dtype=dt, device=dev)
    elif tuple(out.shape) != shape or out.dtype != dt or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {shape} tensor of {dt} on {dev}")
    if npoints == 0 or Wc.shape[0] == 0:
        return out
    check(lib().hgp_rff_matvec(_lib.dtype_code(dt), ndim, m, ptrs, xp, npoints if x is not None else 0,
                               ctypes.c_void_p(om.data_ptr()), ctypes.c_void_p(ph.data_ptr()), nfeat,
                               ctypes.c_void_p(Wc.data_ptr()), Wc.shape[0], float(scale), int(bool(transposed)),
                               float(beta), int(nsplit), ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr(dev)))
    return out


def line_features(omega, phase, x):
    """(nobs, nfeat) line integrals |x_i| int_0^1 cos(a omega_f . x_i + phase_f) da of the features
    along the segments from the origin to the rows of x, in torch and in the dtype of x: the closed
    form |x| cos(phase + T / 2) sinc(T / 2), T = omega . x in radians (`torch.sinc(z)` is
    sin(pi z) / (pi z), so z = T / 2 pi).  What `rff_line_matvec` sums without storing it."""
    T = x.matmul(omega.t())
    return torch.linalg.vector_norm(x, dim=1)[:, None] * torch.cos(phase + T / 2) * torch.sinc(T / TWO_PI)


def rff_line_matvec(omega, phase, W, x, scale=1.0, transposed=False, out=None, beta=0.0, nsplit=0):
    """scale * L W^T with L[i, f] = |x_i| int_0^1 cos(a omega_f . x_i + phase_f) da, the line integrals
    of the features of `rff_matvec` along the segments from the origin to the rows of x (nobs, ndim),
    without the (nobs, nfeat) matrix L (hgp_rff_line_matvec; closed form |x| cos(phase + T / 2)
    sinc(T / 2), T = omega . x).  omega, phase, W, scale, transposed, out, beta and nsplit as
    `rff_matvec` takes them; explicit rows only.  None for CPU tensors (the caller takes a torch
    route, `line_features`)."""
    if x.device.type != "cuda" or x.dtype not in (torch.float32, torch.float64):
        return None
    dev, dt = x.device, x.dtype
    W = W.detach()
    if W.dim() == 1:
        W = W[None, :]
    nfeat = omega.shape[0]
    if W.dim() != 2 or W.shape[1] != nfeat or phase.numel() != nfeat:
        raise ValueError(f"W must be (nw, nfeat) and phase (nfeat,) with nfeat = {nfeat}, got {tuple(W.shape)} "
                         f"and {tuple(phase.shape)}")
    Wc = W.to(device=dev, dtype=dt).contiguous()
    om = (omega.detach().to(device=dev, dtype=torch.float64) / TWO_PI).to(dt).contiguous()
    ph = (phase.detach().to(device=dev, dtype=torch.float64).reshape(-1) / TWO_PI).to(dt).contiguous()
    if x.dim() != 2 or x.shape[1] != om.shape[1] or not 1 <= x.shape[1] <= 3:
        raise ValueError(f"x must be (nobs, ndim) with ndim = {om.shape[1]} in 1..3, got {tuple(x.shape)}")
    xc = x.detach().contiguous()
    nobs = x.shape[0]
    shape = (Wc.shape[0], nobs) if transposed else (nobs, Wc.shape[0])
    if out is None:
        if beta != 0:
            raise ValueError("beta != 0 needs the tensor to accumulate into (out)")
        out = torch.empty(shape, dtype=dt, device=dev)
    elif tuple(out.shape) != shape or out.dtype != dt or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {shape} tensor of {dt} on {dev}")
    if nobs == 0 or Wc.shape[0] == 0:
        return out
    check(lib().hgp_rff_line_matvec(_lib.dtype_code(dt), x.shape[1], ctypes.c_void_p(xc.data_ptr()), nobs,
                                    ctypes.c_void_p(om.data_ptr()), ctypes.c_void_p(ph.data_ptr()), nfeat,
                                    ctypes.c_void_p(Wc.data_ptr()), Wc.shape[0], float(scale), int(bool(transposed)),
                                    float(beta), int(nsplit), ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr(dev)))
    return out
