"""Shared by tests/test_rff_line_{cpu,gpu}.py: the rows and features at which the line-integral
feature product can go wrong, and a quadrature of the line integral that owes nothing to its
closed form."""
import numpy as np
import torch

TWO_PI = 2 * np.pi
# omega . x of the special features at the special row, in revolutions: next to 0 (the series), on
# each side of the kernel's threshold 0.25 with either sign (fract of a negative half), and large
SPECIAL_T = (1e-9, -1e-3, 0.2499, 0.2501, -0.2499, -0.2501, 500.3)
NSPECIAL_F = len(SPECIAL_T) + 1
NSPECIAL_X = 2
PANELS, NODES = 128, 48


def special_row(ndim):
    """x = (a, a, c): omega = (1, -1, 0) has omega . x = 0 exactly."""
    return torch.tensor([0.625, 0.625, -0.375][:ndim], dtype=torch.float64)


def special_features(ndim):
    """(omega (NSPECIAL_F, ndim), in radians): first the feature with omega . x_s = 0 exactly
    (omega = (1, -1, 0); omega = 0 in one dimension), then omega = 2 pi t x_s / |x_s|^2 for t in
    SPECIAL_T, so that omega . x_s = t revolutions."""
    xs = special_row(ndim)
    zero = torch.tensor([1., -1., 0.][:ndim], dtype=torch.float64) if ndim > 1 else torch.zeros(1, dtype=torch.float64)
    rows = [zero] + [TWO_PI * t * xs / float(xs @ xs) for t in SPECIAL_T]
    return torch.stack(rows)


def with_specials(x, omega, ndim):
    """Copies of x (nobs, ndim) and omega (nfeat, ndim) (fp64, CPU) whose LAST rows are replaced by
    the special ones, as many as fit: rows x_s then x = 0 (x_s alone when nobs = 1, so that the
    result is not all zero), features in the order of `special_features`."""
    x, omega = x.clone(), omega.clone()
    sx = torch.stack([special_row(ndim), torch.zeros(ndim, dtype=torch.float64)])[:min(NSPECIAL_X, x.shape[0])]
    if len(sx):
        x[x.shape[0] - len(sx):] = sx.to(x.dtype)
    sf = special_features(ndim)[:min(NSPECIAL_F, omega.shape[0])]
    if len(sf):
        omega[omega.shape[0] - len(sf):] = sf
    return x, omega


def quad_line_features(omega, phase, x):
    """(nobs, nfeat) |x_i| int_0^1 cos(a omega_f . x_i + phase_f) da by composite Gauss-Legendre
    quadrature in NumPy fp64: PANELS = 128 equal panels of NODES = 48 nodes.  On a panel the phase
    a T runs over half-width kappa = |T| / 256 <= 24.6 rad for |T| <= 1000 revolutions, and an
    n-node rule integrates exp(i kappa s) on [-1, 1] with an error that falls faster than
    (e kappa / 4 n)^(2 n) once n > kappa: (0.35)^96 here, far below fp64 rounding."""
    omega, phase, x = (np.asarray(t, dtype=np.float64) for t in (omega, phase, x))
    T = x @ omega.T
    s, w = np.polynomial.legendre.leggauss(NODES)
    acc = np.zeros_like(T)
    for p in range(PANELS):
        a = (p + (s + 1) / 2) / PANELS
        acc += np.einsum("q,qnf->nf", w / (2 * PANELS), np.cos(a[:, None, None] * T[None] + phase[None, None, :]))
    return np.sqrt(np.sum(x * x, axis=1))[:, None] * acc
