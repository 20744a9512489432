"""Case table of the k_sep_pass sweep: every half-length H = 2 ... 8192 that
hgp_sep_dispatch.hpp instantiates, on axis 0 and on axis 1, in both dtypes.  No device.

Column: per axis of m points the factor t[i] = exp(-(i / w)^2 / 2) with a width of
w = min(20, max(0.5, (m - 1) / 8)) GRID STEPS (so a 2-point axis still convolves; with one shared
length scale on linspace(-1, 1, m) the short axis of a 4200 x 2 grid is the identity), the column
c = t0 t1^T + 1e-3 on c[0][0], computed in fp64 and stored in the plan dtype.  Its smallest raw
circulant eigenvalue is >= 9.98e-4 at every shape below (nothing is clamped at 1e-6) and the fp32
column's product-form residual <= 1.32 rounding units of the 4 accepted
(tests/test_sep_sweep_cpu.py asserts both)."""
import numpy as np

JITTER = 1e-3

# each shape is used as written and transposed: H = 8192 ... 2 on axis 0 and on axis 1, lines
# exactly H long (m = 8192, 4096, 2048, 1024, 512, 16, 8, 4), a partial last row block under every C
_BASE = [(4200, 2), (2100, 3), (1100, 5), (600, 11), (300, 19), (150, 37), (83, 83),
         (8192, 7), (4096, 3), (2048, 9), (1024, 17), (512, 6), (16, 16), (8, 4),
         # a 2-point axis (H = 2) beside one that fp64 holds: the only other one is 4200 x 2, which
         # fp64 does not run as a product (below); 301 rows are three blocks of 2C = 128, the last odd
         (301, 2)]


def _both(shapes):
    out = []
    for s in shapes:
        for d in (s, s[::-1]):
            if d not in out:
                out.append(d)
    return out


SHAPES = _both(_BASE)
ALL_H = tuple(2 ** k for k in range(1, 14))              # 2 ... 8192

# row pairs per block C of k_sep_pass<T, H> (SepCfg<T, H>::C, hgp_sep.hpp); fp64 H = 8192 does not
# fit one CU's LDS (sep_candidate refuses the plan: the general passes)
PAIRS = {"f32": {2: 64, 4: 64, 8: 64, 16: 64, 32: 32, 64: 16, 128: 8, 256: 8, 512: 8, 1024: 8, 2048: 8,
                 4096: 4, 8192: 1},
         "f64": {2: 64, 4: 64, 8: 64, 16: 32, 32: 16, 64: 8, 128: 8, 256: 8, 512: 8, 1024: 8, 2048: 4, 4096: 1}}
FIT_H = {k: tuple(sorted(v)) for k, v in PAIRS.items()}

CASES = {"f32": list(SHAPES), "f64": [d for d in SHAPES if max(d) <= 4096]}
# fp64 plans with an H = 8192 axis: no k_sep_pass, the general three passes
FALLBACK_F64 = [(4200, 2), (2, 4200), (8192, 7), (7, 8192)]


def half_len(m):
    """H = next_pow2(2 m - 1) / 2: half the K op's padded line length of an m-point axis"""
    L = 1
    while L < 2 * m - 1:
        L *= 2
    return L // 2


def half_lens(dims):
    return tuple(half_len(m) for m in dims)


def width(m):
    return min(20.0, max(0.5, (m - 1) / 8.0))


def factor(m):
    return np.exp(-0.5 * (np.arange(m, dtype=np.float64) / width(m)) ** 2)


def column(dims, dtype=np.float64):
    """the (m0 * m1,) column in fp64, rounded once to `dtype`"""
    c = np.outer(factor(dims[0]), factor(dims[1]))
    c[0, 0] += JITTER
    return c.reshape(-1).astype(dtype)


def case_id(dims):
    return f"{dims[0]}x{dims[1]}"
