"""Tap radius of the banded product-form passes without a device: hgp_band_radius, the
host rule hgp_plan_set_column applies to the two factor columns.

The rule: the smallest r with 2 sum_{j > r} |t[j]| <= 2^-25 (|t[0]| + 2 sum_{j >= 1} |t[j]|)."""
import ctypes

import numpy as np
import pytest


def _radius(t):
    from hipgp_amd import _lib
    t = np.ascontiguousarray(t, dtype=np.float64)
    r = ctypes.c_int64(-1)
    _lib.check(_lib.lib().hgp_band_radius(t.size, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(r)))
    return r.value


def _rule(t):
    """the rule as stated, in plain NumPy"""
    a = np.abs(np.asarray(t, dtype=np.float64))
    total = a[0] + 2 * a[1:].sum()
    for r in range(a.size):
        if 2 * a[r + 1:].sum() <= 2.0 ** -25 * total:
            return r
    return a.size - 1


def _sqexp(m, ell, lo=-1.0, hi=1.0):
    """first column of the 1-D SqExp(1, ell) Toeplitz matrix on m points of [lo, hi], as fp32 stores it"""
    g = np.linspace(lo, hi, m)
    return np.exp(-0.5 * ((g - g[0]) / ell) ** 2).astype(np.float32).astype(np.float64)


def test_benchmark_factor_has_radius_28():
    t = _sqexp(1024, .01)
    assert np.flatnonzero(t)[-1] == 73          # the last tap fp32 holds at all
    assert _radius(t) == _rule(t) == 28


def test_radius_grows_with_the_length_scale_and_the_grid():
    by_ell = [_radius(_sqexp(1024, ell)) for ell in (.005, .01, .02, .04, .08)]
    assert all(a < b for a, b in zip(by_ell, by_ell[1:])), by_ell
    by_grid = [_radius(_sqexp(m, .01)) for m in (256, 512, 1024, 2048, 4096)]
    assert all(a < b for a, b in zip(by_grid, by_grid[1:])), by_grid
    for m, ell in ((1024, .005), (1024, .08), (256, .01), (4096, .01)):
        assert _radius(_sqexp(m, ell)) == _rule(_sqexp(m, ell))


def test_every_tap_significant_keeps_them_all():
    for m in (2, 17, 64):
        assert _radius(np.ones(m)) == m - 1
        assert _radius(1.0 / (1 + np.arange(m))) == m - 1


def test_single_tap_has_radius_zero():
    for m in (1, 2, 33):
        t = np.zeros(m)
        t[0] = 2.5
        assert _radius(t) == 0
    # taps that together stay below half a rounding unit of the row sum do not count
    t = np.zeros(9)
    t[0] = 1
    t[1:] = 2.0 ** -30
    assert _radius(t) == 0


def test_bad_arguments_are_refused():
    from hipgp_amd import _lib
    r = ctypes.c_int64(0)
    t = (ctypes.c_double * 4)(1, 0, 0, 0)
    assert _lib.lib().hgp_band_radius(0, t, ctypes.byref(r)) != 0
    assert _lib.lib().hgp_band_radius(4, None, ctypes.byref(r)) != 0
    assert _lib.lib().hgp_band_radius(4, t, None) != 0
