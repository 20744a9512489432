"""The case table of the k_sep_pass sweep (tests/sep_cases.py) stays complete, without a device:
every half-length that has a kernel is reached on either axis in either dtype, every stored column
is accepted as a product by the host detection (hgp_separable_detect) and none would be clamped."""
import ctypes

import numpy as np
import pytest

import sep_cases as sc
from oracle import ziggy_oracle as zo

ACCEPT = 4.0          # HGP_SEP_ACCEPT (hgp_sep_host.hpp)
NP_DT = {"f32": np.float32, "f64": np.float64}
EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
ALL = [(k, d) for k in ("f32", "f64") for d in sc.CASES[k]]
IDS = [f"{k}_{sc.case_id(d)}" for k, d in ALL]


def test_half_lengths():
    assert [sc.half_len(m) for m in (2, 3, 4, 5, 8, 9, 16, 17, 4096, 4097, 8192)] == \
        [2, 4, 4, 8, 8, 16, 16, 32, 4096, 8192, 8192]


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_every_fitting_length_on_either_axis(kind):
    assert sc.ALL_H == tuple(2 ** k for k in range(1, 14))
    want = sc.ALL_H if kind == "f32" else sc.ALL_H[:-1]          # 13 in fp32, the 12 up to 4096 in fp64
    assert len(want) == (13 if kind == "f32" else 12) and sc.FIT_H[kind] == want
    for ax in (0, 1):
        got = {sc.half_lens(d)[ax] for d in sc.CASES[kind]}
        assert got == set(want), (kind, ax, sorted(set(want) - got), sorted(got - set(want)))
    # lines exactly H long; under every block shape C, in either pass role, a row count that leaves
    # the last block of 2C rows partial
    assert {8192, 4096, 2048, 1024, 512, 16, 8, 4} <= {m for d in sc.CASES["f32"] for m in d if sc.half_len(m) == m}
    for ax in (0, 1):
        partial = {}
        for d in sc.CASES[kind]:
            C = sc.PAIRS[kind][sc.half_lens(d)[ax]]
            partial[C] = partial.get(C, False) or d[1 - ax] % (2 * C) != 0
        assert all(partial.values()) and set(partial) == set(sc.PAIRS[kind].values()), (kind, ax, partial)


def test_case_sets():
    assert len(sc.SHAPES) == len(set(sc.SHAPES)) and all(d[::-1] in sc.SHAPES for d in sc.SHAPES)
    assert sc.CASES["f32"] == sc.SHAPES
    assert sc.CASES["f64"] == [d for d in sc.SHAPES if max(d) <= 4096]
    for d in sc.FALLBACK_F64:
        assert d in sc.SHAPES and d not in sc.CASES["f64"] and 8192 in sc.half_lens(d)
    assert sorted(sc.FALLBACK_F64) == sorted(d for d in sc.SHAPES if max(d) > 4096)


@pytest.mark.parametrize("kind,dims", ALL, ids=IDS)
def test_stored_column_is_an_unclamped_product(kind, dims):
    from hipgp_amd import _lib
    eps = EPS[kind]
    col = np.ascontiguousarray(sc.column(dims, NP_DT[kind]))
    out = (ctypes.c_double * 4)()
    _lib.check(_lib.lib().hgp_separable_detect(_lib.HGP_F32 if kind == "f32" else _lib.HGP_F64, dims[0], dims[1],
                                               col.ctypes.data_as(ctypes.c_void_p), 0.0, out, None, None))
    ok, sigma, resid = bool(out[0]), out[1], out[2]
    # the fp64 oracle's raw embedding spectrum (clamp_min = -inf: D is Re FFT(C) itself)
    dmin = float(zo.ToeplitzOracle(col.astype(np.float64), dims, clamp_min=-np.inf).D.min())
    print(f"{kind} {dims} H={sc.half_lens(dims)}: residual {resid / eps:.2f} units, sigma - 1e-3 = "
          f"{(sigma - sc.JITTER) / (eps * np.abs(col).max()):.2f} units, min raw eigenvalue {dmin:.3e}")
    assert ok and resid <= ACCEPT * eps, resid / eps
    assert abs(sigma - sc.JITTER) <= 4 * eps * np.abs(col).max(), sigma
    assert dmin >= 1e-6, dmin


@pytest.mark.parametrize("dims", sc.FALLBACK_F64, ids=[sc.case_id(d) for d in sc.FALLBACK_F64])
def test_fallback_columns_are_products_too(dims):
    """the fp64 fallback cases are refused for their length alone: the column itself is a product"""
    from hipgp_amd import _lib
    col = np.ascontiguousarray(sc.column(dims, np.float64))
    out = (ctypes.c_double * 4)()
    _lib.check(_lib.lib().hgp_separable_detect(_lib.HGP_F64, dims[0], dims[1], col.ctypes.data_as(ctypes.c_void_p),
                                               0.0, out, None, None))
    assert out[0] == 1 and out[2] <= ACCEPT * EPS["f64"]
    assert float(zo.ToeplitzOracle(col, dims, clamp_min=-np.inf).D.min()) >= 1e-6
