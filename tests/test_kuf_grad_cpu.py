"""The fused Kuf backward (hgp_kuf_grid_grad / hgp_kuf_semi_mc_grad / hgp_kuf_semi_sqexp_grad) without
a GPU: the ABI and its argument checks (all made before any HIP call), the torch doubly-integrated
diagonal `knn_doubly_diag_ad` against the reference's formula and torch's gradcheck, the `_ad`
wrappers declining CPU tensors, and the register budget of the new fp32 kernels."""
import ctypes
import os
import re

import pytest
import torch

from test_kernel_resources_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_SYMS = ("hgp_kuf_grid_grad", "hgp_kuf_semi_mc_grad", "hgp_kuf_semi_sqexp_grad")
E_ARG, E_UNSUPPORTED = -1, -4
F32, SQEXP, GNEITING = 0, 0, 4


def test_header_declares_and_library_exports_the_grad_entries():
    from hipgp_amd import _lib
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    L = _lib.lib()
    for s in GRAD_SYMS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", src), f"include/hipgp.h does not declare {s}"
        assert hasattr(L, s), f"libhipgp.so does not export {s}"
        assert s in _lib.EXPORTS


class _Args:
    """A well-formed argument set (host addresses standing in for device ones: every call below
    must be refused before anything is launched), with one field replaced per case."""

    def __init__(self):
        self.buf = (ctypes.c_float * 64)()
        p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.m = (ctypes.c_int64 * 2)(4, 4)
        self.grids = (ctypes.c_void_p * 2)(p.value, p.value)
        self.kw = dict(dtype=F32, kind=SQEXP, ndim=2, x=p, nobs=2, npts=3, u=p, g=p, grad2=p)

    def call(self, L, name, **over):
        a = dict(self.kw, **over)
        if name == "hgp_kuf_grid_grad":
            return L.hgp_kuf_grid_grad(a["dtype"], a["kind"], a["ndim"], self.m, self.grids, a["x"], a["nobs"],
                                       1.0, 0.5, a["g"], a["grad2"], None)
        if name == "hgp_kuf_semi_mc_grad":
            return L.hgp_kuf_semi_mc_grad(a["dtype"], a["kind"], 1.0, a["ndim"], self.m, self.grids, a["x"],
                                          a["nobs"], 1.0, 0.5, a["npts"], a["u"], a["g"], a["grad2"], None)
        return L.hgp_kuf_semi_sqexp_grad(a["dtype"], a["ndim"], self.m, self.grids, a["x"], a["nobs"], 1.0, 0.5,
                                         a["g"], a["grad2"], None)


BAD = [("null_g", dict(g=None)), ("null_grad2", dict(grad2=None)), ("bad_dtype", dict(dtype=7)),
       ("bad_kind", dict(kind=9)), ("ndim0", dict(ndim=0)), ("negative_nobs", dict(nobs=-1)),
       ("npts0", dict(npts=0))]


# (the semi-sqexp entry has no kind, only the semi-mc entry has npts)
BAD_CALLS = [(n, t, o) for n in GRAD_SYMS for t, o in BAD
             if not (t == "bad_kind" and n == "hgp_kuf_semi_sqexp_grad")
             and not (t == "npts0" and n != "hgp_kuf_semi_mc_grad")]


@pytest.mark.parametrize("name,tag,over", BAD_CALLS, ids=[f"{c[0]}-{c[1]}" for c in BAD_CALLS])
def test_grad_entries_refuse_bad_arguments(name, tag, over):
    from hipgp_amd import _lib
    L = _lib.lib()
    rc = _Args().call(L, name, **over)
    assert rc == E_ARG, (name, tag, rc)
    assert len(L.hgp_last_error()) > 0


@pytest.mark.parametrize("name", GRAD_SYMS[:2])
def test_grad_entries_refuse_gneiting(name):
    from hipgp_amd import _lib
    L = _lib.lib()
    assert _Args().call(L, name, kind=GNEITING) == E_UNSUPPORTED
    assert b"Gneiting" in L.hgp_last_error()


def _table(N=9, dmax=4.0):
    g = torch.Generator().manual_seed(3)
    grid = torch.linspace(0, dmax, N, dtype=torch.float64)
    knn = torch.rand(N, generator=g, dtype=torch.float64)
    slopes = torch.cat([(knn[1:] - knn[:-1]) / (grid[1:] - grid[:-1]), torch.zeros(1, dtype=torch.float64)])
    return torch.stack([grid, knn, slopes])


def test_knn_doubly_diag_ad_is_the_reference_formula():
    from hipgp_amd.kuf import knn_doubly_diag_ad
    tab = _table()
    g = torch.Generator().manual_seed(4)
    x = torch.rand(11, 2, generator=g, dtype=torch.float64) * 1.6
    x[0] = 0.                                        # distance 0: index -1 wraps to the last entry
    sig2, ell = torch.tensor(1.3, dtype=torch.float64), torch.tensor(0.7, dtype=torch.float64)
    out = knn_doubly_diag_ad(tab, x, (sig2, ell))
    # `KernelDoublyDiagInterpolator.forward`, kernels.py:199-218, inline
    grid, knn, slopes = tab
    dists = torch.sqrt(torch.sum((x / ell) ** 2, dim=-1))
    lower_i = torch.sum(dists[:, None] > grid, dim=-1) - 1
    ref = ell * ell * sig2 * (knn[lower_i] + slopes[lower_i] * (dists - grid[lower_i]))
    assert lower_i[0] == -1
    assert torch.equal(out, ref)


def test_knn_doubly_diag_ad_gradcheck():
    from hipgp_amd.kuf import knn_doubly_diag_ad
    tab = _table()
    # |x| / ell = 0.25 + 0.5 k for ell = 0.7: mid-way between the knots (spacing 0.5), so the
    # finite differences of gradcheck stay on one linear piece
    r = (0.25 + 0.5 * torch.arange(6, dtype=torch.float64)) * 0.7
    th = torch.linspace(0.1, 1.4, 6, dtype=torch.float64)
    x = torch.stack([r * torch.cos(th), r * torch.sin(th)], dim=-1)
    sig2 = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    ell = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda s, e: knn_doubly_diag_ad(tab, x, (s, e)), (sig2, ell))


def test_ad_functions_decline_cpu_tensors():
    import ziggy.kernels as zk
    from hipgp_amd import kuf
    k = zk.SqExp(dtype=torch.float32)
    grids = [torch.linspace(-1, 1, 8)] * 2
    x = torch.full((3, 2), 0.4)
    ell = torch.tensor(0.3, requires_grad=True)
    assert kuf.kuf_grid_ad(k, grids, x, (1.0, ell)) is None
    assert kuf.kuf_semi_mc_ad(k, grids, x, (1.0, ell), 4) is None
    assert kuf.kuf_semi_sqexp_ad(k, grids, x, (1.0, ell)) is None


def test_new_fp32_grad_kernels_do_not_spill():
    ks = [k for k in _kernels() if re.search(r"hgp::k_kuf_\w*grad\w*<float>", k[0])]
    assert len(ks) >= 3, [k[0] for k in ks]
    bad = [f"{n} (spill {s}, scratch {p}, vgpr {v})" for n, s, p, v in ks if s or p]
    assert not bad, "fp32 Kuf backward kernels spilling to scratch:\n" + "\n".join(bad)
