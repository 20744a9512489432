"""The windowed line-integral Kuf products (hgp_kuf_semi_{mc,sqexp}_{matvec,rmatvec}_win behind
`kuf.LineWindowPlan` and the four `kuf.kuf_semi_*_win` functions) without a GPU: the ABI and its argument
checks (all made before any HIP call), the piece-count rule, the plan and the model knob declining where
they must, and the register budget of the new kernels."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from test_kernel_resources_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("hgp_kuf_semi_mc_matvec_win", "hgp_kuf_semi_sqexp_matvec_win", "hgp_kuf_semi_mc_rmatvec_win",
        "hgp_kuf_semi_sqexp_rmatvec_win")
E_ARG = -1
F32, SQEXP, GNEITING = 0, 0, 4


def test_header_declares_and_library_exports_the_line_window_entries():
    from hipgp_amd import _lib
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    L = _lib.lib()
    for s in SYMS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", src), f"include/hipgp.h does not declare {s}"
        assert hasattr(L, s), f"libhipgp.so does not export {s}"
        assert s in _lib.EXPORTS
        assert getattr(L, s).argtypes is not None, f"{s} is not bound"
    for cite in ("kernels.py:19-39", "kernels.py:80-85, 223-237"):
        assert cite in src[src.index("hgp_kuf_semi_mc_matvec over the WINDOW"):]


class _Args:
    """A well-formed argument set (host addresses standing in for device ones: every call below must
    return before anything is launched), with one field replaced per case."""

    def __init__(self):
        self.buf = (ctypes.c_float * 64)()
        self.pc = (ctypes.c_int * 64)()
        p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.m = (ctypes.c_int64 * 2)(4, 4)
        self.grids = (ctypes.c_void_p * 2)(p.value, p.value)
        self.kw = dict(dtype=F32, kind=SQEXP, ndim=2, x=p, nobs=2, rho=0.5, npts=4, u=p,
                       pieces=ctypes.cast(self.pc, ctypes.c_void_p), npieces=2, w=p, nw=2, out=p, m=self.m,
                       grids=self.grids)

    def call(self, L, name, **over):
        a = dict(self.kw, **over)
        head = [a["dtype"]] + ([a["kind"]] if "_mc_" in name else []) + \
               [a["ndim"], a["m"], a["grids"], a["x"], a["nobs"], 1.0, 0.5, a["rho"]]
        if "_mc_" in name:
            head += [a["npts"], a["u"]]
        return getattr(L, name)(*head, a["pieces"], a["npieces"], a["w"], a["nw"], a["out"], None)


BAD = [("null_x", dict(x=None)), ("null_w", dict(w=None)), ("null_out", dict(out=None)), ("null_m", dict(m=None)),
       ("null_grids", dict(grids=None)), ("bad_dtype", dict(dtype=7)), ("ndim0", dict(ndim=0)), ("ndim4", dict(ndim=4)),
       ("negative_nobs", dict(nobs=-1, npieces=-1)), ("negative_nw", dict(nw=-1)), ("negative_rho", dict(rho=-1e-3)),
       ("nan_rho", dict(rho=float("nan"))), ("inf_rho", dict(rho=float("inf"))),
       ("grid_size0", dict(m=(ctypes.c_int64 * 2)(4, 0))), ("null_grid", dict(grids=(ctypes.c_void_p * 2)(None, None))),
       ("null_pieces", dict(pieces=None)), ("short_pieces", dict(npieces=1)), ("long_pieces", dict(npieces=3))]
BAD_MC = [("bad_kind", dict(kind=9)), ("negative_kind", dict(kind=-1)), ("gneiting", dict(kind=GNEITING)),
          ("npts0", dict(npts=0)), ("npts1025", dict(npts=1025)), ("null_u", dict(u=None))]
BAD_CALLS = [(n, t, o) for n in SYMS for t, o in BAD + (BAD_MC if "_mc_" in n else [])]


@pytest.mark.parametrize("name,tag,over", BAD_CALLS, ids=[f"{c[0]}-{c[1]}" for c in BAD_CALLS])
def test_line_window_entries_refuse_bad_arguments_before_any_hip_call(name, tag, over):
    from hipgp_amd import _lib
    L = _lib.lib()
    a = _Args()
    for i in range(64):
        a.buf[i] = 3.0
    rc = a.call(L, name, **over)
    assert rc == E_ARG, (name, tag, rc)
    assert len(L.hgp_last_error()) > 0
    assert all(v == 3.0 for v in a.buf)


@pytest.mark.parametrize("name", SYMS)
def test_empty_line_window_products_return_zero_before_any_launch(name):
    from hipgp_amd import _lib
    a = _Args()
    for i in range(64):
        a.buf[i] = 3.0
    assert a.call(_lib.lib(), name, nw=0, w=None) == 0
    if "_matvec_" in name:
        assert a.call(_lib.lib(), name, nobs=0, npieces=0, x=None, out=None, pieces=None) == 0
    assert all(v == 3.0 for v in a.buf), "an empty product wrote something"


def test_the_piece_count_rule():
    from hipgp_amd import kuf
    rho = 0.05
    x = torch.tensor([[0., 0., 0.], [0.049, -0.01, 0.], [0.0499, 0.0499, -0.0499], [0.051, 0., 0.], [-0.7, 0.2, 0.1],
                      [1., 1., 1.], [100., 0., 0.], [float("nan"), 0.3, 0.], [float("inf"), 0., 0.]])
    p = kuf.line_pieces(x, rho)
    assert p.dtype == torch.int32 and p.is_contiguous() and tuple(p.shape) == (9,)
    assert p.tolist() == [1, 1, 1, 2, 14, 20, 64, 1, 64]
    g = torch.Generator().manual_seed(0)
    xr = torch.randn(1000, 2, generator=g) * 3
    for r in (1e-6, 0.05, 10., 0.):
        pr = kuf.line_pieces(xr, r)
        assert int(pr.min()) >= 1 and int(pr.max()) <= kuf.LINE_MAX_PIECES == 64
        if r > 0:       # about one piece per rho of the largest |x_a|: never a piece longer than rho under the cap
            free = pr < 64
            assert bool((xr.abs().amax(dim=1)[free].double() / pr[free] <= r).all())
    assert kuf.line_pieces(torch.zeros(0, 3), 0.1).shape == (0,)


def test_line_window_plan_declines_cpu_tensors_and_unsupported_kernels():
    import ziggy.kernels as zk
    from hipgp_amd import kuf
    k = zk.SqExp(dtype=torch.float32)
    grids = [torch.linspace(0, 1, 8)] * 2
    x = torch.full((3, 2), 0.4)
    assert kuf.LineWindowPlan.make(k, grids, x, (1.0, 0.3), 1e-6) is None            # a CPU tensor
    with pytest.raises(ValueError, match="windowed line-integral Kuf products do not apply"):
        kuf.LineWindowPlan(k, grids, x, (1.0, 0.3), 1e-6)
    # what `support_radius` declines is declined whatever the device: Gneiting, a vector ell, tol outside (0, 1)
    assert kuf.LineWindowPlan.make(zk.Gneiting(dtype=torch.float32), grids, x, (1.0, 0.3), 1e-6) is None
    assert kuf.LineWindowPlan.make(k, grids, x, (1.0, torch.tensor([0.3, 0.2])), 1e-6) is None
    for tol in (0.0, 1.0, -1e-3, 2.0, None):
        assert kuf.LineWindowPlan.make(k, grids, x, (1.0, 0.3), tol) is None
        assert kuf.support_radius(k, (1.0, 0.3), tol) is None
    assert kuf.support_radius(zk.Gneiting(dtype=torch.float32), (1.0, 0.3), 1e-6) is None
    assert kuf.support_radius(k, (1.0, torch.tensor([0.3, 0.2])), 1e-6) is None
    assert list(inspect.signature(kuf.LineWindowPlan.__init__).parameters) == ["self", "kernel", "xgrids", "x", "params",
                                                                              "tol", "rho"]
    assert list(inspect.signature(kuf.kuf_semi_mc_matvec_win).parameters) == ["plan", "W", "npts", "u"]
    assert list(inspect.signature(kuf.kuf_semi_mc_rmatvec_win).parameters) == ["plan", "C", "npts", "u"]
    assert list(inspect.signature(kuf.kuf_semi_sqexp_matvec_win).parameters) == ["plan", "W"]
    assert list(inspect.signature(kuf.kuf_semi_sqexp_rmatvec_win).parameters) == ["plan", "C"]


def test_the_line_knob_defaults_off_and_a_cpu_model_takes_the_dense_route(monkeypatch):
    from test_kuf_matvec_cpu import SolvingKmm, _model, _oracle, _points
    monkeypatch.delenv("HGP_KUF_LINE_SUPPORT_TOL", raising=False)
    monkeypatch.delenv("HGP_KUF_SUPPORT_TOL", raising=False)
    mod = _model()
    assert mod.kuf_line_support_tol is None and mod._kuf_line_support_tol() is None and mod._lwin is None
    monkeypatch.setenv("HGP_KUF_LINE_SUPPORT_TOL", "1e-5")
    assert mod._kuf_line_support_tol() == 1e-5
    mod.kuf_line_support_tol = 1e-7                # the attribute goes before the environment
    assert mod._kuf_line_support_tol() == 1e-7
    for bad in (0.0, 1.0, -1.0):
        mod.kuf_line_support_tol = bad
        with pytest.raises(ValueError, match="support tolerance"):
            mod._kuf_line_support_tol()
    monkeypatch.delenv("HGP_KUF_LINE_SUPPORT_TOL")
    mod.kuf_line_support_tol = None
    Kmm = SolvingKmm(_oracle())
    x = _points()
    kw = dict(integrated_obs=True, semi_integrated_estimator="mc-biased", semi_integrated_samps=5,
              mc_offset=torch.tensor([0.3], dtype=torch.float64), Kmm=Kmm)      # the stand-in's kernel is a Matern
    # the line-integral grams need the device (the Knn_diag table kernel); here a fixed smooth stand-in for Knm
    A = torch.linspace(-2, 2, 2 * mod.M, dtype=torch.float64).reshape(2, mod.M)
    grams = []
    mod._make_grams = lambda xb, **k: grams.append(k["integrated_obs"]) or (torch.cos(xb.double() @ A) * .1,)
    dense = (mod.predict_mean(x, **kw),
             mod.predict_draws(x, 2, eps=torch.ones(2, mod.Mprime, dtype=torch.float64), **kw))
    seen = []

    def plan_seen(x, params, real=mod._line_window_plan):
        seen.append(mod._lwin["tol"])
        return real(x, params)
    mod._line_window_plan = plan_seen
    mod.kuf_line_support_tol = 1e-6                # the line knob alone: point observations are not windowed
    assert mod._kuf_support_tol() is None
    again = (mod.predict_mean(x, **kw),
             mod.predict_draws(x, 2, eps=torch.ones(2, mod.Mprime, dtype=torch.float64), **kw))
    assert seen and set(seen) == {1e-6}, "the knob did not reach the products"
    assert grams and all(grams), "the dense route was not the one taken"
    for a, b in zip(dense, again):
        assert torch.equal(a, b), "a CPU stand-in with the line knob set must return what it returns today"
    assert mod._lwin is None
    n = len(seen)
    mod.predict_mean(x, Kmm=Kmm)                   # point observations never ask for a line plan
    assert len(seen) == n
    # the point knob still refuses line integrals, in the same words
    mod.kuf_support_tol = 1e-6
    with pytest.raises(NotImplementedError, match="tube"):
        mod.predict_mean(x, **kw)


def test_line_window_kernels_do_not_spill():
    ks = [k for k in _kernels() if re.search(r"hgp::k_kuf_line_win_\w+<", k[0])]
    mv = [k for k in ks if "k_kuf_line_win_mv<" in k[0]]
    rmv = [k for k in ks if "k_kuf_line_win_rmv<" in k[0]]
    assert len(mv) == 2 * 2 * 3 and len(rmv) == 2 * 2 * 3 * 3, (len(mv), len(rmv))
    bad = [f"{n} (spill {s}, scratch {p}, vgpr {v})" for n, s, p, v in ks if s or p]
    assert not bad, bad
