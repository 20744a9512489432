"""SqExp with one length scale per axis (`kernels.py:73-79` with a vector ell; the hgp_kuf_grid*_ard
entries behind `kuf.kuf_grid`, the two products, their windowed twins and `kuf.kuf_grid_ad`) without a GPU:
the per-axis truncation rule of `kuf.support_radius`, the model's construction with a list `ell_init`,
the argument checks of the six entries (all made before any HIP call), and the per-axis scaling of the
Fourier-feature frequencies."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARD_SYMS = ("hgp_kuf_grid_ard", "hgp_kuf_grid_matvec_ard", "hgp_kuf_grid_rmatvec_ard",
            "hgp_kuf_grid_matvec_win_ard", "hgp_kuf_grid_rmatvec_win_ard", "hgp_kuf_grid_grad_ard")
E_ARG = -1
F32, SQEXP, MATERN32, GNEITING = 0, 0, 2, 4
TOLS = (1e-3, 2.0 ** -24, 1e-12)


def _sqexp(dtype=torch.float64):
    import hipgp_amd.ziggy.kernels as zk
    return zk.SqExp(dtype=dtype, ard=True)     # declared per-axis: a plain SqExp declines a vector ell


def _matern(dtype=torch.float64):
    import hipgp_amd.ziggy.kernels as zk
    return zk.Matern(nu=1.5, dtype=dtype)


# ---- support_radius ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [(0.01, 0.02), (0.3, 0.12, 0.7), (0.05,)], ids=lambda e: "x".join(map(str, e)))
@pytest.mark.parametrize("tol", TOLS, ids=lambda t: f"{t:.1e}")
def test_support_radius_per_axis(tol, ell):
    from hipgp_amd import kuf
    k = _sqexp()
    for form in (list(ell), tuple(ell), torch.tensor(ell, dtype=torch.float64)):
        if torch.is_tensor(form) and form.numel() == 1:
            continue                                   # a tensor of one element is a scalar ell: a float comes back
        rho = kuf.support_radius(k, (2.5, form), tol)
        assert isinstance(rho, list) and len(rho) == len(ell)
        for a, (r, e) in enumerate(zip(rho, ell)):
            closed = e * math.sqrt(2 * math.log(1 / tol))
            at = math.exp(-((r / e) ** 2) / 2)          # axis a's factor alone, the fp64 formula
            print(f"tol={tol:.3e} axis {a} ell={e}: rho = {r:.17g}, closed form {closed:.17g}, factor at rho {at:.6e}")
            assert abs(r - closed) <= 1e-15 * closed
            assert at <= tol
            assert math.exp(-((0.999 * r / e) ** 2) / 2) > tol
            assert r == kuf.support_radius(k, (2.5, e), tol), "each axis follows the scalar rule"


def test_support_radius_scalar_unchanged_and_declines():
    from hipgp_amd import kuf
    k = _sqexp()
    for tol in TOLS:
        rho = kuf.support_radius(k, (1.0, 0.3), tol)
        assert isinstance(rho, float)
        want = 0.3 * math.sqrt(2 * math.log(1 / tol))
        for _ in range(4):
            if math.exp(-((want / 0.3) ** 2) / 2) <= tol:
                break
            want = math.nextafter(want, math.inf)
        assert rho == want
        assert kuf.support_radius(k, (1.0, torch.tensor(0.3, dtype=torch.float64)), tol) == rho
    # a vector ell: a SqExp declared with ard=True alone, positive finite entries, 1-D
    import hipgp_amd.ziggy.kernels as zk
    plain = zk.SqExp(dtype=torch.float64)
    assert plain.ard is False and k.ard is True
    assert kuf.support_radius(plain, (1.0, [0.2, 0.3]), 1e-6) is None
    assert kuf.support_radius(plain, (1.0, torch.tensor([0.2, 0.3])), 1e-6) is None
    assert kuf.support_radius(plain, (1.0, 0.3), 1e-6) == kuf.support_radius(k, (1.0, 0.3), 1e-6)
    assert kuf.support_radius(_matern(), (1.0, [0.2, 0.3]), 1e-6) is None
    assert kuf.support_radius(k, (1.0, [0.2, -0.3]), 1e-6) is None
    assert kuf.support_radius(k, (1.0, [0.2, float("nan")]), 1e-6) is None
    assert kuf.support_radius(k, (1.0, torch.tensor([[0.2, 0.3]])), 1e-6) is None
    assert kuf.support_radius(k, (1.0, [0.2, 0.3]), 1.5) is None


def test_ell_arg_and_grid_call_args():
    from hipgp_amd import kuf
    assert kuf._ell_arg(0.3, 2) == 0.3 and kuf._ell_arg(torch.tensor([0.3]), 2) == pytest.approx(0.3)
    assert kuf._ell_arg([0.3, 0.1], 2) == [0.3, 0.1]
    assert kuf._ell_arg(torch.tensor([0.5, 0.25], dtype=torch.float64), 2) == [0.5, 0.25]
    assert kuf._ell_arg([0.3, 0.1, 0.2], 2) is None and kuf._ell_arg(torch.ones(2, 2), 2) is None
    # the line-integral wrappers keep declining a vector ell (a CPU tensor declines anyway: the plans say why)
    k = _sqexp(torch.float32)
    grids = [torch.linspace(-1, 1, 8)] * 2
    x = torch.full((3, 2), 0.4)
    assert kuf.LineWindowPlan.make(k, grids, x, (1.0, [0.3, 0.2]), 1e-6) is None
    assert kuf.kuf_semi_sqexp(k, grids, x, (1.0, [0.3, 0.2])) is None
    assert kuf.kuf_semi_mc(k, grids, x, (1.0, [0.3, 0.2]), 4) is None


# ---- the model ---------------------------------------------------------------------------------------
def _grids(dims, dt=torch.float64):
    return [torch.linspace(-1, 1, m, dtype=dt) for m in dims]


@pytest.mark.parametrize("family", ["mean-field", "block"])
def test_model_takes_a_list_ell_init(family, capsys):
    import hipgp_amd.ziggy.hipgp as hg
    cls = hg.MeanFieldToeplitzGP if family == "mean-field" else hg.BlockToeplitzGP
    dt = torch.float64
    fam = {} if family == "mean-field" else dict(xblock_size=2)      # blocks of the expanded 10 x 14 grid
    mod = cls(_sqexp(dt), _grids((6, 8)), num_obs=5, sig2_init=1.2, ell_init=[0.3, 0.12], noise2_init=.1,
              learn_kernel=True, dtype=dt, **fam)
    out = capsys.readouterr().out
    assert "ell_init = (0.30, 0.12)" in out
    assert tuple(mod.ell.shape) == (2,) and tuple(mod.log_ell.shape) == (2,) and mod.log_ell.requires_grad
    assert mod.kernel.ard is True
    import hipgp_amd.ziggy.kernels as zk
    plain = zk.SqExp(dtype=dt)
    assert cls(plain, _grids((6, 8)), num_obs=5, ell_init=[0.3, 0.12], dtype=dt, **fam).kernel.ard is True
    assert plain.ard is True, "a vector ell_init declares the kernel it is given per-axis"
    assert torch.equal(mod.ell, torch.tensor([0.3, 0.12], dtype=dt))
    sig2, ell = mod.get_kernel_params()
    assert tuple(ell.shape) == (2,) and torch.allclose(ell, mod.ell)
    # the scalar form is what it was
    sc = cls(_sqexp(dt), _grids((6, 8)), num_obs=5, ell_init=0.3, learn_kernel=False, dtype=dt, **fam)
    assert "ell_init = 0.30," in capsys.readouterr().out
    assert sc.ell.dim() == 0 and sc.log_ell.dim() == 0
    sc.update_kernel_params(ell=(0.2, 0.4))
    assert tuple(sc.ell.shape) == (2,) and sc.get_kernel_params()[1] is sc.ell
    sc.update_kernel_params(ell=0.25)
    assert sc.ell.dim() == 0
    with pytest.raises(ValueError):
        sc.update_kernel_params(ell=(0.2, 0.4, 0.1))


def test_model_refuses_a_wrong_vector():
    import hipgp_amd.ziggy.hipgp as hg
    dt = torch.float64
    kw = dict(num_obs=5, learn_kernel=False, dtype=dt)
    with pytest.raises(ValueError, match="one value per grid axis"):
        hg.MeanFieldToeplitzGP(_sqexp(dt), _grids((6, 8)), ell_init=[0.3, 0.12, 0.2], **kw)
    with pytest.raises(ValueError, match="SqExp kernel only"):
        hg.MeanFieldToeplitzGP(_matern(dt), _grids((6, 8)), ell_init=[0.3, 0.12], **kw)
    with pytest.raises(ValueError, match="positive"):
        hg.MeanFieldToeplitzGP(_sqexp(dt), _grids((6, 8)), ell_init=[0.3, 0.0], **kw)


def test_model_refuses_line_integrals_with_a_vector_ell():
    import hipgp_amd.ziggy.hipgp as hg
    dt = torch.float64
    mod = hg.MeanFieldToeplitzGP(_sqexp(dt), _grids((6, 8)), num_obs=5, ell_init=[0.3, 0.12], learn_kernel=False,
                                 dtype=dt)
    x = torch.full((3, 2), 0.4, dtype=dt)
    y = torch.zeros(3, 1, dtype=dt)
    with pytest.raises(NotImplementedError, match="one length scale per axis"):
        mod._make_grams(x, integrated_obs=True)
    for call in (lambda: mod.predict(x, integrated_obs=True), lambda: mod.predict_mean(x, integrated_obs=True),
                 lambda: mod.predict_draws(x, 2, integrated_obs=True), lambda: mod.fit_mean(x, y, integrated_obs=True),
                 lambda: mod.predict_line_samples(x, 2)):
        with pytest.raises(NotImplementedError, match="one length scale per axis"):
            call()


# ---- the C ABI ---------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_ard_entries():
    from hipgp_amd import _lib
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    L = _lib.lib()
    for s in ARD_SYMS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + s + r"\s*\(", src, re.S)
        assert m, f"include/hipgp.h does not declare {s} under a comment"
        assert "kernels.py:73-79" in m.group(1), f"{s}: the declaration does not cite the reference lines it serves"
        assert hasattr(L, s), f"libhipgp.so does not export {s}"
        assert s in _lib.EXPORTS and getattr(L, s).argtypes is not None


class _Args:
    """A well-formed argument set (host addresses standing in for device ones: every call below must
    return before anything is launched), with one field replaced per case."""

    def __init__(self):
        self.buf = (ctypes.c_float * 64)()
        self.idx = (ctypes.c_int64 * 64)()
        p = ctypes.cast(self.buf, ctypes.c_void_p)
        q = ctypes.cast(self.idx, ctypes.c_void_p)
        self.m = (ctypes.c_int64 * 2)(4, 4)
        self.grids = (ctypes.c_void_p * 2)(p.value, p.value)
        self.kw = dict(kind=SQEXP, ndim=2, ell=(0.5, 0.25), rho=(0.5, 0.3), p=p, q=q)

    def call(self, L, name, **over):
        a = dict(self.kw, **over)
        dv = lambda v: None if v is None else (ctypes.c_double * len(v))(*v)
        ell, rho, p, q = dv(a["ell"]), dv(a["rho"]), a["p"], a["q"]
        head = (F32, a["kind"], a["ndim"], self.m, self.grids, p, 2, 1.0, ell)
        if name == "hgp_kuf_grid_ard":
            return L.hgp_kuf_grid_ard(*head, p, None)
        if name == "hgp_kuf_grid_grad_ard":
            return L.hgp_kuf_grid_grad_ard(*head, p, p, None)
        if name == "hgp_kuf_grid_matvec_ard":
            return L.hgp_kuf_grid_matvec_ard(*head, p, 2, 0, p, None)
        if name == "hgp_kuf_grid_rmatvec_ard":
            return L.hgp_kuf_grid_rmatvec_ard(*head, p, 2, 0, p, None)
        if name == "hgp_kuf_grid_matvec_win_ard":
            return L.hgp_kuf_grid_matvec_win_ard(*head, rho, p, 2, p, None)
        return L.hgp_kuf_grid_rmatvec_win_ard(*head, rho, p, 2, q, q, p, None)


BAD = [("matern", dict(kind=MATERN32)), ("gneiting", dict(kind=GNEITING)), ("bad_kind", dict(kind=9)),
       ("zero_ell", dict(ell=(0.5, 0.0))), ("negative_ell", dict(ell=(-0.5, 0.25))),
       ("nan_ell", dict(ell=(float("nan"), 0.25))), ("inf_ell", dict(ell=(0.5, float("inf")))),
       ("null_ell", dict(ell=None)), ("ndim0", dict(ndim=0)), ("ndim4", dict(ndim=4)),
       ("negative_rho", dict(rho=(0.5, -1e-3))), ("nan_rho", dict(rho=(float("nan"), 0.3))),
       ("inf_rho", dict(rho=(float("inf"), 0.3))), ("null_rho", dict(rho=None))]
BAD_CALLS = [(n, t, o) for n in ARD_SYMS for t, o in BAD if "rho" not in t or "_win_" in n]


@pytest.mark.parametrize("name,tag,over", BAD_CALLS, ids=[f"{c[0]}-{c[1]}" for c in BAD_CALLS])
def test_ard_entries_refuse_bad_arguments_before_any_hip_call(name, tag, over):
    from hipgp_amd import _lib
    L = _lib.lib()
    a = _Args()
    for i in range(64):
        a.buf[i] = 3.0
    rc = a.call(L, name, **over)
    assert rc == E_ARG, (name, tag, rc)
    assert len(L.hgp_last_error()) > 0
    assert all(v == 3.0 for v in a.buf)


# ---- the Fourier features ----------------------------------------------------------------------------
def test_spectral_features_scale_per_axis():
    from hipgp_amd import rff
    k = _sqexp()
    ell = [0.3, 0.12, 0.7]
    gen = lambda: torch.Generator().manual_seed(17)          # the same normal draws for every call
    iso, ph0 = rff.spectral_features(k, (1.0, 1.0), 3, 64, generator=gen())
    for form in (ell, torch.tensor(ell, dtype=torch.float64)):
        om, ph = rff.spectral_features(k, (1.0, form), 3, 64, generator=gen())
        assert torch.equal(ph, ph0)
        assert torch.equal(om, iso / torch.tensor(ell, dtype=torch.float64))
    one, _ = rff.spectral_features(k, (1.0, 0.3), 3, 64, generator=gen())
    assert torch.equal(one, iso / 0.3), "a scalar ell is what it was"
    with pytest.raises(NotImplementedError):
        rff.spectral_features(_matern(), (1.0, ell), 3, 64, generator=gen())
    with pytest.raises(NotImplementedError):
        rff.spectral_features(k, (1.0, ell[:2]), 3, 64, generator=gen())
    import hipgp_amd.ziggy.kernels as zk
    with pytest.raises(NotImplementedError, match="SqExp"):       # not declared per-axis: refused as before
        rff.spectral_features(zk.SqExp(dtype=torch.float64), (1.0, ell), 3, 64, generator=gen())
