"""Product-form detection without a device (hgp_separable_detect, the host arithmetic that
hgp_plan_set_column's device scan repeats), and the register budget of the k_sep_pass kernels."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import ziggy_oracle as zo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipgp_amd", "libhipgp.so")
LLVM = "/opt/rocm/lib/llvm/bin"
ACCEPT = 4.0          # HGP_SEP_ACCEPT (hgp_sep_host.hpp)


def _column(kind, dims, params, jitter, dt):
    grids = [np.linspace(-1, 1, m) for m in dims]
    nu = 1.5 if kind == "matern" else None
    return zo.toeplitz_column(grids, lambda x, y: zo.kernel_eval(kind, x, y, params, nu=nu), jitter).astype(dt)


def _detect(col, dims, jitter=0.0):
    from hipgp_amd import _lib
    col = np.ascontiguousarray(col)
    out = (ctypes.c_double * 4)()
    t0 = (ctypes.c_double * dims[0])()
    t1 = (ctypes.c_double * dims[1])()
    _lib.check(_lib.lib().hgp_separable_detect(_lib.HGP_F32 if col.dtype == np.float32 else _lib.HGP_F64, dims[0],
                                               dims[1], col.ctypes.data_as(ctypes.c_void_p), jitter, out, t0, t1))
    return bool(out[0]), out[1], out[2], out[3], np.array(t0), np.array(t1)


CASES = [((1024, 1024), .01, 1e-3, np.float32),      # the benchmark's grid: most entries underflow
         ((1024, 1024), .2, 1e-2, np.float32),       # a wide kernel
         ((96, 80), .2, 1e-2, np.float32), ((1024, 16), .05, 1e-3, np.float32), ((16, 1024), .05, 1e-3, np.float32),
         ((48, 40), .1, 1e-3, np.float64), ((33, 64), .1, 0.0, np.float64), ((64, 256), .02, 1e-3, np.float64)]


@pytest.mark.parametrize("dims,ell,jitter,dt", CASES, ids=[f"{d[0]}x{d[1]}_{np.dtype(t).name}" for d, _, _, t in CASES])
def test_sqexp_columns_are_accepted(dims, ell, jitter, dt):
    eps = 2.0 ** -24 if dt == np.float32 else 2.0 ** -53
    col = _column("sqexp", dims, (1., ell), jitter, dt)
    ok, sigma, resid, k00, t0, t1 = _detect(col, dims)
    print(f"{dims} ell={ell} {np.dtype(dt).name}: residual {resid / eps:.2f} units of rounding")
    assert ok and resid <= ACCEPT * eps
    assert abs(sigma - jitter) <= 4 * eps * abs(col).max()
    assert abs(t0[0] * t1[0] - k00) <= 1e-15 * k00
    c2 = col.astype(np.float64).reshape(dims)
    rec = np.outer(t0, t1)
    rec[0, 0] += sigma
    assert np.max(np.abs(rec - c2)) <= ACCEPT * eps * abs(col).max()


def test_jitter_argument_is_added_to_the_corner():
    dims = (48, 40)
    col = _column("sqexp", dims, (1., .1), 0.0, np.float64)
    ok, sigma, *_ = _detect(col, dims, jitter=1e-3)
    assert ok and abs(sigma - 1e-3) <= 4 * 2.0 ** -53


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_matern_and_perturbed_columns_are_refused(dt):
    eps = 2.0 ** -24 if dt == np.float32 else 2.0 ** -53
    dims = (96, 80)
    ok, _, resid, *_ = _detect(_column("matern", dims, (.1, .1), 1e-3, dt), dims)
    assert not ok and resid > 1e4 * ACCEPT * eps
    col = _column("sqexp", dims, (1., .05), 1e-3, dt).reshape(dims).copy()
    col[3, 2] *= 1 + 1e-3
    ok, _, resid, *_ = _detect(col.reshape(-1), dims)
    assert not ok and resid > 100 * ACCEPT * eps
    # every off-corner entry underflowed: nothing to estimate k00 from
    z = np.zeros(dims, dt)
    z[0, :] = 1e-3
    z[:, 0] = 1e-3
    z[0, 0] = 1
    assert not _detect(z.reshape(-1), dims)[0]
    # a negative jitter is not a product kernel plus a nugget
    col = _column("sqexp", dims, (1., .05), 0.0, dt)
    assert not _detect(col, dims, jitter=-1e-3)[0]


def test_sep_kernels_do_not_spill_and_fit_four_waves():
    if not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-objdump")):
        pytest.skip("library or ROCm LLVM tools absent")
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(LIB, td)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", os.path.basename(LIB)], cwd=td, capture_output=True, check=True)
        notes = "".join(subprocess.run([f"{LLVM}/llvm-readelf", "--notes", os.path.join(td, f)], capture_output=True,
                                       text=True, check=True).stdout for f in sorted(os.listdir(td)) if "gfx950" in f)
    recs = {}
    for blk in notes.split("  - .agpr_count")[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m and "k_sep_pass" in m.group(1):
            get = lambda k: int((re.search(r"\." + k + r":\s+(\d+)", blk) or [0, 0])[1])
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            recs[name] = (get("vgpr_spill_count"), get("private_segment_fixed_size"), get("vgpr_count"))
    f32 = {n: r for n, r in recs.items() if "<float" in n}
    assert len(f32) >= 12
    assert not [n for n, (s, p, v) in f32.items() if s or p], f32
    s, p, v = recs["void hgp::k_sep_pass<float, 1024>(hgp::SepDesc)"]
    assert v <= 128, v
