"""hgp_rt_stats without a GPU: the symbol is exported and bound with the declared signature, the
header and the ctypes binding agree on the argument list, and the argument errors that need no
device return the documented codes.  (The register check of the new k_row_inv_t<.., EPI_STATS, ..>
instantiations is tests/test_kernel_resources_cpu.py on the rebuilt library.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HGP_E_ARG = -1


def _header_decl():
    src = open(os.path.join(ROOT, "include", "hipgp.h")).read()
    m = re.search(r"\bint\s+hgp_rt_stats\s*\(([^)]*)\)\s*;", src)
    assert m, "include/hipgp.h does not declare hgp_rt_stats"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbol_exported_and_bound():
    from hipgp_amd import _lib
    L = _lib.lib()
    assert "hgp_rt_stats" in _lib.EXPORTS
    fn = L.hgp_rt_stats
    assert fn.restype is ctypes.c_int
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert list(fn.argtypes) == [vp, vp, i64, vp, vp, vp]


def test_header_and_binding_agree():
    from hipgp_amd import _lib
    args = _header_decl()
    assert args == ["hgp_plan* plan", "const void* d", "int64_t nrhs", "const void* qm", "const void* qS", "void* out3"]
    ctype_of = lambda a: ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_void_p if "*" in a else None
    assert [ctype_of(a) for a in args] == list(_lib.lib().hgp_rt_stats.argtypes)


def test_argument_errors_without_device():
    from hipgp_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.hgp_rt_stats(None, p, 1, p, p, p) == HGP_E_ARG
    assert b"null plan" in L.hgp_last_error()
    assert L.hgp_rt_stats(None, None, 0, None, None, None) == HGP_E_ARG     # the plan is checked first


def test_python_entry_points_exist():
    from hipgp_amd.plan import ToeplitzPlan
    from hipgp_amd.ziggy.misc.toeplitz_tensor import ToeplitzTensor
    import hipgp_amd.ziggy.hipgp as hg
    import inspect
    assert callable(ToeplitzPlan.rt_stats) and callable(ToeplitzTensor.rt_stats)
    sig = inspect.signature(hg.ToeplitzInducingGP.predict)
    assert sig.parameters["fused"].default is None
    assert hg.MeanFieldToeplitzGP.predict_stats is not hg.ToeplitzInducingGP.predict_stats
    assert hg.BlockToeplitzGP.predict_stats is hg.ToeplitzInducingGP.predict_stats
