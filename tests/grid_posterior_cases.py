"""Shared by tests/test_grid_posterior_{cpu,gpu}.py: the NumPy restatement of HGP_OP_RSQ on the
oracle's spectrum, dense references of the inducing-grid posterior, and error figures."""
import numpy as np
import scipy.fft as sfft
import torch

from oracle import ziggy_oracle as zo


def oracle_rsq(O, w):
    """(R o R) w on a ToeplitzOracle: the circulant whose generator is the square of R's generator
    s = IFFT_n(sqrt D), applied to w (B, M') on the n-grid and cropped to the m-grid."""
    B = w.shape[0]
    spec = sfft.fftn(sfft.ifftn(O.D_sqrt).real ** 2)
    c = np.asarray(w).reshape((B,) + O.ndims).astype(zo._cdtype(O.dtype))
    return O._crop(O._apply(spec, c)).astype(O.dtype)


def dense_R(O):
    """R as a dense (M, M') matrix from the oracle's own operator."""
    return O.matmul_R(np.eye(O.Mp, dtype=O.dtype)).T.copy()


def max_rel(a, ref):
    """max |a - ref| / max |ref| in fp64."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


class OracleKmm:
    """A Kmm whose R and R o R are the fp64 oracle's, on CPU tensors: what `grid_posterior` and
    `sample_grid` call."""

    def __init__(self, O):
        self.O = O
        self.column = torch.tensor(O.column)
        self.calls = []

    def _matmul_by_R(self, w):
        self.calls.append(("R", tuple(w.shape)))
        return torch.from_numpy(self.O.matmul_R(w.detach().numpy()))

    def _matmul_by_Rsq(self, w):
        self.calls.append(("Rsq", tuple(w.shape)))
        return torch.from_numpy(oracle_rsq(self.O, w.detach().numpy()))
