"""Toeplitz-whitened SVGP ("HIP-GP") models on the MI355X operators.

Mirrors the reference model API of `ziggy/hipgp.py` for the parts that sit on the hot path:
`ToeplitzInducingGP.compute_kn` (`hipgp.py:117-146`) and the mean-field
family's ELBO, natural gradient and prediction (`hipgp.py:160-276, 370-446, 449-524`,
SURVEY §8(f) row 3).  `Knm` comes from the fused grid kernel hgp_kuf_grid (SURVEY §8(f)
row 1, `hipgp_amd/kuf.py`).  `kn = R^T K^{-1} Knm^T` runs as one plan set-up + hgp_pcg_solve +
hgp_toeplitz_apply(R^T) on the device; the batch reductions are device tensor ops.

The natural-gradient statistics are split into per-RHS sums (`batch_stats`) and the update
built from them (`apply_stats`), so a caller that shards the minibatch over GPUs
(`hipgp_amd.dist`) all-reduces exactly those sums.

Line-integral observations come from the fused kernels of `hipgp_amd.kuf`.
The block-diagonal family's statistics (per-block grams, kn^T S kn) are the fused kernel
hgp_block_stats.

Kernel / noise hyper-parameter learning: with learn_kernel / learn_noise the
ELBO returned by `elbo_and_grad` carries the autograd graph through Knm, Knn and kn (InvMatmul's
backward PCG + hgp_plan_dqf, the R^T column gradient hgp_plan_column_grad), as the reference's
fit loop needs it (`svi_gp.py:317-326`).

`batch_solve` (`hipgp.py:278-368`, the full-batch solve of the mean-field family) is built:
one compute_kn per batch and the device statistics kernel, with the reference's
UnboundLocalError at `hipgp.py:314` fixed (parity pinned by the oracle restatement only).
Not built (OUT of the hot path): the full-rank variational family
(`FullRankToeplitzGP`, `hipgp.py:693-797`: a dense M' x M' covariance, 70 TB at C2).
"""
import collections
import contextlib
import os

import numpy as np
import torch
from torch import nn

from hipgp_amd.ziggy.misc.toeplitz_tensor import ToeplitzTensor
from hipgp_amd.ziggy.svi_gp import SviGP

LN_2PI = float(np.log(2 * np.pi))

# what `ToeplitzInducingGP.fit_mean` returns
MeanFit = collections.namedtuple("MeanFit", ["weights", "qm", "iters", "relres"])


def diag_kl_to_standard(m, S):
    """KL(N(m, diag S) || N(0, I))  (`ziggy/misc/stats.py:4-8`)."""
    return 0.5 * (torch.sum(S) + torch.sum(m * m) - torch.sum(torch.log(S)) - m.shape[0])


def expanded_size(xgrids):
    """M' = prod(2 m_i - 2) (m_i > 1) else m_i  (`hipgp.py:72`)."""
    return int(np.prod([2 * len(g) - 2 if len(g) > 1 else len(g) for g in xgrids]))


class ToeplitzInducingGP(SviGP):
    """`hipgp.py:15-446` (hot-path subset)."""

    def __init__(self, kernel, xgrids, num_obs, sig2_init=1., ell_init=.05, noise2_init=1.,
                 learn_kernel=True, learn_noise=True, dtype=torch.float, whitened_type='ziggy',
                 parameterization='expectation-family', jitter_val=1e-3):
        super().__init__()
        assert len(xgrids) > 1, len(xgrids)
        self.learn_kernel = learn_kernel
        self.learn_noise = learn_noise
        self.jitter_val = jitter_val
        self.dtype = dtype
        self.kernel = kernel
        self.N = num_obs
        # ell_init: a float, or one positive float per axis (SqExp alone: `kernels.py:73-79` takes ell
        # "a scalar, or a tensor that matches the dimension of data"); self.ell and log_ell are then (D,)
        self.ell = self._ell_tensor(ell_init, kernel, len(xgrids), dtype)
        self.sig2 = torch.tensor(sig2_init, dtype=dtype)
        self.noise2 = torch.tensor(noise2_init, dtype=dtype)
        self.log_ell = nn.Parameter(torch.log(self.ell.clone()), requires_grad=learn_kernel)
        self.log_sig2 = nn.Parameter(torch.log(self.sig2.clone()), requires_grad=learn_kernel)
        self.log_noise2 = nn.Parameter(torch.log(self.noise2.clone()), requires_grad=learn_noise)
        ell_txt = f"{float(self.ell):.2f}" if self.ell.dim() == 0 else \
            "(" + ", ".join(f"{float(e):.2f}" for e in self.ell) + ")"
        print(f"Model initialization: sig2 = {sig2_init:.2f}, ell_init = {ell_txt}, noise2 = {noise2_init:.2f}")
        self.xgrids = xgrids
        mesh = torch.meshgrid(*xgrids, indexing="ij")
        self.xinduce = torch.stack([g.reshape(-1) for g in mesh], dim=-1)
        self.M = self.xinduce.shape[0]
        self.whitened_type = whitened_type
        if whitened_type == 'cholesky':
            self.Mprime = self.M
        else:
            assert whitened_type == 'ziggy', whitened_type
            self.Mprime = expanded_size(xgrids)
        self.parameterization = parameterization

    @property
    def name(self):
        raise NotImplementedError

    def cuda_params(self, cuda_num=0):
        """Move the model and its grids to `cuda:{cuda_num}` (`hipgp.py:80-90`)."""
        device = torch.device(f"cuda:{cuda_num}")
        self.to(device)
        self.xinduce = self.xinduce.to(device)
        self.kernel = self.kernel.to(device)
        self.xgrids = [g.to(device) for g in self.xgrids]
        if self._ard():      # a (D,) ell divides device tensors (a 0-d one may stay on the host, as it always has)
            self.ell = self.ell.to(device)
        return self

    @staticmethod
    def _ell_tensor(ell, kernel, ndim, dtype, device=None):
        """ell as the model keeps it: a 0-d tensor for a scalar, a (D,) tensor for one length scale per
        axis.  ValueError for a vector with a kernel other than SqExp, of the wrong length or with an
        entry that is not positive.  A valid vector declares the kernel per-axis (`SqExp.ard = True`), which
        is what lets the fused routes of `hipgp_amd.kuf` / `hipgp_amd.rff` read it as per-axis scales."""
        if torch.is_tensor(ell):
            t = ell.detach().to(dtype=dtype, device=device)
        else:
            t = torch.tensor(ell, dtype=dtype, device=device)
        if t.dim() == 0:
            return t
        from . import kernels as zk
        if not isinstance(kernel, zk.SqExp):
            raise ValueError(f"one length scale per axis is defined for the SqExp kernel only, not {type(kernel).__name__} "
                             "(the Matern formula has no vector ell)")
        if t.dim() != 1 or t.numel() != ndim:
            raise ValueError(f"ell must be a scalar or hold one value per grid axis ({ndim}), got shape {tuple(t.shape)}")
        if not bool(torch.all(t > 0)) or not bool(torch.all(torch.isfinite(t))):
            raise ValueError(f"every length scale must be positive and finite, got {t.tolist()}")
        kernel.ard = True
        return t

    def _ard(self):
        """True when the kernel has one length scale per axis."""
        return self.ell.dim() > 0

    _NO_ARD_LINES = ("integrated_obs=True with one length scale per axis: the line-integral cross covariances and "
                     "the doubly-integrated diagonal table are functions of |x / ell| for ONE ell; use a scalar ell "
                     "for line-integral observations")

    def _check_ard_lines(self, integrated_obs):
        if integrated_obs and self._ard():
            raise NotImplementedError(self._NO_ARD_LINES)

    def get_kernel_params(self):
        if not self.learn_kernel:
            return self.sig2, self.ell
        return torch.exp(self.log_sig2), torch.exp(self.log_ell)

    def update_kernel_params(self, sig2=None, ell=None):
        assert not self.learn_kernel
        if sig2 is not None:
            self.sig2 = torch.tensor(sig2, dtype=self.dtype, device=self.sig2.device)
        if ell is not None:
            self.ell = self._ell_tensor(ell, self.kernel, len(self.xgrids), self.dtype, self.ell.device)
            if self._ard():
                self.ell = self.ell.to(self.xgrids[0].device)

    def noise_terms(self, noise_std_batch):
        """(1/sigma_n^2, log sigma_n): per observation or from log_noise2 (`hipgp.py:227-230,394-399`)."""
        if noise_std_batch is not None:
            return (1 / noise_std_batch ** 2), torch.log(noise_std_batch)
        return torch.exp(-self.log_noise2), 0.5 * self.log_noise2

    # ---- the hot path ----------------------------------------------------------------------
    def toeplitz(self):
        """A fresh ToeplitzTensor for the current kernel parameters (`hipgp.py:142-143`)."""
        params = self.get_kernel_params()
        return ToeplitzTensor(xgrids=self.xgrids, kernel=lambda x, y: self.kernel(x, y, params=params),
                              batch_shape=None, jitter_val=self.jitter_val)

    def compute_kn(self, Knm, maxiter_cg=10, tol=1e-8, Kmm=None):
        """kn = R^T Kmm^{-1} Knm^T (ziggy whitening) or L^{-1} Knm^T (cholesky), (bsz, M')."""
        if self.whitened_type == 'cholesky':
            params = self.get_kernel_params()
            if Kmm is None:
                Kmm = self.kernel(self.xinduce, self.xinduce, params)
            eye = torch.eye(Kmm.shape[0], dtype=Knm.dtype, device=Knm.device)
            L = torch.linalg.cholesky(Kmm + self.jitter_val * eye)
            return torch.linalg.solve_triangular(L, Knm.t(), upper=False).t()
        if Kmm is None:
            Kmm = self.toeplitz()
        d0 = Kmm.inv_matmul(Knm, do_precond=True, maxiter=maxiter_cg, tol=tol)
        return Kmm._matmul_by_RT(d0)

    # ---- variational family hooks ------------------------------------------------------------
    def standard_variational_params(self):
        raise NotImplementedError

    def compute_knSkn(self, kn, qS):
        raise NotImplementedError

    def predict_stats(self, Knm, maxiter_cg=50, Kmm=None):
        """(bsz, 3) rows (kn.qm, kn.kn, kn S kn) for `predict(fused=True)` without kn itself, or
        None where the family (or the whitening, or a caller's Kmm) has no fused route."""
        return None

    def fit_stats(self, Knm, ybatch, Knn_diag, noise_std_batch=None, maxiter_cg=10, Kmm=None):
        """The dict of `batch_stats` for `elbo_and_grad(fused=True)` without kn itself, or None
        (Knm untouched) where the family, the whitening or a caller's Kmm has no fused route."""
        return None

    def streamed_predict_stats(self, Knm, maxiter_cg=50, Kmm=None):
        """`predict_stats` for `predict(streamed=True)`: the same (bsz, 3) rows from kn streamed a
        piece of right-hand sides at a time (hgp_rt_block_stats), or None (Knm untouched) where the
        family, the whitening or a caller's Kmm has no streamed route."""
        return None

    def streamed_fit_stats(self, Knm, ybatch, Knn_diag, noise_std_batch=None, maxiter_cg=10, Kmm=None):
        """`fit_stats` for `elbo_and_grad(streamed=True)`: the dict of `batch_stats` from kn streamed
        a piece of right-hand sides at a time (hgp_rt_block_stats), or None (Knm untouched) where the
        family, the whitening or a caller's Kmm has no streamed route."""
        return None

    def get_kl_to_prior(self, qm, qS):
        raise NotImplementedError

    # ---- the posterior on the whole inducing grid ---------------------------------------------
    _NO_GRID_POSTERIOR = ("the inducing-grid posterior needs the whitened mean-field family "
                          "(MeanFieldToeplitzGP, whitened_type='ziggy'): its variance diag(R S R^T) is the "
                          "circulant operator R o R applied to diag S only for a diagonal S -- a "
                          "block-diagonal S has no circulant R S R^T diagonal, and cholesky whitening has "
                          "no circulant R at all")

    def grid_posterior(self, prior=False, Kmm=None):
        raise NotImplementedError(self._NO_GRID_POSTERIOR)

    def sample_grid(self, n, prior=False, generator=None, eps=None, Kmm=None):
        raise NotImplementedError(self._NO_GRID_POSTERIOR)

    # ---- ELBO --------------------------------------------------------------------------------
    def compute_batch_an(self, xbatch, ybatch, noise_std_batch=None, qm=None, qS=None, Knm=None,
                         Knn_diag=None, kn=None, maxiter_cg=10, integrated_obs=False,
                         semi_integrated_estimator=None, semi_integrated_samps=None,
                         cache_K_matmul=None, print_debug_info=False, Kmm=None):
        """a_n = -1/2 ln 2 pi s^2 - (mse + Knn - kn.kn + kn S kn) / 2 s^2  (`hipgp.py:370-414`)."""
        if qm is None or qS is None:
            qm, qS = self.standard_variational_params()
        if Knm is None or Knn_diag is None:
            Knm, Knn_diag = self._make_grams(xbatch, integrated_obs=integrated_obs,
                                             semi_integrated_estimator=semi_integrated_estimator or "analytic",
                                             semi_integrated_samps=semi_integrated_samps or 10)
        if kn is None:
            kn = self.compute_kn(Knm, maxiter_cg=maxiter_cg, Kmm=Kmm)
        ivar, log_sd = self.noise_terms(noise_std_batch)
        if noise_std_batch is not None:
            # reference shapes (hipgp.py:396-398): ivar squeezed, log(noise_std) kept (bsz, 1), so
            # with per-observation noise a_n broadcasts to (bsz, bsz); its mean is the ELBO term
            ivar = ivar.squeeze()
        mse = (kn.matmul(qm).squeeze() - ybatch.squeeze()) ** 2
        variance = Knn_diag.squeeze() - torch.sum(kn * kn, dim=-1).squeeze() + self.compute_knSkn(kn, qS)
        if print_debug_info:
            print("mse = {:.4f}".format(torch.mean(mse)))
            print("variance = {:.4f}".format(torch.mean(variance)))
        return -0.5 * ivar * (mse + variance) - log_sd - 0.5 * LN_2PI

    def elbo(self, xbatch, ybatch, noise_std_batch=None, maxiter_cg=10, integrated_obs=False,
             semi_integrated_estimator="analytic", semi_integrated_samps=10, Kmm=None,
             print_debug_info=False):
        """mean_n a_n - KL/N  (`hipgp.py:160-192`)."""
        Knm, Knn_diag = self._make_grams(xbatch, integrated_obs=integrated_obs,
                                         semi_integrated_estimator=semi_integrated_estimator,
                                         semi_integrated_samps=semi_integrated_samps)
        kn = self.compute_kn(Knm, maxiter_cg=maxiter_cg, Kmm=Kmm)
        qm, qS = self.standard_variational_params()
        an = self.compute_batch_an(xbatch, ybatch, noise_std_batch, qm=qm, qS=qS, Knm=Knm,
                                   Knn_diag=Knn_diag, kn=kn)
        return torch.mean(an) - self.get_kl_to_prior(qm, qS) / self.N

    def elbo_and_grad(self, xbatch, ybatch, noise_std_batch=None, maxiter_cg=10, integrated_obs=False,
                      semi_integrated_estimator="analytic", semi_integrated_samps=10,
                      print_debug_info=False, Kmm=None, mc_offset=None, fused=None, streamed=None):
        """ELBO estimate; sets theta1.grad / theta2.grad to minus the natural gradient
        (`hipgp.py:194-276`).  mc_offset: see `SviGP._make_grams` (sharded fits).

        fused=True takes the batch sums straight from the R^T pass (`fit_stats`, hgp_rt_fit_stats)
        where the family has them and no hyper-parameter gradient is asked for (the autograd ELBO
        needs kn), so the (bsz, M') kn is never allocated; every other case takes the materialised
        path.  None reads HGP_FIT_FUSED (default off).

        streamed=True is the block family's route to the same end (`streamed_fit_stats`,
        hgp_rt_block_stats: kn held one piece of right-hand sides at a time), tried first and under
        the same condition; a family without it proceeds as if the keyword were off.  None reads
        HGP_BLOCK_STREAMED (default off).

        With learn_kernel the returned ELBO carries the graph through Knm; the model attribute
        `kuf_grad` (None reads HGP_KUF_GRAD, default off) makes that graph the fused Kuf forward
        and backward of `hipgp_amd.kuf` (`SviGP._make_grams`) instead of torch's (B, M, D)
        broadcast and the intermediates autograd keeps of it."""
        assert self.parameterization == 'expectation-family', \
            "need parameterization=expectation-family when performing natural gradient descent"
        if fused is None:
            fused = os.environ.get("HGP_FIT_FUSED", "0") not in ("", "0")
        if streamed is None:
            streamed = os.environ.get("HGP_BLOCK_STREAMED", "0") not in ("", "0")
        Knm, Knn_diag = self._make_grams(xbatch, integrated_obs=integrated_obs,
                                         semi_integrated_estimator=semi_integrated_estimator,
                                         semi_integrated_samps=semi_integrated_samps, mc_offset=mc_offset)
        if streamed and not self.hyper_grad_needed(noise_std_batch):
            stats = self.streamed_fit_stats(Knm, ybatch, Knn_diag, noise_std_batch, maxiter_cg=maxiter_cg, Kmm=Kmm)
            if stats is not None:
                return self.apply_stats(stats, xbatch.shape[0])
        if fused and not self.hyper_grad_needed(noise_std_batch):
            stats = self.fit_stats(Knm, ybatch, Knn_diag, noise_std_batch, maxiter_cg=maxiter_cg, Kmm=Kmm)
            if stats is not None:
                return self.apply_stats(stats, xbatch.shape[0])
        kn = self.compute_kn(Knm, maxiter_cg=maxiter_cg, Kmm=Kmm)
        stats = self.batch_stats(kn, ybatch, Knn_diag, noise_std_batch)
        elbo = self.apply_stats(stats, xbatch.shape[0])
        if self.hyper_grad_needed(noise_std_batch):
            # learn_kernel / learn_noise: the fit loop back-propagates the returned ELBO
            # (`svi_gp.py:317-326`), so it carries the graph to log_sig2 / log_ell / log_noise2
            # through Knm, Knn and kn (InvMatmul.backward + the R^T column gradient) as in
            # `hipgp.py:214-227`, with the variational parameters held fixed (`:216-217`)
            elbo = self.autograd_elbo(xbatch, ybatch, noise_std_batch, Knm, Knn_diag, kn)
        return elbo

    def batch_solve(self, xobs, yobs, noise_std=None, batch_size=-1, maxiter_cg=10, integrated_obs=False,
                    semi_integrated_estimator="analytic", semi_integrated_samps=10, compute_elbo=False,
                    Kmm=None, print_debug_info=False):
        """Closed-form variational parameters from all observations (`hipgp.py:278-368`):
           lam  = I_lam + sum_n ivar_n kn_n kn_n^T restricted to the family (diag / blocks),
           b    = sum_n ivar_n y_n kn_n,
           m    = (I + sum_n ivar_n kn_n kn_n^T)^{-1} b   (dense M' x M' solve),
           theta2 = -lam / 2, theta1 = lam m (mean-field) / blockdiag(lam) m (block);
        with compute_elbo the ELBO of the solved model over the same batches.

        kn per batch is the device compute_kn (one plan reused for every batch: the reference
        builds an identical ToeplitzTensor per call, `:294`).  The dense M' x M' system limits this
        to small grids (M' = 1444 on 20 x 20), as in the reference.  The reference reads
        `noise_std_batch` before assigning it (`:314`, UnboundLocalError on every call); here the
        intended rule holds: per-observation noise_std[bi] when given, else exp(-log_noise2)."""
        if xobs.shape[0] != self.N:
            print("x obs shape = {}, total_num_obs = {}".format(xobs.shape[0], self.N))
        if batch_size == -1:
            batch_size = xobs.shape[0]
        nb = int(np.ceil(len(xobs) / batch_size))
        batches = [slice(i * batch_size, min((i + 1) * batch_size, len(xobs))) for i in range(nb)]
        dev = self.xgrids[0].device
        if self.whitened_type == 'cholesky':
            Kmm = self.kernel(self.xinduce, self.xinduce, self.get_kernel_params())
        elif Kmm is None:
            Kmm = self.toeplitz()
        gram_kw = dict(integrated_obs=integrated_obs, semi_integrated_estimator=semi_integrated_estimator,
                       semi_integrated_samps=semi_integrated_samps)

        def noise_of(bi):
            return None if noise_std is None else noise_std[bi].to(dev)

        lam = self.get_identity_for_lam()
        b = 0
        big_lam = torch.eye(self.Mprime, dtype=self.dtype, device=dev)
        with torch.no_grad():
            for bi in batches:
                xb, yb = xobs[bi].to(dev), yobs[bi].to(dev)
                Knm, _ = self._make_grams(xb, **gram_kw)
                kn = self.compute_kn(Knm, maxiter_cg=maxiter_cg, Kmm=Kmm)
                sb = noise_of(bi)
                ivar = 1 / sb ** 2 if sb is not None else torch.exp(-self.log_noise2)
                lam = lam + self.get_lam(ivar_noise=ivar, kn=kn, bscale=1.0, add_identity=False)
                b = b + torch.sum(ivar * yb * kn, dim=0)
                big_lam += (ivar * kn).t().matmul(kn)
            mhat = torch.linalg.solve(big_lam, b[:, None])
            if self.parameterization == 'standard':
                self.global_S.data[:] = self.get_S_from_lam(lam)
                self.global_m.data[:] = mhat
            else:
                self.global_theta2.data[:] = -.5 * lam
                if self.name == 'mean-field':
                    self.global_theta1.data[:] = (mhat.squeeze() * lam.squeeze())[:, None]
                else:
                    self.global_theta1.data[:] = self.block_diag_multiply(lam, mhat.t()).t()
        if not compute_elbo:
            return None
        qm, qS = self.standard_variational_params()
        elbo = 0
        for bi in batches:
            an = self.compute_batch_an(xobs[bi].to(dev), yobs[bi].to(dev), noise_of(bi), qm=qm, qS=qS,
                                       maxiter_cg=maxiter_cg, Kmm=Kmm, print_debug_info=print_debug_info,
                                       **gram_kw)
            elbo += torch.sum(an)
        return elbo / xobs.shape[0] - self.get_kl_to_prior(qm, qS) / self.N

    def hyper_grad_needed(self, noise_std_batch=None):
        """True when the ELBO must carry an autograd graph to the kernel / noise parameters."""
        if not torch.is_grad_enabled():
            return False
        kern = self.learn_kernel and (self.log_sig2.requires_grad or self.log_ell.requires_grad)
        noise = noise_std_batch is None and self.log_noise2.requires_grad
        return bool(kern or noise)

    def autograd_elbo(self, xbatch, ybatch, noise_std_batch, Knm, Knn_diag, kn, nsum=None, bsz=None):
        """mean_n a_n - KL/N with autograd through Knm, Knn_diag, kn and the noise terms
        (`hipgp.py:214-227`); qm, qS fixed.  With nsum/bsz (a shard of a minibatch of bsz rows)
        the shard's share sum_n a_n / bsz is returned instead (no KL term)."""
        with torch.no_grad():
            qm, qS = self.standard_variational_params()
            qm, qS = qm.detach(), qS.detach()
        an = self.compute_batch_an(xbatch, ybatch, noise_std_batch, qm=qm, qS=qS, Knm=Knm,
                                   Knn_diag=Knn_diag, kn=kn)
        if bsz is not None:
            # a_n may be the reference's (n, n) broadcast (per-observation noise): its mean
            # equals the mean of the per-row values, so mean * n is the shard's sum
            return torch.mean(an) * nsum / bsz
        return torch.mean(an) - self.get_kl_to_prior(qm, qS) / self.N

    def predict(self, x, integrated_obs=False, semi_integrated_estimator="analytic",
                semi_integrated_samps=10, maxiter_cg=50, Kmm=None, fused=None, streamed=None):
        """E[f(x)] and sd[f(x)] (`hipgp.py:416-446`), returned on the CPU.

        fused=True takes kn.qm, |kn|^2 and kn^2.qS straight from the R^T pass (hgp_rt_stats) where
        the family has them (`predict_stats`), so the (bsz, M') kn and its temporaries are never
        allocated; families without it take the materialised path.  None reads HGP_PREDICT_FUSED
        (default off).

        streamed=True is the block family's route (`streamed_predict_stats`, hgp_rt_block_stats: kn
        held one piece of right-hand sides at a time), tried first; a family without it proceeds as
        if the keyword were off.  None reads HGP_BLOCK_STREAMED (default off)."""
        if fused is None:
            fused = os.environ.get("HGP_PREDICT_FUSED", "0") not in ("", "0")
        if streamed is None:
            streamed = os.environ.get("HGP_BLOCK_STREAMED", "0") not in ("", "0")
        x = x.to(self.xgrids[0].device)
        Knm, Knn_diag = self._make_grams(x, integrated_obs=integrated_obs,
                                         semi_integrated_estimator=semi_integrated_estimator,
                                         semi_integrated_samps=semi_integrated_samps)
        out3 = self.streamed_predict_stats(Knm, maxiter_cg=maxiter_cg, Kmm=Kmm) if streamed else None
        if out3 is None and fused:
            out3 = self.predict_stats(Knm, maxiter_cg=maxiter_cg, Kmm=Kmm)
        if out3 is not None:
            qm, _ = self.standard_variational_params()
            mu = out3[:, 0].reshape(-1, *qm.shape[1:])
            ktilde = (Knn_diag - out3[:, 1]).clamp_min(1e-5)
            sig = torch.sqrt(ktilde + out3[:, 2])[:, None]
            return mu.cpu().detach(), sig.cpu().detach()
        kn = self.compute_kn(Knm, maxiter_cg=maxiter_cg, Kmm=Kmm)
        qm, qS = self.standard_variational_params()
        mu = kn.matmul(qm)
        ktilde = (Knn_diag - torch.sum(kn * kn, dim=-1)).clamp_min(1e-5)
        sig = torch.sqrt(ktilde + self.compute_knSkn(kn, qS))[:, None]
        return mu.cpu().detach(), sig.cpu().detach()

    # ---- the posterior mean and draws at any number of points from ONE solve -------------------
    # kn(x).v = Knm(x) K^-1 R v = sum_j k(x, u_j) alpha_j with alpha = K^-1 R v an M-vector that
    # does not depend on x: one single-RHS solve, then a product with Knm that never stores it
    # (hgp_kuf_*_matvec).  `predict` solves once per point (`hipgp.py:416-446`); it stays as it is
    # and still owns the predictive sd, which needs those solves.
    _NO_MEAN_WEIGHTS = ("mean_weights / predict_mean / predict_draws / fit_mean need whitened_type='ziggy': they "
                        "solve with the Toeplitz operators (K alpha = R v; (K + Kuf^T Sigma^-1 Kuf) beta = "
                        "Kuf^T Sigma^-1 y, qm = R^T beta), and cholesky whitening has no circulant R")

    def variational_draws(self, n, eps=None, generator=None):
        """(n, M') rows v_s = qm + S^{1/2} eps_s of the whitened variational posterior on the device;
        eps (n, M') standard normal draws (given, for reproducibility, or from torch.randn with
        `generator`).  The family supplies S^{1/2}."""
        raise NotImplementedError

    def _draw_eps(self, n, eps, generator):
        dev = self.xgrids[0].device
        if eps is None:
            return torch.randn((int(n), self.Mprime), generator=generator, dtype=self.dtype, device=dev)
        if tuple(eps.shape) != (int(n), self.Mprime):
            raise ValueError(f"eps must be (n, M') = ({int(n)}, {self.Mprime}), got {tuple(eps.shape)}")
        return eps.detach().to(device=dev, dtype=self.dtype, copy=True)         # the caller's eps stays

    def mean_weights(self, v=None, maxiter_cg=50, tol=1e-8, Kmm=None):
        """alpha = K^-1 R v as (nv, M) rows on the device, no graph: one `_matmul_by_R` and one
        preconditioned solve of nv right-hand sides (in place where `inv_matmul_` allows).  v: (nv, M')
        rows, an M'-vector or an (M', 1) column in the whitened space; None means qm.  The rows
        depend on the model state only, so a caller may keep them across `predict_mean` calls."""
        if self.whitened_type != 'ziggy':
            raise NotImplementedError(self._NO_MEAN_WEIGHTS)
        with torch.no_grad():
            if Kmm is None:
                Kmm = self.toeplitz()
            if v is None:
                v = self.standard_variational_params()[0]
            v = v.detach()
            if v.dim() == 1 or tuple(v.shape) == (self.Mprime, 1):
                v = v.reshape(1, -1)
            if v.dim() != 2 or v.shape[1] != self.Mprime:
                raise ValueError(f"v must be (nv, M') rows with M' = {self.Mprime}, got {tuple(v.shape)}")
            nv = v.shape[0]
            rows = v.to(device=self.xgrids[0].device, dtype=self.dtype).contiguous()
            if hasattr(Kmm, "set_batch_shape"):
                Kmm.set_batch_shape((nv,))
            b = Kmm._matmul_by_R(rows).reshape(nv, self.M)
            return self._solve_rows(Kmm, b, maxiter_cg, tol)

    @staticmethod
    def _solve_rows(Kmm, b, maxiter_cg, tol):
        """K^-1 b for (nv, M) rows b, no graph: in place of b where `inv_matmul_` allows."""
        if hasattr(Kmm, "inv_matmul_") and b.is_contiguous() and not Kmm.column.requires_grad:
            return Kmm.inv_matmul_(b, do_precond=True, maxiter=maxiter_cg, tol=tol)
        return Kmm.inv_matmul(b, do_precond=True, maxiter=maxiter_cg, tol=tol)

    # ---- the windowed Kuf products: a kernel far shorter than the grid ----------------------------
    # With a support tolerance (the `support_tol` argument where a method has one, else the
    # attribute `kuf_support_tol`, else env HGP_KUF_SUPPORT_TOL) `_kuf_product` / `_kuf_rproduct`
    # take `kuf.kuf_grid_matvec_win` / `kuf.kuf_grid_rmatvec_win` for point observations, through
    # one `kuf.WindowPlan` per (x, dtype) kept for the length of the public call.  With none set,
    # `self._win` stays None and nothing below changes.
    @contextlib.contextmanager
    def _windowed(self, support_tol, integrated_obs):
        tol = self._kuf_support_tol(support_tol)
        if tol is not None and integrated_obs:
            raise NotImplementedError("a support tolerance with integrated_obs=True: the window of a line integral is "
                                      "a tube around the segment and is not built; unset support_tol / "
                                      "kuf_support_tol / HGP_KUF_SUPPORT_TOL for line-integral observations")
        prev = getattr(self, "_win", None)
        self._win = None if tol is None else {"tol": tol, "plans": {}}
        try:
            yield
        finally:
            self._win = prev

    # Line integrals have a knob of their own: the attribute `kuf_line_support_tol`, else env
    # HGP_KUF_LINE_SUPPORT_TOL.  With it set `_kuf_product` / `_kuf_rproduct` take the windowed line
    # products of `hipgp_amd.kuf` for integrated_obs=True ("analytic" and "mc-biased"), through one
    # `kuf.LineWindowPlan` per (x, dtype) kept for the length of the public call; where the plan
    # declines the dense route runs.  Unset, `self._lwin` stays None and nothing changes.
    def _kuf_line_support_tol(self):
        tol = getattr(self, "kuf_line_support_tol", None)
        if tol is None:
            env = os.environ.get("HGP_KUF_LINE_SUPPORT_TOL", "")
            tol = float(env) if env not in ("", "0") else None
        if tol is None:
            return None
        tol = float(tol)
        if not (0. < tol < 1.):
            raise ValueError(f"the line support tolerance must lie in (0, 1), got {tol}")
        return tol

    @contextlib.contextmanager
    def _line_windowed(self, integrated_obs=True):
        tol = self._kuf_line_support_tol() if integrated_obs else None
        prev = getattr(self, "_lwin", None)
        self._lwin = None if tol is None else {"tol": tol, "plans": {}}
        try:
            yield
        finally:
            self._lwin = prev

    def _line_window_plan(self, x, params):
        """The call's `kuf.LineWindowPlan` for the lines x (one per x and dtype), or None: no line
        tolerance is set, or the plan declines (the dense route then runs as before)."""
        win = getattr(self, "_lwin", None)
        if win is None or not torch.is_tensor(x) or x.device.type != "cuda":
            return None
        from hipgp_amd import kuf
        key = (x.data_ptr(), tuple(x.shape), x.dtype)
        if key not in win["plans"]:
            win["plans"][key] = (kuf.LineWindowPlan.make(self.kernel, self.xgrids, x, params, win["tol"]), x)
        return win["plans"][key][0]

    def _window_plan(self, x, params):
        """The call's `kuf.WindowPlan` for the points x (one per x and dtype), or None: no tolerance
        is set, or the plan declines (the dense route then runs as before)."""
        win = getattr(self, "_win", None)
        if win is None:
            return None
        from hipgp_amd import kuf
        key = (x.data_ptr(), tuple(x.shape), x.dtype)
        if key not in win["plans"]:
            # x is kept with the plan so that its address stays its own while the key lives
            win["plans"][key] = (kuf.WindowPlan.make(self.kernel, self.xgrids, x, params, win["tol"]), x)
        return win["plans"][key][0]

    def _kuf_product(self, x, W, integrated_obs, estimator, samps, mc_offset, batch_size):
        """Knm(x) W^T, (N, nw) on the device, for weight rows W (nw, M): the fused products of
        `hipgp_amd.kuf` where they apply (Knm never stored), else `_make_grams(piece)[0] @ W^T` over
        pieces of `batch_size` points (None: a piece whose Knm stays under 256 MiB) -- every kernel,
        the "numerical" estimator and CPU stand-ins take that route."""
        from hipgp_amd import kuf
        self._check_ard_lines(integrated_obs)
        params = self.get_kernel_params()
        out = None
        plan = None if integrated_obs else self._window_plan(x, params)
        lplan = self._line_window_plan(x, params) if integrated_obs else None
        if plan is not None:
            out = kuf.kuf_grid_matvec_win(plan, W)
        elif lplan is not None and estimator == "analytic" and lplan.kind == 0:
            out = kuf.kuf_semi_sqexp_matvec_win(lplan, W)
        elif lplan is not None and estimator == "mc-biased":
            out = kuf.kuf_semi_mc_matvec_win(lplan, W, samps, u=mc_offset)
        elif not integrated_obs:
            out = kuf.kuf_grid_matvec(self.kernel, self.xgrids, x, params, W)
        elif estimator == "analytic":
            out = kuf.kuf_semi_sqexp_matvec(self.kernel, self.xgrids, x, params, W)
        elif estimator == "mc-biased":
            out = kuf.kuf_semi_mc_matvec(self.kernel, self.xgrids, x, params, samps, u=mc_offset, W=W)
        if out is not None:
            return out
        if batch_size is None:
            batch_size = max(1, (256 << 20) // (self.M * x.element_size()))
        pieces = [self._make_grams(x[a:a + batch_size], integrated_obs=integrated_obs,
                                   semi_integrated_estimator=estimator, semi_integrated_samps=samps,
                                   mc_offset=mc_offset)[0].matmul(W.t())
                  for a in range(0, x.shape[0], int(batch_size))]
        return torch.cat(pieces, dim=0) if pieces else W.new_zeros((0, W.shape[0]))

    def predict_mean(self, x, integrated_obs=False, semi_integrated_estimator="analytic",
                     semi_integrated_samps=10, maxiter_cg=50, Kmm=None, weights=None, batch_size=None,
                     mc_offset=None):
        """E[f(x)] alone, on the CPU and shaped like `predict`'s mu, from one single-RHS solve
        however many points x holds: kn(x).qm = Knm(x) alpha, alpha = `mean_weights()` (or the
        caller's `weights`, kept from an earlier call), the product by `_kuf_product`.  The sd is
        not available this way (it needs kn itself): use `predict`.  With the "mc-biased" estimator
        and no `mc_offset` the fused product draws one offset for all of x, the fallback one per
        piece, as `_make_grams` would.

        With a support tolerance t (the model's `kuf_support_tol`, else env HGP_KUF_SUPPORT_TOL; see
        `kuf.support_radius`) point observations take the windowed product: every point sums only the
        nodes within the kernel's reach, and the mean moves by at most t sig2 sum_j |alpha_j|.  With
        integrated_obs=True a tolerance raises NotImplementedError."""
        if self.whitened_type != 'ziggy':
            raise NotImplementedError(self._NO_MEAN_WEIGHTS)
        self._check_ard_lines(integrated_obs)
        with torch.no_grad(), self._windowed(None, integrated_obs), self._line_windowed(integrated_obs):
            x = x.to(self.xgrids[0].device)
            if weights is None:
                weights = self.mean_weights(maxiter_cg=maxiter_cg, Kmm=Kmm)
            mu = self._kuf_product(x, weights.reshape(-1, self.M)[:1], integrated_obs, semi_integrated_estimator,
                                   semi_integrated_samps, mc_offset, batch_size)
            return mu.reshape(-1, 1).cpu().detach()

    # ---- the optimal variational mean of ALL observations from one matrix-free solve -------------
    # m* = (I + sum_n iv_n kn_n kn_n^T)^-1 sum_n iv_n y_n kn_n (`batch_solve`) equals R^T beta with
    #   (K + Kuf^T diag(iv) Kuf) beta = Kuf^T (iv o y)
    # by the push-through identity and R R^T = K: one SPD M x M system whose operator is a K
    # matvec, a product Kuf p (hgp_kuf_*_matvec) and a product Kuf^T c (hgp_kuf_*_rmatvec); no kn,
    # no per-observation solve, no dense M' x M' matrix.  beta is also the weight row
    # `predict_mean(x, weights=...)` takes: K^-1 R qm = K^-1 R R^T beta = beta.
    _FIT_MEAN_SWEEPS = 4      # fp32 models: sweeps of the recurrence between fp64 residuals (`fit_mean`)

    def _kuf_rproduct(self, x, C, integrated_obs, estimator, samps, mc_offset, batch_size):
        """C Knm(x), (nc, M) on the device, for coefficient rows C (nc, N): the twin of
        `_kuf_product`.  The fused products of `hipgp_amd.kuf` where they apply (Knm never stored),
        else the sum of `C[:, piece] @ _make_grams(piece)[0]` over pieces of `batch_size`
        observations (None: a piece whose Knm stays under 256 MiB)."""
        from hipgp_amd import kuf
        self._check_ard_lines(integrated_obs)
        params = self.get_kernel_params()
        out = None
        plan = None if integrated_obs else self._window_plan(x, params)
        lplan = self._line_window_plan(x, params) if integrated_obs else None
        if plan is not None:
            out = kuf.kuf_grid_rmatvec_win(plan, C)
        elif lplan is not None and estimator == "analytic" and lplan.kind == 0:
            out = kuf.kuf_semi_sqexp_rmatvec_win(lplan, C)
        elif lplan is not None and estimator == "mc-biased":
            out = kuf.kuf_semi_mc_rmatvec_win(lplan, C, samps, u=mc_offset)
        elif not integrated_obs:
            out = kuf.kuf_grid_rmatvec(self.kernel, self.xgrids, x, params, C)
        elif estimator == "analytic":
            out = kuf.kuf_semi_sqexp_rmatvec(self.kernel, self.xgrids, x, params, C)
        elif estimator == "mc-biased":
            out = kuf.kuf_semi_mc_rmatvec(self.kernel, self.xgrids, x, params, samps, u=mc_offset, C=C)
        if out is not None:
            return out
        if batch_size is None:
            batch_size = max(1, (256 << 20) // (self.M * x.element_size()))
        out = C.new_zeros((C.shape[0], self.M))
        for a in range(0, x.shape[0], int(batch_size)):
            Knm = self._make_grams(x[a:a + batch_size], integrated_obs=integrated_obs,
                                   semi_integrated_estimator=estimator, semi_integrated_samps=samps,
                                   mc_offset=mc_offset)[0]
            out += C[:, a:a + batch_size].matmul(Knm)
        return out

    def fit_mean(self, xobs, yobs, noise_std=None, integrated_obs=False, semi_integrated_estimator="analytic",
                 semi_integrated_samps=10, maxiter=1000, tol=1e-6, Kmm=None, mc_offset=None, batch_size=None,
                 update=True, callback=None):
        """The ELBO-optimal variational mean for all observations at once, `batch_solve`'s
        m* = (I + sum_n iv_n kn_n kn_n^T)^-1 sum_n iv_n y_n kn_n, as qm = R^T beta with

            (K + Kuf^T diag(iv) Kuf) beta = Kuf^T (iv o y),

        solved matrix-free by C^-1-preconditioned CG from beta = 0 (one K matvec, one `_kuf_product`
        and one `_kuf_rproduct` per iteration; neither kn nor Knm is stored on the fused route, and
        no M' x M' matrix).  iv = 1 / noise_std^2 per observation when given, else exp(-log_noise2).
        The optimum does not depend on the variational covariance, which is left alone.

        Stops when |r| < tol |b| or after `maxiter` iterations; `callback(it, relres)` is called
        each iteration.  An fp32 model on the device runs up to 4 such sweeps: beta, b and the
        residual between sweeps are fp64 (one fp64 application of the operator per sweep, on an fp64
        plan built here), each sweep is the fp32 recurrence on the fp64 residual, and it ends when
        that residual is under tol |b| or `maxiter` iterations are spent in all; R^T is applied in
        fp64.  Without this the fp32 recurrence stalls near eps cond(A) and the mean is 1e-3 off.  With the "mc-biased" estimator and no `mc_offset` one offset is drawn here
        and used for every product: CG needs one fixed symmetric operator.

        Returns MeanFit(weights, qm, iters, relres): weights = beta as a (1, M) device row, what
        `predict_mean(x, weights=...)` takes (K^-1 R qm = beta); qm = R^T beta (M', 1); relres the
        recurrence's last |r| / |b|.  update=True writes the mean into the model as `batch_solve`
        does (theta1 = lam qm with lam = -2 theta2 as it stands, or global_m = qm).

        With a support tolerance t (the model's `kuf_support_tol`, else env HGP_KUF_SUPPORT_TOL) and
        point observations both Kuf products are the windowed ones, exact transposes of each other on
        one `kuf.WindowPlan` built here once (the fp64 refinement builds its own on the fp64 points,
        with the same radius): the system solved is the one with Kuf replaced by its windowed part,
        every entry of which is within t sig2 of the dense one.  With integrated_obs=True a tolerance
        raises NotImplementedError."""
        if self.whitened_type != 'ziggy':
            raise NotImplementedError(self._NO_MEAN_WEIGHTS)
        self._check_ard_lines(integrated_obs)
        with torch.no_grad(), self._windowed(None, integrated_obs), self._line_windowed(integrated_obs):
            dev = self.xgrids[0].device
            if Kmm is None:
                Kmm = self.toeplitz()
            x = xobs.to(dev)
            y = yobs.to(device=dev, dtype=self.dtype).reshape(-1)
            if noise_std is not None:
                iv = 1 / noise_std.to(device=dev, dtype=self.dtype).reshape(-1) ** 2
            else:
                iv = torch.exp(-self.log_noise2).detach().to(dev).expand(y.shape[0])
            if integrated_obs and semi_integrated_estimator == "mc-biased" and mc_offset is None:
                mc_offset = torch.rand(1, dtype=self.kernel.dtype, device=dev)      # kernels.py:28-29
            route = (integrated_obs, semi_integrated_estimator, semi_integrated_samps, mc_offset, batch_size)
            if hasattr(Kmm, "set_batch_shape"):
                Kmm.set_batch_shape((1,))

            def operator(Kop, xx, ivv):
                def A(p):
                    f = self._kuf_product(xx, p, *route).reshape(-1)
                    return Kop._matmul_by_K(p).reshape(1, self.M) + self._kuf_rproduct(xx, (ivv * f)[None, :], *route)
                return A

            A = operator(Kmm, x, iv)
            # fp32 on the device: the recurrence alone stalls near eps * cond(A), and R^T turns that
            # into 1e-3 of the mean.  So beta, b and the residual between sweeps are kept in fp64
            # (one fp64 application of the operator per sweep, on a second plan); the iterations stay fp32.
            refine = self.dtype == torch.float32 and dev.type == 'cuda'
            if refine:
                kparams = self.get_kernel_params()
                K64 = ToeplitzTensor(xgrids=[g.double() for g in self.xgrids],
                                     kernel=lambda a, c: self.kernel(a, c, params=kparams), batch_shape=None,
                                     jitter_val=self.jitter_val)
                K64.set_batch_shape((1,))
                x64, iv64 = x.double(), iv.double()
                A64 = operator(K64, x64, iv64)
                b = self._kuf_rproduct(x64, (iv64 * y.double())[None, :], *route)
            else:
                b = self._kuf_rproduct(x, (iv * y)[None, :], *route)
            beta = torch.zeros_like(b)
            bnorm = float(torch.linalg.vector_norm(b))
            it, relres = 0, 0.0
            if bnorm > 0:
                relres = 1.0
                rtrue = b
                for _ in range(self._FIT_MEAN_SWEEPS if refine else 1):
                    # one sweep: PCG on A d = rtrue from d = 0, until |r| < tol |b|
                    r = rtrue.to(self.dtype).clone()
                    d = torch.zeros_like(r)
                    z = Kmm._matmul_by_Cinv(r).reshape(1, self.M)
                    p = z.clone()
                    rz = torch.sum(r * z)
                    while it < maxiter:
                        Ap = A(p)
                        alpha = rz / torch.sum(p * Ap)
                        d += alpha * p
                        r -= alpha * Ap
                        it += 1
                        relres = float(torch.linalg.vector_norm(r)) / bnorm
                        if callback is not None:
                            callback(it, relres)
                        if relres < tol:
                            break
                        z = Kmm._matmul_by_Cinv(r).reshape(1, self.M)
                        rz_new = torch.sum(r * z)
                        p = z + (rz_new / rz) * p
                        rz = rz_new
                    beta += d.to(beta.dtype)
                    if not refine or it >= maxiter:
                        break
                    rtrue = b - A64(beta)
                    if float(torch.linalg.vector_norm(rtrue)) < tol * bnorm:
                        break
            if refine:
                qm = K64._matmul_by_RT(beta).reshape(self.Mprime, 1).to(self.dtype)
                beta = beta.to(self.dtype)
            else:
                qm = Kmm._matmul_by_RT(beta).reshape(self.Mprime, 1)
            if update:
                if self.parameterization == 'standard':
                    self.global_m.data[:] = qm
                else:
                    lam = -2 * self.global_theta2.data
                    if self.name == 'mean-field':
                        self.global_theta1.data[:] = lam * qm
                    else:
                        self.global_theta1.data[:] = self.block_diag_multiply(lam, qm.t()).t()
            return MeanFit(beta, qm, it, relres)

    def predict_draws(self, x, n, eps=None, generator=None, integrated_obs=False,
                      semi_integrated_estimator="analytic", semi_integrated_samps=10, maxiter_cg=50, Kmm=None,
                      batch_size=None, mc_offset=None):
        """n joint draws at the points x, (n, N) on the CPU: kn(x).v_s for v_s = qm + S^{1/2} eps_s
        (`variational_draws`; eps (n, M') makes them reproducible), from one solve of n right-hand
        sides and one fused product with n weight rows.

        These are draws of the PROJECTED process K_xu K^-1 u with u = R v the inducing values: their
        mean is `predict`'s mean and their variance is the kn S kn term of its variance.  They
        exclude the residual `ktilde` = Knn - |kn|^2 that `predict`'s sd adds, so between inducing
        points they are smoother and narrower than draws of f itself.

        A support tolerance (`kuf_support_tol` / HGP_KUF_SUPPORT_TOL) windows the product as in
        `predict_mean`."""
        if self.whitened_type != 'ziggy':
            raise NotImplementedError(self._NO_MEAN_WEIGHTS)
        self._check_ard_lines(integrated_obs)
        with torch.no_grad(), self._windowed(None, integrated_obs), self._line_windowed(integrated_obs):
            x = x.to(self.xgrids[0].device)
            v = self.variational_draws(n, eps=eps, generator=generator)
            alpha = self.mean_weights(v, maxiter_cg=maxiter_cg, Kmm=Kmm)
            out = self._kuf_product(x, alpha, integrated_obs, semi_integrated_estimator, semi_integrated_samps,
                                    mc_offset, batch_size)
            return out.t().contiguous().cpu().detach()

    # ---- joint draws of f itself at any points: pathwise conditioning -------------------------------
    # Matheron's rule with a random-Fourier-feature prior.  A draw of the prior everywhere,
    #   f_prior(x) = sqrt(2 sig2 / F) sum_f w_f cos(omega_f . x + b_f),
    # is corrected at the inducing points from its own values u_prior = f_prior(U) + sqrt(jitter) xi to
    # a draw u = R v of the variational posterior:
    #   f(x) = f_prior(x) + sum_j k(x, u_j) alpha_j,   alpha = K^-1 (u - u_prior).
    # Its covariance is k(x, x') - k_xU K^-1 k_Ux' + k_xU K^-1 R S R^T K^-1 k_Ux': `predict`'s variance,
    # ktilde included, up to the feature error of the prior.  Per draw: one right-hand side of the
    # batched solve, one row of the fused Kuf product and one row of the fused feature product
    # (hgp_rff_matvec), which also runs once on the whole mesh to form the right-hand side.
    def _rff_product(self, x, omega, phase, W, scale, transposed=False, out=None, beta=0.0, line=False):
        """scale * cos(p omega^T + phase) W^T for weight rows W (nw, F), (npoints, nw) or transposed
        (nw, npoints), accumulated into `out` with beta = 1: the part `_kuf_product` plays for Kuf.
        The points are x, or the inducing mesh when x is None.  The fused product of `hipgp_amd.rff`
        where it applies (the features never stored), else torch over pieces of points whose
        (piece, F) features stay under 256 MiB -- CPU stand-ins take that route.

        line=True: the features are integrated along the segments from the origin to the rows of x
        (`rff.rff_line_matvec`, in torch `rff.line_features`); x must be given."""
        from hipgp_amd import rff
        if line:
            if x is None:
                raise TypeError("the line-integral feature product takes explicit rows x (no mesh mode)")
            res = rff.rff_line_matvec(omega, phase, W, x, scale=scale, transposed=transposed, out=out, beta=beta)
            pts = x
        elif x is None:
            res = rff.rff_matvec(omega, phase, W, xgrids=self.xgrids, scale=scale, transposed=transposed, out=out,
                                 beta=beta)
            pts = self.xinduce
        else:
            res = rff.rff_matvec(omega, phase, W, x=x, scale=scale, transposed=transposed, out=out, beta=beta)
            pts = x
        if res is not None:
            return res
        piece = max(1, (256 << 20) // (omega.shape[0] * pts.element_size()))
        if line:
            feats = lambda p: rff.line_features(omega, phase, p)
        else:
            feats = lambda p: torch.cos(p.matmul(omega.t()) + phase)
        cols = [scale * W.matmul(feats(pts[a:a + piece]).t())
                for a in range(0, pts.shape[0], piece)]
        acc = torch.cat(cols, dim=1) if cols else W.new_zeros((W.shape[0], 0))         # (nw, npoints)
        if not transposed:
            acc = acc.t()
        if out is None:
            return acc.contiguous()
        return out.mul_(beta).add_(acc) if beta != 0 else out.copy_(acc)

    def predict_samples(self, x, n, nfeat=4096, eps=None, features=None, prior_w=None, nugget_eps=None,
                        generator=None, maxiter_cg=50, Kmm=None, integrated_obs=False, support_tol=None):
        """n joint draws of f ITSELF at the points x, (n, N) on the CPU like `predict_draws`, by
        pathwise conditioning: f(x) = f_prior(x) + Knm(x) K^-1 (R v - f_prior(U) - sqrt(jitter) xi)
        with f_prior a random-Fourier-feature draw of the prior and v = qm + S^{1/2} eps
        (`variational_draws`).  Unlike `predict_draws` the draws carry the residual ktilde = Knn -
        |kn|^2: their mean is `predict`'s mean and their variance `predict`'s variance.

        One solve of n right-hand sides, one fused Kuf product and two fused feature products (on
        the inducing mesh for the right-hand side, at x for the result); nothing of size (N, F),
        (M, F) or (N, M) is stored on the device route.

        ONE feature set (omega, b), `nfeat` features, is shared by all n draws of a call: the prior
        covariance the draws see differs from k by O(nfeat^-1/2), and that error does not average
        out over the draws of a call (it does over calls with fresh features).

        Every random input can be given, which makes a call reproducible: eps (n, M') for the
        variational draw, features = (omega (F, ndim), phase (F)) in radians as
        `hipgp_amd.rff.spectral_features` returns them, prior_w (n, F) and nugget_eps (n, M)
        standard normal.  What is not given is drawn with `generator`.  Point observations and
        whitened_type='ziggy' only (integrated_obs=True raises: the feature prior is a prior of point
        values); SqExp and Matern kernels with a scalar ell, SqExp also with one ell per axis (no
        Gneiting).

        support_tol (None: the model's `kuf_support_tol`, else env HGP_KUF_SUPPORT_TOL) windows the
        Kuf product alone, as in `predict_mean`; the feature products are unchanged."""
        if self.whitened_type != 'ziggy':
            raise NotImplementedError(self._NO_MEAN_WEIGHTS)
        if integrated_obs:
            raise NotImplementedError("predict_samples draws f at points: the random-Fourier-feature prior has no "
                                      "line-integral form here (integrated_obs=True); use predict_draws for the "
                                      "projected process of line integrals")
        from hipgp_amd import rff
        with torch.no_grad():
            dev = self.xgrids[0].device
            n = int(n)
            x = x.to(device=dev, dtype=self.dtype)
            params = self.get_kernel_params()
            if features is None:
                features = rff.spectral_features(self.kernel, params, len(self.xgrids), nfeat, generator=generator,
                                                 device=dev, dtype=torch.float64)
            omega, phase = (t.detach().to(device=dev, dtype=torch.float64) for t in features)
            F = omega.shape[0]
            if omega.dim() != 2 or omega.shape[1] != len(self.xgrids) or tuple(phase.shape) != (F,) or F < 1:
                raise ValueError(f"features must be (omega (F, {len(self.xgrids)}), phase (F,)), got "
                                 f"{tuple(omega.shape)} and {tuple(phase.shape)}")

            def normal(t, shape, name):
                if t is None:
                    return torch.randn(shape, generator=generator, dtype=self.dtype, device=dev)
                if tuple(t.shape) != shape:
                    raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
                return t.detach().to(device=dev, dtype=self.dtype)

            v = self.variational_draws(n, eps=eps, generator=generator)
            W = normal(prior_w, (n, F), "prior_w").contiguous()
            xi = normal(nugget_eps, (n, self.M), "nugget_eps")
            if x.device.type != "cuda":          # the torch route evaluates the features in the model dtype
                omega, phase = omega.to(self.dtype), phase.to(self.dtype)
            scale = float(torch.sqrt(2 * torch.as_tensor(params[0]).detach().double() / F))
            if Kmm is None:
                Kmm = self.toeplitz()
            if hasattr(Kmm, "set_batch_shape"):
                Kmm.set_batch_shape((n,))
            b = Kmm._matmul_by_R(v.contiguous()).reshape(n, self.M)
            b = b.contiguous().sub_(xi, alpha=float(np.sqrt(self.jitter_val)))
            b = self._rff_product(None, omega, phase, W, -scale, transposed=True, out=b, beta=1.0)
            alpha = self._solve_rows(Kmm, b, maxiter_cg, 1e-8)
            with self._windowed(support_tol, False):
                out = self._kuf_product(x, alpha, False, "analytic", 10, None, None).contiguous()
            out = self._rff_product(x, omega, phase, W, scale, out=out, beta=1.0)
            return out.t().contiguous().cpu().detach()

    # ---- joint draws of line integrals: the same rule with the features integrated ---------------
    # The line integral F(x) = |x| int_0^1 f(a x) da of the prior draw above has a closed form per feature,
    #   |x| int_0^1 cos(a T + b) da = |x| cos(b + T / 2) sinc(T / 2),   T = omega . x,
    # and the correction term integrates to sum_j k_semi(u_j, x) alpha_j with the SAME alpha: the
    # right-hand side is point values on the mesh, unchanged.  F at lines and f at points of one draw
    # share v, W, xi and alpha.
    def predict_line_samples(self, x, n, xpoint=None, nfeat=4096, eps=None, features=None, prior_w=None,
                             nugget_eps=None, generator=None, maxiter_cg=50, Kmm=None,
                             semi_integrated_estimator="analytic", semi_integrated_samps=10, mc_offset=None,
                             batch_size=None):
        """n joint draws of the LINE INTEGRALS F(x_i) = |x_i| int_0^1 f(a x_i) da of f to the rows of x,
        (n, N) on the CPU, by the pathwise conditioning of `predict_samples`:
        F(x) = F_prior(x) + Knm_semi(x) alpha with alpha = K^-1 (R v - f_prior(U) - sqrt(jitter) xi)
        exactly as there (point values on the mesh), F_prior the exact line integral of the same
        random-Fourier-feature draw (`hipgp_amd.rff.rff_line_matvec`, closed form per feature) and
        Knm_semi the line-integral cross-covariance of `predict(integrated_obs=True)`.  Unlike
        `predict_draws(integrated_obs=True)` the draws carry the residual ktilde.

        With xpoint (Np, ndim) the result is the pair (lines (n, N), points (n, Np)): draws of f at
        xpoint FROM THE SAME DRAWS (the same v, W, xi and alpha, one solve), equal to what
        `predict_samples(xpoint, n, ...)` returns for the same random inputs.

        One solve of n right-hand sides, the fused semi-integrated Kuf product, the fused feature
        product on the mesh and the fused line feature product (plus the two point products with
        xpoint); nothing of size (N, F), (M, F) or (N, M) is stored on the device route.

        The feature prior is always the EXACT line integral; the cross-covariance is the caller's
        estimator.  "analytic" (SqExp) is exact too.  With "mc-biased" (the only route for Matern;
        `semi_integrated_samps` nodes, offset `mc_offset` or one drawn per call) the draws' mean is
        `predict_mean`'s with that estimator, and their variance exceeds the exact one by the
        second-order term (k~ - k)^T K^-1 (k~ - k), k~ the estimated and k the exact line-integral
        cross-covariance: the prior and the correction no longer cancel exactly at the inducing points.

        Random inputs (eps, features, prior_w, nugget_eps, generator) and the one shared feature
        set per call as in `predict_samples`.  whitened_type='ziggy' only; SqExp and Matern kernels
        with a scalar ell (no Gneiting, no ARD: one ell per axis raises NotImplementedError)."""
        if self.whitened_type != 'ziggy':
            raise NotImplementedError(self._NO_MEAN_WEIGHTS)
        self._check_ard_lines(True)
        from hipgp_amd import rff
        with torch.no_grad(), self._line_windowed():
            dev = self.xgrids[0].device
            n = int(n)
            x = x.to(device=dev, dtype=self.dtype)
            if xpoint is not None:
                xpoint = xpoint.to(device=dev, dtype=self.dtype)
            params = self.get_kernel_params()
            if features is None:
                features = rff.spectral_features(self.kernel, params, len(self.xgrids), nfeat, generator=generator,
                                                 device=dev, dtype=torch.float64)
            omega, phase = (t.detach().to(device=dev, dtype=torch.float64) for t in features)
            F = omega.shape[0]
            if omega.dim() != 2 or omega.shape[1] != len(self.xgrids) or tuple(phase.shape) != (F,) or F < 1:
                raise ValueError(f"features must be (omega (F, {len(self.xgrids)}), phase (F,)), got "
                                 f"{tuple(omega.shape)} and {tuple(phase.shape)}")

            def normal(t, shape, name):
                if t is None:
                    return torch.randn(shape, generator=generator, dtype=self.dtype, device=dev)
                if tuple(t.shape) != shape:
                    raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
                return t.detach().to(device=dev, dtype=self.dtype)

            v = self.variational_draws(n, eps=eps, generator=generator)
            W = normal(prior_w, (n, F), "prior_w").contiguous()
            xi = normal(nugget_eps, (n, self.M), "nugget_eps")
            if x.device.type != "cuda":          # the torch route evaluates the features in the model dtype
                omega, phase = omega.to(self.dtype), phase.to(self.dtype)
            scale = float(torch.sqrt(2 * torch.as_tensor(params[0]).detach().double() / F))
            if Kmm is None:
                Kmm = self.toeplitz()
            if hasattr(Kmm, "set_batch_shape"):
                Kmm.set_batch_shape((n,))
            b = Kmm._matmul_by_R(v.contiguous()).reshape(n, self.M)
            b = b.contiguous().sub_(xi, alpha=float(np.sqrt(self.jitter_val)))
            b = self._rff_product(None, omega, phase, W, -scale, transposed=True, out=b, beta=1.0)
            alpha = self._solve_rows(Kmm, b, maxiter_cg, 1e-8)
            out = self._kuf_product(x, alpha, True, semi_integrated_estimator, semi_integrated_samps, mc_offset,
                                    batch_size).contiguous()
            out = self._rff_product(x, omega, phase, W, scale, out=out, beta=1.0, line=True)
            lines = out.t().contiguous().cpu().detach()
            if xpoint is None:
                return lines
            pts = self._kuf_product(xpoint, alpha, False, "analytic", 10, None, None).contiguous()
            pts = self._rff_product(xpoint, omega, phase, W, scale, out=pts, beta=1.0)
            return lines, pts.t().contiguous().cpu().detach()


class MeanFieldToeplitzGP(ToeplitzInducingGP):
    """Diagonal variational covariance in the expanded space (`hipgp.py:449-524`)."""

    def __init__(self, kernel, xgrids, num_obs, sig2_init=1., ell_init=.05, noise2_init=1.,
                 init_Svar=.1, learn_kernel=False, learn_noise=False, dtype=torch.float,
                 whitened_type='ziggy', parameterization='expectation-family', jitter_val=1e-3):
        super().__init__(kernel, xgrids, num_obs, sig2_init=sig2_init, ell_init=ell_init,
                         noise2_init=noise2_init, learn_kernel=learn_kernel, learn_noise=learn_noise,
                         dtype=dtype, whitened_type=whitened_type, parameterization=parameterization,
                         jitter_val=jitter_val)
        col = lambda: torch.zeros(self.Mprime, 1, dtype=dtype)
        if parameterization == 'standard':
            self.global_m = nn.Parameter(nn.init.xavier_normal_(col()), requires_grad=True)
            self.global_S = nn.Parameter(init_Svar * torch.ones(self.Mprime, 1, dtype=dtype), requires_grad=True)
        else:
            self.global_theta1 = nn.Parameter(nn.init.xavier_normal_(col()), requires_grad=True)
            self.global_theta2 = nn.Parameter((-.5 / init_Svar) * torch.ones(self.Mprime, 1, dtype=dtype),
                                              requires_grad=True)

    @property
    def name(self):
        return 'mean-field'

    def standard_variational_params(self):
        if self.parameterization == 'standard':
            return self.global_m, self.global_S
        S = -0.5 / self.global_theta2
        return S * self.global_theta1, S

    def get_kl_to_prior(self, qm=None, qS=None):
        if qm is None or qS is None:
            qm, qS = self.standard_variational_params()
        return diag_kl_to_standard(qm, qS)

    def get_identity_for_lam(self):
        return 1

    def get_lam(self, ivar_noise, kn, bscale=1, add_identity=True):
        return (bscale * torch.sum(ivar_noise * kn * kn, dim=0) + (1 if add_identity else 0))[:, None]

    def get_S_from_lam(self, lam):
        return 1. / lam

    def compute_knSkn(self, kn, qS):
        return torch.sum(kn * kn * qS.t(), dim=-1).squeeze()

    def predict_stats(self, Knm, maxiter_cg=50, Kmm=None):
        """Diagonal S: the three dots are ToeplitzTensor.rt_stats (hgp_rt_stats) on the PCG solution,
        with compute_kn's PCG settings; Knm is consumed (the solve overwrites it where it can).  None,
        with Knm untouched, for cholesky whitening or a Kmm without rt_stats."""
        if self.whitened_type != 'ziggy':
            return None
        if Kmm is None:
            Kmm = self.toeplitz()
        if not hasattr(Kmm, "rt_stats"):
            return None
        with torch.no_grad():
            # Knm is the caller's to consume (predict made it for this call): the solve overwrites it
            # where the tensor allows, so no second (bsz, M) tensor is held beside it
            if hasattr(Kmm, "inv_matmul_") and Knm.is_contiguous() and not Knm.requires_grad \
                    and not Kmm.column.requires_grad:
                d0 = Kmm.inv_matmul_(Knm, do_precond=True, maxiter=maxiter_cg, tol=1e-8)
            else:
                d0 = Kmm.inv_matmul(Knm, do_precond=True, maxiter=maxiter_cg, tol=1e-8)
            qm, qS = self.standard_variational_params()
            return Kmm.rt_stats(d0, qm, qS)

    # ---- the posterior on the whole inducing grid (no reference counterpart: the reference leaves
    # sample() a TODO, `hipgp.py:111-115`, and predicts point by point) ---------------------------
    def _grid_kmm(self, Kmm):
        """`predict_stats`' rule for a caller's Kmm: it must have the operator, else a fresh one."""
        if self.whitened_type != 'ziggy':
            raise NotImplementedError(self._NO_GRID_POSTERIOR)
        if Kmm is None or not hasattr(Kmm, "_matmul_by_Rsq"):
            Kmm = self.toeplitz()
        return Kmm

    def _grid_rows(self, Kmm, t, nrows):
        """t as the (nrows, M') operator input in the model dtype on the grid's device."""
        if hasattr(Kmm, "set_batch_shape"):
            Kmm.set_batch_shape((nrows,))
        return t.detach().reshape(nrows, self.Mprime).to(device=self.xgrids[0].device, dtype=self.dtype).contiguous()

    def grid_posterior(self, prior=False, Kmm=None):
        """(mean, sd) of the variational posterior of the inducing values u on the whole inducing
        grid, device tensors shaped (m_1, ..., m_d), from two operator applications and no solve.

        The whitened family is u = R v, v ~ N(qm, diag qS), so E[u] = R qm (HGP_OP_R) and
        Var[u]_j = sum_k R_jk^2 qS_k = ((R o R) qS)_j (HGP_OP_RSQ: R is the crop of a circulant with
        generator s = IFFT_n(sqrt D), so R o R is the crop of the circulant with generator s^2).
        prior=True: (0, sqrt((R o R) 1)), the prior sd sqrt(K_jj) = sqrt(column[0]) where no
        eigenvalue is clamped.

        This is the posterior of the inducing values u, whose prior covariance is K INCLUDING the
        nugget -- not that of f(x_j), which `predict` computes.  On the grid Knm = K - jitter I, so
        the two means are related exactly by predict_mean(xinduce) = u - jitter K^-1 u, u = R qm."""
        with torch.no_grad():
            Kmm = self._grid_kmm(Kmm)
            dims = tuple(len(g) for g in self.xgrids)
            qm, qS = self.standard_variational_params()
            if prior:
                mean = torch.zeros(dims, dtype=self.dtype, device=self.xgrids[0].device)
                w = torch.ones_like(qS)
            else:
                mean = Kmm._matmul_by_R(self._grid_rows(Kmm, qm, 1)).reshape(dims)
                w = qS
            var = Kmm._matmul_by_Rsq(self._grid_rows(Kmm, w, 1))
            # a sum of non-negative terms; the transforms' rounding can leave -eps where it is ~0
            return mean, torch.sqrt(var.clamp_min(0)).reshape(dims)

    def sample_grid(self, n, prior=False, generator=None, eps=None, Kmm=None):
        """n joint draws of the inducing values on the inducing grid, (n, m_1, ..., m_d) on the
        device: u = R (qm + sqrt(qS) * eps), or R eps with prior=True (one HGP_OP_R of n rows).
        eps (n, M') standard normal draws makes the result reproducible; otherwise they come from
        torch.randn with `generator`, shifted and scaled in place (one (n, M') buffer).  The same
        quantity as `grid_posterior` (u, nugget included), whose mean and sd the draws have."""
        with torch.no_grad():
            Kmm = self._grid_kmm(Kmm)
            dims = tuple(len(g) for g in self.xgrids)
            dev = self.xgrids[0].device
            if eps is None:
                v = torch.randn((int(n), self.Mprime), generator=generator, dtype=self.dtype, device=dev)
            else:
                if tuple(eps.shape) != (int(n), self.Mprime):
                    raise ValueError(f"eps must be (n, M') = ({int(n)}, {self.Mprime}), got {tuple(eps.shape)}")
                v = eps.detach().to(device=dev, dtype=self.dtype, copy=True)     # the caller's eps stays
            if not prior:
                qm, qS = self.standard_variational_params()
                row = lambda t: t.detach().reshape(1, -1).to(device=dev, dtype=self.dtype)
                v.mul_(torch.sqrt(row(qS))).add_(row(qm))
            return Kmm._matmul_by_R(self._grid_rows(Kmm, v, int(n))).reshape(int(n), *dims)

    def variational_draws(self, n, eps=None, generator=None):
        """v_s = qm + sqrt(qS) * eps_s, (n, M') on the device (the rows `sample_grid` applies R to)."""
        with torch.no_grad():
            v = self._draw_eps(n, eps, generator)
            qm, qS = self.standard_variational_params()
            row = lambda t: t.detach().reshape(1, -1).to(device=v.device, dtype=self.dtype)
            return v.mul_(torch.sqrt(row(qS))).add_(row(qm))

    def fit_stats(self, Knm, ybatch, Knn_diag, noise_std_batch=None, maxiter_cg=10, Kmm=None):
        """`batch_stats` of kn = R^T K^-1 Knm^T (`hipgp.py:234-250`) without the (bsz, M') kn:
        d = K^-1 Knm^T by compute_kn's PCG in place of Knm (consumed), the three row dots and
        lam_sum from ToeplitzTensor.rt_fit_stats (hgp_rt_fit_stats) on d, a_n and bdiff_n from the
        dots as in `batch_stats_slab`, and, R^T being linear,
            dm_sum = -sum_n bdiff_n kn_n = R^T (-sum_n bdiff_n d_n):
        one fixed-order (bsz, M) -> (M) column sum (hgp_meanfield_cols on d with Mp = M) and a
        single-RHS R^T.  None, with Knm untouched, for cholesky whitening, an empty batch or a Kmm
        without rt_fit_stats."""
        if self.whitened_type != 'ziggy' or Knm.shape[0] == 0:
            return None
        if Kmm is None:
            Kmm = self.toeplitz()
        if not hasattr(Kmm, "rt_fit_stats"):
            return None
        with torch.no_grad():
            Knm = Knm.detach()
            B = Knm.shape[0]
            dev, dt = Knm.device, Knm.dtype
            if hasattr(Kmm, "inv_matmul_") and Knm.is_contiguous() and not Kmm.column.requires_grad:
                d0 = Kmm.inv_matmul_(Knm, do_precond=True, maxiter=maxiter_cg, tol=1e-8)
            else:
                d0 = Kmm.inv_matmul(Knm, do_precond=True, maxiter=maxiter_cg, tol=1e-8)
            qm, qS = self.standard_variational_params()
            ivar, log_sd = self.noise_terms(noise_std_batch)
            col = lambda v: torch.as_tensor(v, dtype=dt, device=dev).detach().reshape(-1).expand(B).contiguous()
            y, iv, kd, lsd = col(ybatch), col(ivar), col(Knn_diag), col(log_sd)
            qmv = qm.detach().reshape(-1).to(dt).contiguous()
            qSv = qS.detach().reshape(-1).to(dt).contiguous()
            dots, lam = Kmm.rt_fit_stats(d0, qmv, qSv, iv)
            knm, knkn, knSkn = dots[:, 0], dots[:, 1], dots[:, 2]
            an = -0.5 * iv * ((knm - y) ** 2 + kd - knkn + knSkn) - lsd - 0.5 * LN_2PI
            bdiff = (iv * (knm - y)).contiguous()
            if d0.is_cuda:
                import ctypes
                from hipgp_amd import _lib
                p = lambda t: ctypes.c_void_p(t.data_ptr())
                d0 = d0.contiguous()
                M = d0.shape[1]
                scr = torch.empty(M, dtype=dt, device=dev)      # sum_n iv_n d_nj^2: not used
                v = torch.empty(M, dtype=dt, device=dev)
                _lib.check(_lib.lib().hgp_meanfield_cols(_lib.dtype_code(dt), p(d0), B, M, p(iv), p(bdiff), p(scr),
                                                         p(v), _lib.stream_ptr(dev)))
            else:       # CPU tensors only in the host-logic tests
                v = -(bdiff[None, :].matmul(d0)).reshape(-1)
            dm = Kmm._matmul_by_RT(v[None, :]).reshape(-1)
        return {"an_sum": an.sum(), "lam_sum": lam.reshape(-1), "dm_sum": dm, "n": B}

    # ---- natural gradient as batch sums + update (sharding-friendly) ------------------------
    def batch_stats(self, kn, ybatch, Knn_diag, noise_std_batch=None):
        """Sums over this minibatch (or this rank's shard of it):
           an_sum  = sum_n a_n
           lam_sum = sum_n ivar_n kn_n^2            (M',)   `hipgp.py:241`
           dm_sum  = -sum_n ivar_n (kn_n.m - y_n) kn_n   (M',)   `hipgp.py:234-236`"""
        if kn.shape[0] == 0:    # an empty shard of a minibatch (hipgp_amd.dist)
            z = kn.new_zeros(kn.shape[1])
            return {"an_sum": kn.new_zeros(()), "lam_sum": z, "dm_sum": z.clone(), "n": 0}
        with torch.no_grad():
            qm, qS = self.standard_variational_params()
            ivar, log_sd = self.noise_terms(noise_std_batch)
            if kn.is_cuda:      # the device path: two streaming passes of hgp_meanfield_stats
                return self._batch_stats_device(kn, ybatch, Knn_diag, qm, qS, ivar, log_sd)
            # CPU tensors only reach here in the gloo host-logic tests (tests/test_model_cpu.py)
            y = ybatch.reshape(-1)
            knm = kn.matmul(qm).reshape(-1)
            kk = kn * kn
            knkn = kk.sum(dim=-1)
            knSkn = kk.matmul(qS).reshape(-1)
            iv = ivar.reshape(-1) if torch.is_tensor(ivar) and ivar.dim() > 0 else ivar
            lsd = log_sd.reshape(-1) if torch.is_tensor(log_sd) and log_sd.dim() > 0 else log_sd
            an = -0.5 * iv * ((knm - y) ** 2 + Knn_diag.reshape(-1) - knkn + knSkn) - lsd - 0.5 * LN_2PI
            ivcol = iv[:, None] if torch.is_tensor(iv) and iv.dim() > 0 else iv
            lam_sum = torch.sum(ivcol * kk, dim=0)
            bdiff = iv * (knm - y)
            dm_sum = -(bdiff[None, :].matmul(kn)).reshape(-1)
            an_sum = an.sum()
        return {"an_sum": an_sum, "lam_sum": lam_sum, "dm_sum": dm_sum, "n": kn.shape[0]}

    def _batch_stats_device(self, kn, ybatch, Knn_diag, qm, qS, ivar, log_sd):
        import ctypes
        from hipgp_amd import _lib
        B, Mp = kn.shape
        dev, dt = kn.device, kn.dtype
        col = lambda v: torch.as_tensor(v, dtype=dt, device=dev).reshape(-1).expand(B).contiguous()
        knc = kn.detach().contiguous()
        qmv = qm.detach().reshape(-1).to(dt).contiguous()
        qSv = qS.detach().reshape(-1).to(dt).contiguous()
        y, iv, kd, lsd = col(ybatch), col(ivar), col(Knn_diag), col(log_sd)
        an = torch.empty(B, dtype=dt, device=dev)
        lam = torch.empty(Mp, dtype=dt, device=dev)
        dm = torch.empty(Mp, dtype=dt, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(_lib.lib().hgp_meanfield_stats(_lib.dtype_code(dt), p(knc), B, Mp, p(qmv), p(qSv), p(y), p(iv),
                                                  p(kd), p(lsd), p(an), p(lam), p(dm), _lib.stream_ptr(dev)))
        return {"an_sum": an.sum(), "lam_sum": lam, "dm_sum": dm, "n": B}

    def batch_stats_slab(self, kn, j0, ybatch, Knn_diag, noise_std_batch=None, reduce=None, lead=True):
        """`batch_stats` of a minibatch whose kn is held in column slabs over ranks (grid-block
        sharding, `hipgp_amd.slab.SlabFit`): kn (B, w) are this rank's expanded-grid columns
        [j0, j0 + w).  The per-observation dots kn.qm, |kn|^2 and kn^2.qS are sums over the
        slabs: this rank's partials (hgp_meanfield_rowdots) go through `reduce` (an in-place SUM
        all-reduce of the (B, 3) tensor, B values per dot), then a_n and the slab's columns of
        lam_sum / dm_sum follow as in `batch_stats` (hgp_meanfield_cols), written into zero
        M'-vectors: summed over the ranks (allreduce_stats) they give the single-process sums.
        an_sum and n are counted on the `lead` rank only, so that sum is not multiplied."""
        B, w = kn.shape
        Mp = self.Mprime
        with torch.no_grad():
            qm, qS = self.standard_variational_params()
            ivar, log_sd = self.noise_terms(noise_std_batch)
            dev, dt = kn.device, kn.dtype
            col = lambda v: torch.as_tensor(v, dtype=dt, device=dev).reshape(-1).expand(B).contiguous()
            qmv = qm.detach().reshape(-1)[j0:j0 + w].to(dt).contiguous()
            qSv = qS.detach().reshape(-1)[j0:j0 + w].to(dt).contiguous()
            knc = kn.detach().contiguous()
            y, iv, kd, lsd = col(ybatch), col(ivar), col(Knn_diag), col(log_sd)
            if kn.is_cuda:
                import ctypes
                from hipgp_amd import _lib
                p = lambda t: ctypes.c_void_p(t.data_ptr())
                dots = torch.zeros((B, 3), dtype=dt, device=dev)
                _lib.check(_lib.lib().hgp_meanfield_rowdots(_lib.dtype_code(dt), p(knc), B, w, p(qmv), p(qSv), p(dots),
                                                            _lib.stream_ptr(dev)))
            else:       # CPU tensors only in the gloo host-logic tests
                kk = knc * knc
                dots = torch.stack([knc.matmul(qmv), kk.sum(-1), kk.matmul(qSv)], dim=1).contiguous()
            if reduce is not None:
                reduce(dots)
            knm, knkn, knSkn = dots[:, 0], dots[:, 1], dots[:, 2]
            an = -0.5 * iv * ((knm - y) ** 2 + kd - knkn + knSkn) - lsd - 0.5 * LN_2PI
            bdiff = (iv * (knm - y)).contiguous()
            lam = torch.zeros(Mp, dtype=dt, device=dev)
            dm = torch.zeros(Mp, dtype=dt, device=dev)
            if kn.is_cuda:
                ls, ds = lam[j0:j0 + w], dm[j0:j0 + w]
                _lib.check(_lib.lib().hgp_meanfield_cols(_lib.dtype_code(dt), p(knc), B, w, p(iv), p(bdiff), p(ls), p(ds),
                                                         _lib.stream_ptr(dev)))
            else:
                lam[j0:j0 + w] = torch.sum(iv[:, None] * knc * knc, dim=0)
                dm[j0:j0 + w] = -(bdiff[None, :].matmul(knc)).reshape(-1)
            an_sum = an.sum() if lead else an.new_zeros(())
        return {"an_sum": an_sum, "lam_sum": lam, "dm_sum": dm, "n": B if lead else 0}

    def apply_stats(self, stats, bsz):
        """ELBO estimate and theta grads from (all-reduced) batch sums of `bsz` observations."""
        qm, qS = self.standard_variational_params()
        with torch.no_grad():
            qm, qS = qm.detach(), qS.detach()
            bscale = self.N / bsz
            elbo = stats["an_sum"] / bsz - self.get_kl_to_prior(qm, qS) / self.N
            dm = bscale * stats["dm_sum"][:, None] - qm
            lam_diag = bscale * stats["lam_sum"] + 1
            dS = -.5 * lam_diag[:, None] - self.global_theta2.data
            deta1 = dm + dS * (-2 * qm)
        self.global_theta1.grad = -deta1
        self.global_theta2.grad = -dS
        return elbo


# ---- block-diagonal variational family -------------------------------------------------------
def block_chunks(dims, chunk_sizes):
    """Block ordering of a 2-D / 3-D grid (`ziggy/misc/util.py:79-130`, define_block_chunks):
    blocks C-order over the block grid, points C-order inside a block.  Returns
    (block_idx (num_blocks, block_size) int64 on the CPU, to_blocks, from_blocks); the two maps are
    reshape/permute views (no gather table on the device)."""
    dims, chunks = [int(d) for d in dims], [int(c) for c in chunk_sizes]
    assert len(dims) == len(chunks), "xgrids ndim = {}, chunk_sizes ndim = {}".format(len(dims), len(chunks))
    assert len(dims) in (2, 3), "only 2d or 3d inputs"
    for d, (n, c) in enumerate(zip(dims, chunks)):
        assert n % c == 0, "xgrid-{}={} not divis by chunk_size={}".format(d, n, c)
    nd = len(dims)
    split = []
    for n, c in zip(dims, chunks):
        split += [n // c, c]
    perm = [2 * a for a in range(nd)] + [2 * a + 1 for a in range(nd)]
    inv = [perm.index(a) for a in range(2 * nd)]
    nblk, bs = int(np.prod([n // c for n, c in zip(dims, chunks)])), int(np.prod(chunks))

    def to_blocks(m):
        lead = m.shape[:-1]
        t = m.reshape(*lead, *split).permute(*range(len(lead)), *[len(lead) + p for p in perm])
        return t.reshape(*lead, nblk, bs)

    def from_blocks(block_m):
        b = block_m.shape[0]
        t = block_m.reshape(b, *[split[p] for p in perm]).permute(0, *[1 + p for p in inv])
        return t.reshape(b, -1)

    block_idx = to_blocks(torch.arange(int(np.prod(dims))))
    return block_idx, to_blocks, from_blocks


def block_kl_to_standard(blk_m, blk_S):
    """KL(N(m, blockdiag S) || N(0, I)) with a 1e-4 nugget in the log det (`ziggy/misc/stats.py:15-29`)."""
    eye = torch.eye(blk_S.shape[1], dtype=blk_S.dtype, device=blk_S.device)
    L = torch.linalg.cholesky(blk_S + 1e-4 * eye)
    lndet = 2.0 * torch.sum(torch.log(torch.diagonal(L, dim1=-2, dim2=-1)))
    n_blk, blk_size, _ = blk_S.shape
    Strace = torch.sum(torch.diagonal(blk_S, dim1=-2, dim2=-1))
    return .5 * (Strace + torch.sum(blk_m * blk_m) - lndet - n_blk * blk_size)


class BlockToeplitzGP(ToeplitzInducingGP):
    """Block-diagonal variational covariance over neighbouring points of the (expanded) grid
    (`hipgp.py:527-691`).  qm lives in grid order, qS / theta2 in block order
    (num_blocks, block_size, block_size).  On the device the per-block statistics are one fused
    kernel (hgp_block_stats): sum_n ivar_n kn_blk kn_blk^T and kn^T S kn in a single read of kn.
    With streamed=True (`elbo_and_grad`, `predict`) the same sums come from kn held one piece of
    right-hand sides at a time (hgp_rt_block_stats), the (bsz, M') kn never allocated."""

    def __init__(self, kernel, xgrids, num_obs, xblock_size=10, block_sizes=None, sig2_init=1., ell_init=.05,
                 noise2_init=1., init_Svar=.1, learn_kernel=False, learn_noise=False, dtype=torch.float,
                 whitened_type='ziggy', parameterization='expectation-family', jitter_val=1e-3):
        super().__init__(kernel, xgrids, num_obs, sig2_init=sig2_init, ell_init=ell_init,
                         noise2_init=noise2_init, learn_kernel=learn_kernel, learn_noise=learn_noise,
                         dtype=dtype, whitened_type=whitened_type, parameterization=parameterization,
                         jitter_val=jitter_val)
        input_dim = len(xgrids)
        if block_sizes is not None:
            assert input_dim == len(block_sizes), "xgrids ndim = {}, block ndim = {}".format(input_dim, len(block_sizes))
        else:
            block_sizes = [xblock_size for _ in range(input_dim)]
        if self.whitened_type == 'cholesky':
            self.block_dims = [len(x) for x in xgrids]
        else:      # blocks of the expanded grid arange(2m - 2)  (hipgp.py:599-601, 629-634)
            self.block_dims = [2 * len(x) - 2 for x in xgrids]
        self.block_sides = [int(b) for b in block_sizes]
        self.block_idx, self.to_blocks, self.from_blocks = block_chunks(self.block_dims, self.block_sides)
        self.num_blocks, self.block_size = self.block_idx.shape
        eye = torch.eye(self.block_size, dtype=dtype)
        col = lambda: torch.zeros(self.Mprime, 1, dtype=dtype)
        if parameterization == 'standard':
            self.global_m = nn.Parameter(nn.init.xavier_normal_(col()), requires_grad=True)
            self.global_S = nn.Parameter((init_Svar * eye)[None].repeat(self.num_blocks, 1, 1), requires_grad=True)
        else:
            self.global_theta1 = nn.Parameter(nn.init.xavier_normal_(col()), requires_grad=True)
            self.global_theta2 = nn.Parameter(((-.5 / init_Svar) * eye)[None].repeat(self.num_blocks, 1, 1),
                                              requires_grad=True)

    @property
    def name(self):
        return 'block'

    def get_expanded_xgrids(self, xgrids):
        return [torch.arange(2 * len(x) - 2) for x in xgrids]

    def standard_variational_params(self):
        if self.parameterization == 'standard':
            return self.global_m, self.global_S
        S = torch.inverse(-2 * self.global_theta2)                      # block inverse
        m = self.block_diag_multiply(S, self.global_theta1.t()).t()
        return m, S

    def block_diag_multiply(self, S_block, v):
        """rows of v (bsz, M') times the block-diagonal S (num_blocks, bs, bs)  (`hipgp.py:645-656`)."""
        Sv_block = S_block.matmul(self.to_blocks(v)[..., None])
        return self.from_blocks(Sv_block)

    def get_S_from_lam(self, lam):
        return torch.inverse(lam)

    def _block_kernel(self, kn, ivar=None, S=None, gram=True, knSkn=True, trace=False):
        import ctypes
        from hipgp_amd import _lib
        B, Mp = kn.shape
        dev, dt = kn.device, kn.dtype
        nd = len(self.block_dims)
        dims = (ctypes.c_int64 * nd)(*self.block_dims)
        blks = (ctypes.c_int64 * nd)(*self.block_sides)
        knc = kn.detach().contiguous()
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        ivv = None if ivar is None else torch.as_tensor(ivar, dtype=dt, device=dev).reshape(-1).expand(B).contiguous()
        Sc = None if S is None else S.detach().to(dt).contiguous()
        G = torch.empty(self.num_blocks, self.block_size, self.block_size, dtype=dt, device=dev) if gram else None
        q = torch.empty(B, dtype=dt, device=dev) if knSkn else None
        tr = torch.empty((), dtype=dt, device=dev) if trace else None
        _lib.check(_lib.lib().hgp_block_stats(_lib.dtype_code(dt), nd, dims, blks, p(knc), B, p(ivv), p(Sc),
                                              p(G), p(q), p(tr), _lib.stream_ptr(dev)))
        return (G, q, tr) if trace else (G, q)

    def compute_knSkn(self, kn, qS):
        """kn_n^T S kn_n per row (`hipgp.py:661-664`)."""
        if kn.is_cuda and not (torch.is_grad_enabled() and (kn.requires_grad or qS.requires_grad)):
            return self._block_kernel(kn, S=qS, gram=False)[1].squeeze()
        Skn = self.block_diag_multiply(qS, kn)
        return torch.sum(kn * Skn, dim=-1).squeeze()

    def get_identity_for_lam(self):
        return torch.eye(self.block_size, device=self.xgrids[0].device, dtype=self.dtype)

    def get_lam(self, ivar_noise, kn, bscale=1, add_identity=True):
        """bscale sum_n ivar_n kn_blk kn_blk^T (+ I), (num_blocks, bs, bs)  (`hipgp.py:669-685`)."""
        if kn.is_cuda:
            G = self._block_kernel(kn, ivar=ivar_noise, knSkn=False)[0]
        else:
            blk_kn = self.to_blocks(kn).transpose(0, 1)
            G = torch.matmul(blk_kn.transpose(1, 2), ivar_noise * blk_kn)
        return bscale * G + (self.get_identity_for_lam() if add_identity else 0)

    def get_kl_to_prior(self, qm=None, qS=None):
        if qm is None or qS is None:
            qm, qS = self.standard_variational_params()
        return block_kl_to_standard(qm, qS)

    def variational_draws(self, n, eps=None, generator=None):
        """v_s = qm + L eps_s with L the per-block Cholesky factor of S (L L^T = S), (n, M') on the
        device in grid order."""
        with torch.no_grad():
            v = self._draw_eps(n, eps, generator)
            qm, qS = self.standard_variational_params()
            L = torch.linalg.cholesky(qS.detach().to(device=v.device, dtype=self.dtype))
            return self.block_diag_multiply(L, v) + qm.detach().reshape(1, -1).to(device=v.device, dtype=self.dtype)

    # ---- the streamed route: the batch sums without the (bsz, M') kn ---------------------------
    # right-hand sides per piece of kn held at a time (hgp_rt_block_stats' piece_rhs); 0: its default
    kn_piece_rhs = 0

    def _streamed_solve(self, Knm, maxiter_cg, Kmm):
        """(Kmm, d = K^-1 Knm^T by compute_kn's PCG, in place of Knm where the tensor allows), or None
        with Knm untouched: cholesky whitening, an empty batch, a Kmm without rt_block_stats."""
        if self.whitened_type != 'ziggy' or Knm.shape[0] == 0:
            return None
        if Kmm is None:
            Kmm = self.toeplitz()
        if not hasattr(Kmm, "rt_block_stats"):
            return None
        if hasattr(Kmm, "inv_matmul_") and Knm.is_contiguous() and not Knm.requires_grad \
                and not Kmm.column.requires_grad:
            return Kmm, Kmm.inv_matmul_(Knm, do_precond=True, maxiter=maxiter_cg, tol=1e-8)
        return Kmm, Kmm.inv_matmul(Knm.detach(), do_precond=True, maxiter=maxiter_cg, tol=1e-8)

    def streamed_predict_stats(self, Knm, maxiter_cg=50, Kmm=None):
        """Rows (kn.qm, |kn|^2, kn^T S kn) from ToeplitzTensor.rt_block_stats (hgp_rt_block_stats, no
        gram) on the PCG solution, with compute_kn's PCG settings; Knm is consumed."""
        with torch.no_grad():
            sol = self._streamed_solve(Knm, maxiter_cg, Kmm)
            if sol is None:
                return None
            Kmm, d0 = sol
            qm, qS = self.standard_variational_params()
            dt = d0.dtype
            return Kmm.rt_block_stats(d0, self.block_sides, qm.detach().reshape(-1).to(dt).contiguous(),
                                      S=qS.detach().to(dt).contiguous(), gram=False,
                                      piece_rhs=self.kn_piece_rhs)[0]

    def streamed_fit_stats(self, Knm, ybatch, Knn_diag, noise_std_batch=None, maxiter_cg=10, Kmm=None):
        """`batch_stats` of kn = R^T K^-1 Knm^T without the (bsz, M') kn, as the mean-field
        `fit_stats`: d = K^-1 Knm^T by compute_kn's PCG in place of Knm (consumed); the three row
        dots and the per-block grams from ToeplitzTensor.rt_block_stats (hgp_rt_block_stats, kn held
        `kn_piece_rhs` right-hand sides at a time); a_n and bdiff_n from the dots; and, R^T being
        linear, dm_sum = R^T (-sum_n bdiff_n d_n): hgp_meanfield_cols on d with Mp = M and one
        single-RHS R^T."""
        with torch.no_grad():
            sol = self._streamed_solve(Knm, maxiter_cg, Kmm)
            if sol is None:
                return None
            Kmm, d0 = sol
            B = d0.shape[0]
            dev, dt = d0.device, d0.dtype
            qm, qS = self.standard_variational_params()
            ivar, log_sd = self.noise_terms(noise_std_batch)
            col = lambda v: torch.as_tensor(v, dtype=dt, device=dev).detach().reshape(-1).expand(B).contiguous()
            y, iv, kd, lsd = col(ybatch), col(ivar), col(Knn_diag), col(log_sd)
            dots, G = Kmm.rt_block_stats(d0, self.block_sides, qm.detach().reshape(-1).to(dt).contiguous(),
                                         S=qS.detach().to(dt).contiguous(), ivar=iv, gram=True,
                                         piece_rhs=self.kn_piece_rhs)
            knm, knkn, knSkn = dots[:, 0], dots[:, 1], dots[:, 2]
            an = -0.5 * iv * ((knm - y) ** 2 + kd - knkn + knSkn) - lsd - 0.5 * LN_2PI
            bdiff = (iv * (knm - y)).contiguous()
            if d0.is_cuda:
                import ctypes
                from hipgp_amd import _lib
                p = lambda t: ctypes.c_void_p(t.data_ptr())
                d0 = d0.contiguous()
                M = d0.shape[1]
                scr = torch.empty(M, dtype=dt, device=dev)      # sum_n iv_n d_nj^2: not used
                v = torch.empty(M, dtype=dt, device=dev)
                _lib.check(_lib.lib().hgp_meanfield_cols(_lib.dtype_code(dt), p(d0), B, M, p(iv), p(bdiff), p(scr),
                                                         p(v), _lib.stream_ptr(dev)))
            else:       # CPU tensors only in the host-logic tests
                v = -(bdiff[None, :].matmul(d0)).reshape(-1)
            dm = Kmm._matmul_by_RT(v[None, :]).reshape(-1)
        return {"an_sum": an.sum(), "lam_sum": G, "dm_sum": dm, "n": B}

    # ---- natural gradient as batch sums + update (sharding-friendly) ------------------------
    def batch_stats(self, kn, ybatch, Knn_diag, noise_std_batch=None):
        """Sums over this minibatch (or this rank's shard of it):
           an_sum  = sum_n a_n                                         `hipgp.py:370-414`
           lam_sum = sum_n ivar_n kn_blk kn_blk^T   (num_blocks, bs, bs)  `hipgp.py:252-256`
           dm_sum  = -sum_n ivar_n (kn_n.m - y_n) kn_n   (M',)          `hipgp.py:234-236`"""
        if kn.shape[0] == 0:    # an empty shard of a minibatch (hipgp_amd.dist)
            G = kn.new_zeros((self.num_blocks, self.block_size, self.block_size))
            return {"an_sum": kn.new_zeros(()), "lam_sum": G, "dm_sum": kn.new_zeros(kn.shape[1]), "n": 0}
        with torch.no_grad():
            qm, qS = self.standard_variational_params()
            qm, qS = qm.detach(), qS.detach()
            ivar, log_sd = self.noise_terms(noise_std_batch)
            B = kn.shape[0]
            if kn.is_cuda:
                import ctypes
                from hipgp_amd import _lib
                dev, dt = kn.device, kn.dtype
                colv = lambda v: torch.as_tensor(v, dtype=dt, device=dev).reshape(-1).expand(B).contiguous()
                # per-block grams and sum_n ivar_n kn_n^T S kn_n = sum_blk <S, G>_F in one read of kn
                G, _, trSG = self._block_kernel(kn, ivar=ivar, S=qS, knSkn=False, trace=True)
                # a_n without the kn S kn term and dm from the streaming row/column passes
                knc = kn.detach().contiguous()
                zero = torch.zeros(kn.shape[1], dtype=dt, device=dev)
                qmv = qm.reshape(-1).to(dt).contiguous()
                y, iv, kd, lsd = colv(ybatch), colv(ivar), colv(Knn_diag), colv(log_sd)
                an = torch.empty(B, dtype=dt, device=dev)
                lam_diag = torch.empty(kn.shape[1], dtype=dt, device=dev)
                dm = torch.empty(kn.shape[1], dtype=dt, device=dev)
                p = lambda t: ctypes.c_void_p(t.data_ptr())
                _lib.check(_lib.lib().hgp_meanfield_stats(_lib.dtype_code(dt), p(knc), B, kn.shape[1], p(qmv),
                                                          p(zero), p(y), p(iv), p(kd), p(lsd), p(an), p(lam_diag),
                                                          p(dm), _lib.stream_ptr(dev)))
                return {"an_sum": an.sum() - 0.5 * trSG, "lam_sum": G, "dm_sum": dm, "n": B}
            # CPU tensors only reach here in the gloo host-logic tests
            y = ybatch.reshape(-1)
            knm = kn.matmul(qm).reshape(-1)
            knSkn = torch.sum(kn * self.block_diag_multiply(qS, kn), dim=-1)
            iv = torch.as_tensor(ivar, dtype=kn.dtype).reshape(-1).expand(B)
            lsd = torch.as_tensor(log_sd, dtype=kn.dtype).reshape(-1).expand(B)
            an = -0.5 * iv * ((knm - y) ** 2 + Knn_diag.reshape(-1) - (kn * kn).sum(-1) + knSkn) - lsd - 0.5 * LN_2PI
            blk_kn = self.to_blocks(kn).transpose(0, 1)                     # (nblk, B, bs)
            G = torch.matmul(blk_kn.transpose(1, 2), iv[None, :, None] * blk_kn)
            dm_sum = -((iv * (knm - y))[None, :].matmul(kn)).reshape(-1)
        return {"an_sum": an.sum(), "lam_sum": G, "dm_sum": dm_sum, "n": B}

    def apply_stats(self, stats, bsz):
        """ELBO estimate and theta grads from (all-reduced) batch sums of `bsz` observations
        (`hipgp.py:222-276`, 'block' branch)."""
        qm, qS = self.standard_variational_params()
        with torch.no_grad():
            qm, qS = qm.detach(), qS.detach()
            bscale = self.N / bsz
            elbo = stats["an_sum"] / bsz - self.get_kl_to_prior(qm, qS) / self.N
            dm = bscale * stats["dm_sum"][:, None] - qm
            lam_block = bscale * stats["lam_sum"] + self.get_identity_for_lam().to(qm.device)
            dS = -.5 * lam_block - self.global_theta2.data
            dSdeta1 = self.block_diag_multiply(dS, -2 * qm[None, :, 0])
            deta1 = dm + dSdeta1.squeeze().unsqueeze(-1)
        self.global_theta1.grad = -deta1
        self.global_theta2.grad = -dS
        return elbo
