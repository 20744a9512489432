/*
 * hipgp.h — C ABI of libhipgp.so, the MI355X (gfx950) native structured-kernel PCG path of
 * HIP-GP (`suyashk12/hipgp`, package `ziggy`).
 *
 * The reference has no FFI: its operator boundary is duck-typed Python.
 * Each entry point below replaces the reference interface named next to it; the Python
 * drop-in (`hipgp_amd/ziggy/...`, re-exported as `ziggy`) binds them through ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - All data pointers are DEVICE pointers on the plan's device, C-contiguous, in the plan's
 *    dtype (HGP_F32 = float, HGP_F64 = double).  Caller owns them; nothing is freed across
 *    the ABI.  Vectors are row layout (nrhs, M) unless a `layout` argument says otherwise.
 *  - M = prod(m_i); M' = prod(n_i) with n_i = 2 m_i - 2 (m_i > 1) else 1  (`hipgp.py:72`).
 *  - Calls are asynchronous w.r.t. the host and ordered on the plan's stream, except where a
 *    host output pointer is passed (that call synchronises the stream).
 *  - Every function returns 0 on success or a negative HGP_E* code, and sets a thread-local
 *    message readable with hgp_last_error().  No C++ exception crosses the ABI.
 */
#ifndef HIPGP_H
#define HIPGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgp_plan hgp_plan;

enum { HGP_F32 = 0, HGP_F64 = 1 };
enum { HGP_OP_K = 0, HGP_OP_CINV = 1, HGP_OP_RT = 2, HGP_OP_R = 3, HGP_OP_RSQ = 4 };
enum { HGP_SPEC_D = 0, HGP_SPEC_DSQRT = 1, HGP_SPEC_DI = 2 };
enum { HGP_LAYOUT_ROWS = 0, HGP_LAYOUT_COLS = 1 };
enum { HGP_KERN_SQEXP = 0, HGP_KERN_MATERN12 = 1, HGP_KERN_MATERN32 = 2, HGP_KERN_MATERN52 = 3,
       HGP_KERN_GNEITING = 4 };
enum {
  HGP_OK = 0, HGP_E_ARG = -1, HGP_E_HIP = -2, HGP_E_STATE = -3, HGP_E_UNSUPPORTED = -4,
  HGP_E_OOM = -5
};

/* Plan for one gridded inducing mesh m[0..ndim-1] (ndim 1..3, C order, last axis fastest).
 * Replaces the shape/state part of `ToeplitzTensor.__init__` (toeplitz_tensor.py:9-45) and
 * `ToeplitzMatmul.__init__` (toeplitz_expanded.py:82-127).  `hip_stream` may be NULL (null
 * stream).  max_rhs is a capacity hint; workspaces grow on demand.  Any axis length (fp32 and
 * fp64 plans): axes of up to 8192 points run the pruned per-axis passes; fp64 plans whose R / R^T
 * lines exceed 16384 points (axes of 5463..8192) run those two ops on the full fp64 L_R grid, and
 * a plan with an axis beyond 8192 points runs all four operators on the full fp64 L_K / L_R grid
 * (recursive radix-2 levels down to an 8192-point base pass; unfused PCG, no slab split).  One
 * right-hand side's intermediate must stay below 2^31 values, else HGP_E_UNSUPPORTED. */
int hgp_plan_create(int device, int ndim, const int64_t* m, int dtype, int64_t max_rhs,
                    void* hip_stream, hgp_plan** out);

/* Change the stream later calls are ordered on (synchronises the previous stream first, so a
 * plan can be handed between streams, e.g. from a pool of idle plans). */
int hgp_plan_set_stream(hgp_plan* plan, void* hip_stream);

/* Spectrum setup from the kernel-evaluated Toeplitz first column (device, M values):
 * column[0] += jitter (toeplitz_tensor.py:132; pass 0 when already included), circulant
 * embedding (toeplitz_tensor.py:135-143), D = clamp(Re FFT(C), clamp_min) (:25-31), and the
 * operator spectra for K, C^-1 and R/R^T.  Replaces toeplitz_tensor.py:12-33.
 * If n_clamped != NULL it receives the number of clamped eigenvalues of the full expanded
 * (n-grid) spectrum, each mirror image counted, as (D_raw < clamp_min).sum() over the
 * reference's D (synchronises). */
int hgp_plan_set_column(hgp_plan* plan, const void* column, double jitter, double clamp_min,
                        int64_t* n_clamped);

/* y = op(x) for nrhs right-hand sides, row layout.
 *   HGP_OP_K    : K v            x:(nrhs,M)  -> y:(nrhs,M)    toeplitz_tensor.py:70-83
 *   HGP_OP_CINV : C^-1 block v   x:(nrhs,M)  -> y:(nrhs,M)    toeplitz_tensor.py:114-125
 *   HGP_OP_RT   : R^T v          x:(nrhs,M)  -> y:(nrhs,M')   toeplitz_tensor.py:85-97
 *   HGP_OP_R    : R w            x:(nrhs,M') -> y:(nrhs,M)    toeplitz_tensor.py:99-112
 *   HGP_OP_RSQ  : (R o R) w      x:(nrhs,M') -> y:(nrhs,M)    no reference counterpart
 * (the first four are ToeplitzMatmul.forward "gram"/"circ_inv"/"RTv"/"Rv",
 *  toeplitz_expanded.py:139-189).  x and y must not alias.
 * HGP_OP_RSQ is the elementwise square of R as an operator: with s = IFFT_n(sqrt D) the even,
 * n-periodic generator of R (R[j,k] = s[(j - k) mod n], j on the m-grid, k on the n-grid),
 *   y[q, j] = sum_k s[(j - k) mod n]^2 x[q, k],
 * so (R o R) qS is the marginal variance of u = R v, v ~ N(qm, diag qS) (the inducing-grid
 * posterior of the whitened mean-field family; the reference has no such route and leaves
 * sample() a TODO, ziggy/hipgp.py:111-115).  It runs HGP_OP_R's pass sequence on a second
 * spectrum table of R's layout and size, built from the set column on the first HGP_OP_RSQ call
 * after a hgp_plan_set_column (that call allocates and must not run inside a stream capture,
 * else HGP_E_STATE); plans that never ask hold no such table.  Plans whose R / R^T take the
 * full-grid route return HGP_E_UNSUPPORTED.  hgp_toeplitz_apply only: the pass-split, slab and
 * column-gradient entry points refuse HGP_OP_RSQ. */
int hgp_toeplitz_apply(hgp_plan* plan, int op, const void* x, void* y, int64_t nrhs);

/* out3[n*3 + c] = (kn_n.qm, |kn_n|^2, kn_n^2.qS) for kn_n = R^T d_n, without writing kn
 * (hipgp.py:436-443 as predict consumes toeplitz_tensor.py:85-97).  d: (nrhs, M); qm, qS: (M',);
 * out3: 3*nrhs values; device, plan dtype; ordered on the plan's stream; fixed reduction order.
 * 2-D / 3-D plans fuse the three sums into R^T's last pass (RHS-chunked as HGP_OP_RT); 1-D plans,
 * the full-grid route and rows beyond one CU's LDS run R^T into plan scratch a bounded piece of
 * RHS at a time.  nrhs = 0: nothing.  HGP_E_ARG: null plan / pointer, nrhs < 0; HGP_E_STATE: no
 * column set. */
int hgp_rt_stats(hgp_plan* plan, const void* d, int64_t nrhs, const void* qm, const void* qS, void* out3);

/* The mean-field natural-gradient step's sums (hipgp.py:234-250) without writing kn = R^T d:
 * out3 as hgp_rt_stats, and lam[j] = sum_n ivar[n] kn_nj^2 (hipgp.py:241; M' values, overwritten).
 * ivar: nrhs values; the rest as hgp_rt_stats.  No atomics, fixed order: bit-reproducible for a
 * given plan and nrhs.  2-D / 3-D plans fuse both into R^T's last pass (RHS-chunked as HGP_OP_RT,
 * one row-inverse launch per RHS so that the lam updates of two RHS are ordered; the RHS chunks of
 * the plan's other streams accumulate into M'-vectors of plan scratch, added in stream order at
 * the end); 1-D plans, the full-grid route and rows beyond one CU's LDS run R^T into plan scratch
 * a bounded piece of RHS at a time and reduce each piece by rows and by columns.  Extra memory
 * O(M') (fused) or one piece (otherwise), independent of nrhs; see hgp_plan_mem.
 * nrhs = 0: lam zeroed.  HGP_E_ARG: null plan / pointer, nrhs < 0; HGP_E_STATE: no column set.
 * dm = -sum_n bdiff_n kn_n needs no kn either: R^T is linear, so it is one single-RHS
 * HGP_OP_RT of -sum_n bdiff_n d_n (hgp_meanfield_cols on d with Mp = M). */
int hgp_rt_fit_stats(hgp_plan* plan, const void* d, int64_t nrhs, const void* qm, const void* qS,
                     const void* ivar, void* out3, void* lam);

/* The block-diagonal family's sums (hipgp.py:252-256, 661-664) without the (nrhs, M') kn = R^T d:
 *   gram[blk] = sum_n ivar[n] kn_{n,blk} kn_{n,blk}^T   ([nblk][bs][bs], overwritten; may be NULL,
 *               and ivar then too),
 *   out3[n*3 + c] = (kn_n.qm, |kn_n|^2, kn_n^T S kn_n)  (S: [nblk][bs][bs], block diagonal; NULL: 0).
 * blocks[ndim] tiles the plan's expanded grid n_a = 2 m_a - 2 under hgp_block_stats's rules (each
 * side divides its axis, <= 128 points per block, 2-D / 3-D).  A gram entry pairs kn values of
 * different grid rows, so this is no epilogue of R^T's last pass: R^T runs into plan scratch
 * piece_rhs right-hand sides at a time and one kernel reads each piece once for the gram and the
 * three dots, the gram continuing from piece to piece (one owner thread per entry and launch,
 * launches ordered on the plan's stream: no atomics, bit-reproducible).  piece_rhs = 0:
 * min(nrhs, max(32 Mi values / M', bs)) -- every piece re-reads and re-writes the gram, as much as
 * bs rows of kn.  Extra memory: one piece plus 3 piece_rhs row partials per workgroup, independent
 * of nrhs (hgp_plan_mem reports it, hgp_plan_trim frees it).  Every route of HGP_OP_RT.
 * nrhs = 0: gram zeroed, nothing else written.  HGP_E_ARG: null plan / pointer, nrhs < 0,
 * piece_rhs < 0; HGP_E_STATE: no column set; HGP_E_UNSUPPORTED: 1-D plans, a size-1 axis, refused
 * block shapes. */
int hgp_rt_block_stats(hgp_plan* plan, const void* d, int64_t nrhs, const int64_t* blocks, int64_t piece_rhs,
                       const void* qm, const void* S, const void* ivar, void* out3, void* gram);

/* Batched PCG, exactly the recurrence of conj_grad2 (cg.py:44-80) for layout ROWS
 * (b,x:(nrhs,M)) and conj_grad (cg.py:5-41) for layout COLS (b,x:(M,nrhs)): A = K,
 * preconditioner C^-1 if use_precond, x0 = 0, per-RHS alpha/beta, stop when ALL
 * sqrt(r.r) < tol after the x/r update.  The early-exit test runs on the device (a flag read
 * by every later kernel), so the host is not synchronised per iteration (solves with
 * maxiter > 32 read the flag every 16 iterations to stop queueing no-op iterations).
 * iters_done (host, may be NULL): number of iterations executed (synchronises).
 * x may be b itself (the solve in place of its right-hand side: b is read once, element by
 * element, before x is first written), here and in hgp_pcg_begin.
 * Replaces ToeplitzTensor._solve (toeplitz_tensor.py:54-68) / InvMatmul.forward. */
int hgp_pcg_solve(hgp_plan* plan, const void* b, void* x, int64_t nrhs, int maxiter,
                  double tol, int use_precond, int layout, int* iters_done);

/* Profiling: run only pass `pass` (0-based; -1 = all) of the op's pass sequence (the
 * intermediate workspace is whatever the previous call left).  hgp_op_pass_count returns the
 * number of passes (1 for 1-D, 3 for 2-D, 5 for 3-D).  Used by bench.py to time each kernel
 * with HIP events.  On a product-form plan (below) a single pass is still one of the general
 * sequence's three -- the sequence the fused PCG runs; pass = -1 runs the product form. */
int hgp_toeplitz_apply_pass(hgp_plan* plan, int op, const void* x, void* y, int64_t nrhs, int pass);
int hgp_op_pass_count(const hgp_plan* plan);

/* Product form.  hgp_plan_set_column tests every 2-D column for c[i][j] = t0[i] t1[j] + sigma
 * [i = j = 0] (a product kernel on a product grid plus the jitter); where it holds to the
 * column's storage rounding and the spectrum clamp changed nothing, hgp_toeplitz_apply(HGP_OP_K)
 * runs K X = T0 X T1^T + sigma X as two 1-D passes on real data instead of the padded 2-D
 * transform (the environment variable HGP_SEPARABLE=0, read by every hgp_plan_set_column, turns this off).
 * hgp_plan_is_separable: 1 if the last column took the product form, 0 if not, a negative HGP_E*
 * code on error; the decision is made on the first such call or plain K matvec after a set_column
 * (it synchronises the plan's stream once and must not run inside a stream capture); sigma / resid
 * (optional) receive the recovered jitter and max |c - t0 t1^T| / max |c|, corner excluded (0
 * where the plan is not tested: 1-D, 3-D, HGP_SEPARABLE=0).
 * hgp_separable_detect runs the same test on a HOST column of m0 x m1 values (no device):
 * out4 = {accepted, sigma, resid, k00}, t0 / t1 (optional, m0 / m1 doubles) the factor columns. */
int hgp_plan_is_separable(hgp_plan* plan, double* sigma, double* resid);
int hgp_separable_detect(int dtype, int64_t m0, int64_t m1, const void* column, double jitter, double* out4,
                         double* t0, double* t1);

/* Banded product form.  A product-form fp32 plan whose factor columns t0, t1 vanish in fp32 beyond
 * a few taps runs the two passes as banded matrix products on the matrix cores, with no transform.
 * The tap radius of a factor t of m values is the smallest r with
 *   2 sum_{j > r} |t[j]| <= 2^-25 (|t[0]| + 2 sum_{j >= 1} |t[j]|);
 * dropping the taps beyond it changes K x by at most 2^-24 ||t0||_1 ||t1||_1 max |x|.  The banded
 * passes run where both radii are at most 32 (the library's HGP_BAND_RMAX) and the environment
 * variable HGP_BANDED, read by every hgp_plan_set_column, is not 0.
 * hgp_plan_band_radius: 1 if the last column runs the banded passes, else 0 (a negative HGP_E* code
 * on error); r (optional) receives the two radii, -1 where the plan is not in product form.  It
 * settles the product-form decision as hgp_plan_is_separable does.
 * hgp_band_radius applies the rule to a HOST column t of m doubles (no device). */
int hgp_plan_band_radius(hgp_plan* plan, int r[2]);
int hgp_band_radius(int64_t m, const double* t, int64_t* r);

/* The banded passes run as ONE kernel that keeps the intermediate V = X S1 in LDS, bit
 * for bit the two-pass result, unless HGP_BAND_FUSED=0 was set when hgp_plan_set_column was called.
 * hgp_plan_band_fused: 1 if the last column's K matvec takes the fused kernel, else 0 (a negative
 * HGP_E* code on error).  hgp_band_fused_tile: {rows of a block's segment, columns of its strip} of
 * the built kernel, both multiples of 16 (no device). */
int hgp_plan_band_fused(hgp_plan* plan);
int hgp_band_fused_tile(int tile[2]);

/* Stepwise PCG for the callback form of conj_grad/conj_grad2 (cg.py:77-78): begin() sets
 * x0 = 0, r = b, z = P r, p = z; step() runs one iteration and, if `converged` != NULL,
 * reports (synchronising) whether the break test fired on it.  x is updated in place in the
 * caller's buffer given to begin(). */
int hgp_pcg_begin(hgp_plan* plan, const void* b, void* x, int64_t nrhs, int use_precond,
                  int layout);
int hgp_pcg_step(hgp_plan* plan, double tol, int* converged);

/* Per-RHS r.r after the last hgp_pcg_step (device, nrhs values in the plan dtype).  With
 * tol < 0 a step never sets the convergence flag, so a caller that shards the right-hand
 * sides over processes can apply the reference's ALL-RHS break rule (cg.py:69-71) globally:
 * step(tol = -1), read r.r, all-reduce "every sqrt(r.r) < tol", stop.  x is final after the
 * step that met the test (the break precedes only the z/p update). */
int hgp_pcg_rnorm2(hgp_plan* plan, void* out);

/* Device-side form of the same all-rank break rule (no host round trip per iteration):
 * hgp_pcg_local_flag writes *flag (device int) = 1 when every sqrt(r.r) of the plan's RHS is
 * below tol after the last step(tol = -1); the caller all-reduces it (MIN, e.g. RCCL on the
 * same stream order) and hgp_pcg_set_done(flag) raises the plan's done flag when the reduced
 * value is 1, so every later step of the solve is a no-op on the device. */
int hgp_pcg_local_flag(hgp_plan* plan, double tol, int* flag);
int hgp_pcg_set_done(hgp_plan* plan, const int* flag);
/* Iterations the current solve has executed whose break test did not stop it, plus the one
 * that did (host int; synchronises the plan's stream). */
int hgp_pcg_iters(hgp_plan* plan, int* iters);

/* Grid-block (slab) sharding along axis 0 (row e2: a 2-D / 3-D grid's axis-0 rows split over
 * ranks; hipgp_amd/slab.py drives it).  Each op is its pass sequence split at the axis-0
 * convolution, which needs whole axis-0 lines and so runs between two all-to-all transposes.
 * Exchange layout E (plan dtype, interleaved complex): E[g][q][i][c]
 *   d = 2: g < NG = L1/2 + 1 compact axis-1 columns, inner = 1;
 *   d = 3: g < NG = L1 axis-1 frequencies, c < inner = the compact half-spectrum pitch of axis 2;
 *   q < nrhs; i = axis-0 row (a rank's rows in FWD / INV, whole lines in CONV).
 * stage HGP_SLAB_FWD : x (nrhs, nrows, rest of the input row) real -> E over this rank's nrows
 *                      input rows (all NG groups)                 toeplitz_tensor.py:79,94,109,122
 * stage HGP_SLAB_CONV: E lines [ng][nrhs][P0][inner], P0 = max(in0, out0) rows per line, groups
 *                      [g0, g0 + ng) of the op's spectrum; in place allowed  (:80-82 etc.)
 * stage HGP_SLAB_INV : E over this rank's nrows output rows -> y (nrhs, nrows, rest) real, crop
 * stage HGP_SLAB_CONV_A2A: the axis-0 convolution of groups [g0, g0 + ng) straight from the
 *                      receive buffer of the first all-to-all to the send buffer of the second
 *                      (no line buffer, no gather / scatter copies): `nrows` = the world size W,
 *                      in  = [r][g][q][i - a_r][c] for the balanced split of the in0 input rows
 *                            over the W ranks (rank r: rows [a_r, a_r + cnt_r)),
 *                      out = [r][g][q][o - b_r][c] for the split of the out0 output rows,
 *                      g < ng, q < nrhs, c < inner; in != out.
 * Partial dot products / PCG scalars are the caller's (all-reduced over ranks). */
enum { HGP_SLAB_FWD = 0, HGP_SLAB_CONV = 1, HGP_SLAB_INV = 2, HGP_SLAB_CONV_A2A = 3 };
int hgp_slab_info(const hgp_plan* plan, int op, int64_t* ngroups, int64_t* inner);
int hgp_slab_pass(hgp_plan* plan, int op, int stage, const void* in, void* out, int64_t nrhs,
                  int64_t nrows, int64_t g0, int64_t ng);
/* hgp_slab_pass with two options for the slab PCG (hipgp_amd/slab.py SlabToeplitz.pcg):
 *   done (device int or NULL): every kernel of the stage is a no-op once *done != 0, so the
 *        iterations after the all-rank break cost (almost) nothing without a host round trip;
 *   dotv, dot_out (HGP_SLAB_INV only, device, or NULL): the stage also leaves this rank's
 *        per-RHS dot dot_out[q] = sum_j y[q, j] dotv[q, j] of its output y (dotv laid out
 *        like y), from per-row-pair partials summed in a fixed order -- p.Ap / z.r of
 *        cg.py:66,74 without a second read of the vectors.  dot_out: nrhs values. */
int hgp_slab_pass_ex(hgp_plan* plan, int op, int stage, const void* in, void* out, int64_t nrhs,
                     int64_t nrows, int64_t g0, int64_t ng, const void* dotv, void* dot_out,
                     const int* done);

/* The slab PCG's vector / scalar updates (cg.py:63-78) on this rank's slab (nrhs rows of M
 * values, plan dtype; M may be 0 on a rank without rows), with every per-RHS dot ALREADY
 * all-reduced by the caller between the calls.  done / iters: device ints (0 at the start);
 * every call is a no-op once *done != 0 (done = the iteration the break fired in).
 *   hgp_slab_cg_xr   : alpha = rs / pAp; x += alpha p; r -= alpha Ap; rr = local sum r.r
 *   hgp_slab_cg_check: iters += 1; done = iters when every sqrt(rr) < tol (rr reduced; NaN =
 *                      not converged, cg.py:70)
 *   hgp_slab_cg_p    : beta = zr / rs; rs = zr; p = z + beta p
 * All per-RHS scalars are device arrays of nrhs values; ordered on the plan's stream. */
int hgp_slab_cg_xr(hgp_plan* plan, void* x, void* r, const void* p, const void* Ap, const void* rs,
                   const void* pAp, void* rr, int64_t nrhs, int64_t M, const int* done);
int hgp_slab_cg_check(hgp_plan* plan, const void* rr, int64_t nrhs, double tol, int* done, int* iters);
int hgp_slab_cg_p(hgp_plan* plan, void* p, const void* z, void* rs, const void* zr, int64_t nrhs,
                  int64_t M, const int* done);

/* The clamped spectrum D (which=HGP_SPEC_D), sqrt(D) or 1/D on the full expanded grid
 * (device, M' reals) — the real parts of ToeplitzTensor.D / D_sqrt / Di
 * (toeplitz_tensor.py:28-31). */
int hgp_get_spectrum(hgp_plan* plan, int which, void* out);

/* Per-row dot products out[b] = sum_j a[b,j] c[b,j] (device), used by the generic
 * conj_grad2 path with caller-supplied A_mul callables (cg.py:64,66,69,74). */
int hgp_rowdot(int dtype, const void* a, const void* c, void* out, int64_t nrhs, int64_t M,
               void* hip_stream);

/* Point-observation cross covariance on a gridded mesh, the PCG right-hand sides:
 *   out[n, j] = k(x_n, u_j),  x: (nobs, ndim) device, u_j the C-order mesh of grids[0..ndim-1]
 *   (device arrays of m[a] points), out: (nobs, M) device, dtype HGP_F32 / HGP_F64.
 * kind: HGP_KERN_SQEXP  sig2 exp(-|(x-u)/ell|^2 / 2)            (kernels.py:73-79)
 *       HGP_KERN_MATERN{12,32,52}  Matern nu = 1/2, 3/2, 5/2    (kernels.py:145-158)
 * Same per-element arithmetic as the reference, without its (nobs, M, ndim) broadcast
 * (replaces svi_gp.py:72 `self.kernel(xbatch, self.xinduce, kern_params)`). */
int hgp_kuf_grid(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                 const void* x, int64_t nobs, double sig2, double ell, void* out,
                 void* hip_stream);

/* Line-integral ("semi-integrated") cross covariance on a gridded mesh, SURVEY §8(f) row 2
 * (the inter-domain observations of config 5: observation n is the segment 0 -> x_n):
 *   out[n, j] = |x_n| * mean_{a < npts} k(u_j, alpha_a x_n),  alpha_a = a/npts + u[0]/npts
 * = Kernel.k_semi_mc (kernels.py:19-39) as svi_gp._make_grams uses it (svi_gp.py:61-64,
 * transposed).  u: device scalar holding the reference's single torch.rand(1) draw, so the
 * caller consumes the RNG exactly as the reference does.  kind: any HGP_KERN_*; kparam is
 * Gneiting's alpha (ignored otherwise).  1 <= npts <= 1024.  Layout as hgp_kuf_grid. */
int hgp_kuf_semi_mc(int dtype, int kind, double kparam, int ndim, const int64_t* m,
                    const void* const* grids, const void* x, int64_t nobs, double sig2,
                    double ell, int npts, const void* u, void* out, void* hip_stream);

/* Analytic SqExp line integral, SqExp.k_semi -> semi_integrated_sqe (kernels.py:80-85,
 * 223-237), replacing svi_gp.py:58-59:  out[n, j] = |x_n| int_0^1 k(u_j, a x_n) da
 * (NaN for |x_n| = 0, as the reference).  Layout as hgp_kuf_grid. */
int hgp_kuf_semi_sqexp(int dtype, int ndim, const int64_t* m, const void* const* grids,
                       const void* x, int64_t nobs, double sig2, double ell, void* out,
                       void* hip_stream);

/* Backward of hgp_kuf_grid with respect to the two kernel hyper-parameters: with g (nobs, M)
 * the upstream gradient, laid out as the forward's out,
 *   grad2[0] = sum_{n,j} g[n,j] dK[n,j]/dsig2,   grad2[1] = sum_{n,j} g[n,j] dK[n,j]/dell
 * (device, 2 values of dtype, ordered on hip_stream).  K is recomputed from x and the grids with
 * the forward's arithmetic, so nothing of the forward is kept: this replaces torch's autograd of
 * kernels.py:73-79, 145-158, which saves the (nobs, M, ndim) difference, its square, the
 * distance and the exponential.  kind: HGP_KERN_SQEXP / HGP_KERN_MATERN{12,32,52};
 * HGP_KERN_GNEITING returns HGP_E_UNSUPPORTED (the reference's own gradient is NaN at a
 * coincident point).  Sums in fp64 in a fixed order, no atomics: the same bits on every call.
 * nobs = 0: two zeros.  HGP_E_ARG (before any HIP call): null pointer, bad dtype / kind / ndim,
 * nobs < 0.  Scratch: at most 2048 fp64 pairs, stream-ordered (hipMallocAsync). */
int hgp_kuf_grid_grad(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                      const void* x, int64_t nobs, double sig2, double ell,
                      const void* g, void* grad2, void* hip_stream);

/* The same two sums for hgp_kuf_semi_mc (the autograd of Kernel.k_semi_mc, kernels.py:19-39,
 * through its (M, nobs * npts, ndim) broadcast): |x_n| mean_a of the point derivatives at the
 * sample points alpha_a x_n.  u: the offset draw the forward used.  kparam is ignored (Gneiting
 * is refused as above).  1 <= npts <= 1024 else HGP_E_ARG. */
int hgp_kuf_semi_mc_grad(int dtype, int kind, double kparam, int ndim, const int64_t* m,
                         const void* const* grids, const void* x, int64_t nobs,
                         double sig2, double ell, int npts, const void* u,
                         const void* g, void* grad2, void* hip_stream);

/* The same two sums for hgp_kuf_semi_sqexp (the autograd of SqExp.k_semi ->
 * semi_integrated_sqe, kernels.py:80-85, 223-237), SqExp only like its forward: the
 * closed-form derivative of the forward's own expression (NaN for |x_n| = 0, as the forward). */
int hgp_kuf_semi_sqexp_grad(int dtype, int ndim, const int64_t* m, const void* const* grids,
                            const void* x, int64_t nobs, double sig2, double ell,
                            const void* g, void* grad2, void* hip_stream);

/* Product with the point-observation cross covariance, never stored:
 *   out[n, s] = sum_j Kuf[n, j] w[s, j],   Kuf[n, j] = k(x_n, u_j) exactly as hgp_kuf_grid writes it,
 *   w: (nw, M) rows, out: (nobs, nw) rows, both device arrays of dtype; x, grids, kind as hgp_kuf_grid
 *   (HGP_KERN_GNEITING refused as there).
 * With w = K^-1 R qm the posterior mean E[f(x_n)] = kn(x_n).qm at any number of points from one
 * single-RHS solve: replaces, for the mean, the per-point route of hipgp.py:416-446 (Knm row by
 * svi_gp.py:72, its solve and R^T by hipgp.py:117-146, the dot with qm at hipgp.py:436).  With
 * several rows w_s = K^-1 R v_s, joint draws kn(x).v_s at arbitrary points (the reference leaves
 * sample() a TODO, hipgp.py:111-115).
 * A block owns 64 points and sweeps a slice of the grid; products are summed in dtype over runs of
 * at most 256 points of the last axis, the runs in fp64.  nsplit: slices the grid is cut into
 * (whole units of 64 mesh points), their fp64 partial sums added in slice order by a second kernel.
 * 0: chosen from (nobs, M) and the device's CU count alone (about 16 blocks per CU, a slice at
 * least 256 mesh points); > 0: that many, at most ceil(M / 64).  No atomics: the same bits on
 * every call with the same arguments on the same device.
 * Scratch, nsplit > 1 only: nsplit * nobs * min(nw, 8) fp64, stream-ordered (hipMallocAsync /
 * hipFreeAsync on hip_stream); with nsplit = 0 at most (16 CUs + nobs / 64) * 4 KiB, under
 * 32 MiB at 256 CUs (from 16 CUs tiles of 64 points on, the grid is one slice: no scratch).
 * nobs = 0 or nw = 0: nothing written, 0 returned.  HGP_E_ARG (before any HIP call): null pointer,
 * bad dtype / kind / ndim, a grid size < 1, nobs / nw / nsplit < 0.  HGP_E_HIP: the launch or the
 * scratch allocation failed (more than 2^31 - 1 blocks: nobs / 64 * nsplit). */
int hgp_kuf_grid_matvec(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                        const void* x, int64_t nobs, double sig2, double ell,
                        const void* w, int64_t nw, int64_t nsplit, void* out, void* hip_stream);

/* The same product with the Monte-Carlo line-integral cross covariance of hgp_kuf_semi_mc
 * (Kernel.k_semi_mc, kernels.py:19-39, as svi_gp.py:61-64 uses it): element values, kind (any
 * HGP_KERN_*), kparam, npts (1..1024, else HGP_E_ARG) and the offset draw u as there.  A block owns
 * one observation and a range of outer mesh indices (all axes but the last); per-thread fp64 sums,
 * a fixed-order block reduction.  nsplit counts ranges of outer indices: 0 picks about 4 blocks per
 * CU, > 0 is clamped to the number of outer indices (1 for a 1-D grid).  Scratch and errors as
 * hgp_kuf_grid_matvec (nsplit * nobs * min(nw, 8) fp64 when nsplit > 1). */
int hgp_kuf_semi_mc_matvec(int dtype, int kind, double kparam, int ndim, const int64_t* m,
                           const void* const* grids, const void* x, int64_t nobs, double sig2,
                           double ell, int npts, const void* u, const void* w, int64_t nw,
                           int64_t nsplit, void* out, void* hip_stream);

/* The same product with the analytic SqExp line integral of hgp_kuf_semi_sqexp (SqExp.k_semi ->
 * semi_integrated_sqe, kernels.py:80-85, 223-237): SqExp only like its forward, NaN rows for
 * |x_n| = 0 as there.  Structure, nsplit, scratch and errors as hgp_kuf_semi_mc_matvec. */
int hgp_kuf_semi_sqexp_matvec(int dtype, int ndim, const int64_t* m, const void* const* grids,
                              const void* x, int64_t nobs, double sig2, double ell,
                              const void* w, int64_t nw, int64_t nsplit, void* out, void* hip_stream);

/* Product with the TRANSPOSED point-observation cross covariance, never stored:
 *   out[s, j] = sum_n Kuf[n, j] c[s, n],   Kuf[n, j] = k(x_n, u_j) exactly as hgp_kuf_grid writes it,
 *   c: (nc, nobs) rows, out: (nc, M) rows in the PCG layout (mesh order, last axis fastest), both
 *   device arrays of dtype; x, grids, kind as hgp_kuf_grid (HGP_KERN_GNEITING refused as there).
 * The arguments mirror hgp_kuf_grid_matvec with (w, nw) replaced by (c, nc).  Together the two give
 * the operator p -> K p + Kuf^T diag(iv) Kuf p of the system whose solution is the optimal
 * variational mean of all observations (the closed form hipgp.py:278-368 reaches through kn and a
 * dense M' x M' solve).
 * A block is one wave and owns 64 mesh points, one per lane; it sweeps the observations in order, so
 * everything indexed by the observation is wave-uniform.  Products are summed in dtype over runs of
 * at most 256 consecutive observations, the runs in fp64 in observation order.  nsplit: slices the
 * observations are cut into (whole runs of 256), their fp64 partial sums part[slice][s][j] added in
 * slice order by a second kernel.  0: chosen from (nobs, M) and the device's CU count alone:
 * 1 when ceil(M / 64) >= 16 CUs, else ceil(16 CUs / ceil(M / 64)); > 0: that many; either way at
 * most ceil(nobs / 256).  No atomics: the same bits on every call with the same arguments on the
 * same device.
 * Scratch, nsplit > 1 only: nsplit * min(nc, 8) * M fp64, stream-ordered (hipMallocAsync /
 * hipFreeAsync on hip_stream); with nsplit = 0 under 32 MiB at 256 CUs.
 * nobs = 0: out is set to zero (an empty sum); nc = 0: nothing written; both return 0.  HGP_E_ARG
 * (before any HIP call): null pointer, bad dtype / kind / ndim, a grid size < 1, nobs / nc /
 * nsplit < 0.  HGP_E_HIP: the launch or the scratch allocation failed (more than 2^31 - 1 blocks). */
int hgp_kuf_grid_rmatvec(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                         const void* x, int64_t nobs, double sig2, double ell,
                         const void* c, int64_t nc, int64_t nsplit, void* out, void* hip_stream);

/* The same product with the Monte-Carlo line-integral cross covariance of hgp_kuf_semi_mc: element
 * values, kind (any HGP_KERN_*), kparam, npts (1..1024, else HGP_E_ARG) and the offset draw u as
 * there.  A block (one wave) owns one outer mesh index and 64 points of the last axis and walks its
 * slice of the observations in order; every term is added in fp64.  nsplit, scratch and errors as
 * hgp_kuf_grid_rmatvec, with outer * ceil(m_last / 64) in place of ceil(M / 64). */
int hgp_kuf_semi_mc_rmatvec(int dtype, int kind, double kparam, int ndim, const int64_t* m,
                            const void* const* grids, const void* x, int64_t nobs, double sig2,
                            double ell, int npts, const void* u, const void* c, int64_t nc,
                            int64_t nsplit, void* out, void* hip_stream);

/* The same product with the analytic SqExp line integral of hgp_kuf_semi_sqexp: SqExp only like its
 * forward; an observation with |x_n| = 0 is a NaN row there and makes every out[s, j] NaN, as the
 * dense product would.  Structure, nsplit, scratch and errors as hgp_kuf_semi_mc_rmatvec. */
int hgp_kuf_semi_sqexp_rmatvec(int dtype, int ndim, const int64_t* m, const void* const* grids,
                               const void* x, int64_t nobs, double sig2, double ell,
                               const void* c, int64_t nc, int64_t nsplit, void* out, void* hip_stream);

/* hgp_kuf_grid_matvec over a WINDOW of pairs, for kernels far shorter than the grid:
 *   out[n, s] = sum_{j in window(n)} k(x_n, u_j) w[s, j];  dtype, kind, ndim, grids, x, w, out as there.
 * Pair (n, j) is in the window iff fabs(x[n][a] - g_a[j_a]) <= rho on every axis a, evaluated in
 * dtype with rho rounded once to dtype: a box of index ranges [lo_a, hi_a), found by binary search
 * on the axis coordinates, which must be strictly increasing.  With rho the distance from which
 * k(r) <= tol sig2 on, every dropped pair is farther than rho, so per output
 *   |dense - windowed| <= tol sig2 sum_j |w[s, j]|.
 * A point farther than rho from the grid's hull on some axis has an empty window: exact zeros.
 * Work is nobs times the window's size.  One wave per point, lanes across the last-axis range, a
 * loop over the outer rows of the box; a lane adds its products of a row in dtype, the rows in
 * fp64, the lanes by a fixed xor butterfly; weight rows in groups of at most 8.  No atomics, no
 * scratch: the same bits on every call with the same arguments.
 * nobs = 0 or nw = 0: nothing written, 0 returned.  HGP_E_ARG (before any HIP call): null pointer,
 * bad dtype / kind / ndim, a grid size < 1, nobs / nw < 0, rho negative or not finite.  HGP_E_HIP:
 * the launch failed. */
int hgp_kuf_grid_matvec_win(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                            const void* x, int64_t nobs, double sig2, double ell, double rho,
                            const void* w, int64_t nw, void* out, void* hip_stream);

/* hgp_kuf_grid_rmatvec over the same window:
 *   out[s, j] = sum_{n: (n, j) in window} c[s, n] k(x_n, u_j);  c, out as hgp_kuf_grid_rmatvec.
 * The same set of pairs and the same element values, bit for bit, as hgp_kuf_grid_matvec_win: the
 * two are exact transposes, which a conjugate-gradient solve on K + Kuf^T diag(iv) Kuf needs.
 * A gather: a block owns a tile of mesh points and visits only the bins of observations that can
 * reach it.  order (nobs, device int64) lists the observations sorted stably by bin; bin_start
 * (total bins + 1, device int64) are the offsets of the bins in that list.  The bin of x on axis a
 * is (number of nodes g_a[i] <= x_a) / tile[a], the bins are numbered in C order over the axes with
 * nbins[a] per axis; tile and nbins come from hgp_kuf_win_bins.  Products are added in dtype over
 * chunks of at most 256 staged observations, the chunks in fp64, in the order of the list: no
 * atomics, the same bits on every call with the same arguments.  The kernel skips any order[k]
 * outside [0, nobs) and any range of bin_start outside 0 <= s0 <= s1 <= nobs, so a wrong list gives
 * wrong sums and never an access out of bounds (bin_start must still hold total bins + 1 entries).
 * nobs = 0: out is set to zero (order and bin_start are not read); nc = 0: nothing written; both
 * return 0.  Errors as hgp_kuf_grid_matvec_win, and null order / bin_start with nobs > 0. */
int hgp_kuf_grid_rmatvec_win(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                             const void* x, int64_t nobs, double sig2, double ell, double rho,
                             const void* c, int64_t nc, const int64_t* order, const int64_t* bin_start,
                             void* out, void* hip_stream);

/* The tile and bin geometry hgp_kuf_grid_rmatvec_win assumes (host only, no HIP call): tile_out[a]
 * mesh points of a tile, and cells of a bin, along axis a; nbins_out[a] = m[a] / tile_out[a] + 1
 * bins, which cover the cells 0 .. m[a].  Both arrays have 3 entries; axes >= ndim get 1 and 1.
 * HGP_E_ARG: ndim outside 1..3, a null pointer, a grid size < 1. */
int hgp_kuf_win_bins(int ndim, const int64_t* m, int64_t* tile_out, int64_t* nbins_out);

/* ---- SqExp with one length scale per axis ("ARD"), point observations -------------------------
 * The reference's SqExp takes ell as "a scalar, or a tensor that matches the dimension of data"
 * (kernels.py:73-79):  k(x, u) = sig2 exp(-sum_a ((x_a - u_a) / ell[a])^2 / 2).  The six entries
 * below are the point-observation entries above with `const double* ell` (ndim host values, read
 * during the call) in place of `double ell`, and for the windowed pair `const double* rho` (ndim
 * host values) in place of `double rho`.  Everything else (layouts, summation orders, scratch,
 * nsplit, determinism, the remaining errors) is the scalar entry's; the scalar entries run the same
 * launch code with their one value on every axis, so equal ell[a] (and rho[a]) give the scalar
 * entry's bits.  Rules of all six, checked before any HIP call: kind must be HGP_KERN_SQEXP (the
 * reference's Matern formula, kernels.py:145-158, defines no vector ell), every ell[a] finite and
 * > 0, every rho[a] finite and >= 0, ell / rho non-null; else HGP_E_ARG. */

/* hgp_kuf_grid with ell[a] per axis (kernels.py:73-79 with a vector ell). */
int hgp_kuf_grid_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                     const void* x, int64_t nobs, double sig2, const double* ell, void* out,
                     void* hip_stream);

/* hgp_kuf_grid_matvec with ell[a] per axis (kernels.py:73-79). */
int hgp_kuf_grid_matvec_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                            const void* x, int64_t nobs, double sig2, const double* ell,
                            const void* w, int64_t nw, int64_t nsplit, void* out, void* hip_stream);

/* hgp_kuf_grid_rmatvec with ell[a] per axis (kernels.py:73-79). */
int hgp_kuf_grid_rmatvec_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                             const void* x, int64_t nobs, double sig2, const double* ell,
                             const void* c, int64_t nc, int64_t nsplit, void* out, void* hip_stream);

/* hgp_kuf_grid_matvec_win with ell[a] and a radius rho[a] per axis (kernels.py:73-79).  Pair (n, j)
 * is in the window iff fabs(x[n][a] - g_a[j_a]) <= rho[a] on every axis a, in dtype, each rho[a]
 * rounded once to dtype.  With rho[a] the distance from which axis a's factor
 * exp(-(r / ell[a])^2 / 2) is <= tol, a dropped pair has an axis whose factor is <= tol while the
 * others are <= 1, so the scalar entry's bound holds: |dense - windowed| <= tol sig2 sum_j |w[s, j]|. */
int hgp_kuf_grid_matvec_win_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                                const void* x, int64_t nobs, double sig2, const double* ell,
                                const double* rho, const void* w, int64_t nw, void* out,
                                void* hip_stream);

/* hgp_kuf_grid_rmatvec_win over that window (kernels.py:73-79): the same predicate and the same
 * element values as hgp_kuf_grid_matvec_win_ard, so the two are exact transposes.  order / bin_start
 * as the scalar entry reads them (hgp_kuf_win_bins: the bins do not depend on the radius). */
int hgp_kuf_grid_rmatvec_win_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                                 const void* x, int64_t nobs, double sig2, const double* ell,
                                 const double* rho, const void* c, int64_t nc, const int64_t* order,
                                 const int64_t* bin_start, void* out, void* hip_stream);

/* Backward of hgp_kuf_grid_ard (the autograd of kernels.py:73-79 with a vector ell): with g (nobs, M)
 * the upstream gradient, 1 + ndim sums of dtype on the device,
 *   grad[0] = sum g dK/dsig2,   grad[1 + a] = sum g dK/dell[a],  dK/dell[a] = K ((x_a - u_a) / ell[a])^2 / ell[a].
 * The tiles, the fp64 sums in a fixed order without atomics and the bit-reproducible result of
 * hgp_kuf_grid_grad; grad[0] has that entry's bits when all ell[a] are equal, and the per-axis sums
 * then add up to its dK/dell sum to rounding.  nobs = 0: 1 + ndim zeros.  Scratch: at most 2048
 * times 4 fp64, stream-ordered. */
int hgp_kuf_grid_grad_ard(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                          const void* x, int64_t nobs, double sig2, const double* ell,
                          const void* g, void* grad, void* hip_stream);

/* hgp_kuf_semi_mc_matvec over the WINDOW of a line, for kernels far shorter than the grid (the
 * Monte-Carlo line integral of Kernel.k_semi_mc, kernels.py:19-39, summed over a tube around the
 * segment in place of the whole mesh):
 *   out[n, s] = sum_{j in window(n)} Kuf[n, j] w[s, j];  dtype, ndim, grids, x, npts, u, w, out as there;
 *   kind HGP_KERN_SQEXP .. HGP_KERN_MATERN52 (HGP_KERN_GNEITING refused).
 * Line n is the segment from the origin to x_n, cut into P = pieces[n] equal pieces (a device int
 * array of npieces = nobs entries; a value outside 1 .. 64 is clamped).  Pair (n, j) is in the window
 * iff node j lies in the bounding box of some piece widened by rho on every axis (lo - u <= rho and
 * u - hi <= rho in dtype, rho rounded once to dtype; the axis coordinates must be strictly
 * increasing).  Every node within Chebyshev distance rho of the segment is in, so with rho the
 * distance from which k(r) <= tol sig2 on, per output
 *   |dense - windowed| <= tol sig2 |x_n| sum_j |w[s, j]|.
 * An in-window element has the bits hgp_kuf_semi_mc gives it.  A line with x_n = 0, with NaN
 * coordinates or farther than rho from the grid's hull has an empty window: exact zeros.
 * A block is one wave and owns a line and a share of the rows of its outer bounding range; per-lane
 * fp64 sums, a fixed xor butterfly, fp64 partials per share added in order.  No atomics: the same
 * bits on every call with the same arguments on the same device.  Scratch: at most
 * ceil(16 CUs / nobs) * nobs * min(nw, 8) fp64, stream-ordered.
 * nobs = 0 or nw = 0: nothing written, 0 returned.  HGP_E_ARG (before any HIP call): null pointer,
 * bad dtype / kind / ndim / npts, a grid size < 1, nobs / nw < 0, rho negative or not finite,
 * npieces != nobs.  HGP_E_HIP: the launch or the scratch allocation failed. */
int hgp_kuf_semi_mc_matvec_win(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                               const void* x, int64_t nobs, double sig2, double ell, double rho, int npts,
                               const void* u, const int* pieces, int64_t npieces, const void* w, int64_t nw,
                               void* out, void* hip_stream);

/* The same with the analytic SqExp line integral of hgp_kuf_semi_sqexp (SqExp.k_semi ->
 * semi_integrated_sqe, kernels.py:80-85, 223-237): SqExp only; an in-window element has the bits
 * hgp_kuf_semi_sqexp gives it.  Unlike the dense product a line with x_n = 0 gives zeros, not NaN. */
int hgp_kuf_semi_sqexp_matvec_win(int dtype, int ndim, const int64_t* m, const void* const* grids, const void* x,
                                  int64_t nobs, double sig2, double ell, double rho, const int* pieces,
                                  int64_t npieces, const void* w, int64_t nw, void* out, void* hip_stream);

/* hgp_kuf_semi_mc_rmatvec over the same window (kernels.py:19-39 transposed):
 *   out[s, j] = sum_{n: (n, j) in window} c[s, n] Kuf[n, j];  c, out as hgp_kuf_semi_mc_rmatvec.
 * The same set of pairs (one predicate, the same pieces) and the same element values, bit for bit,
 * as hgp_kuf_semi_mc_matvec_win: the two are exact transposes, which a conjugate-gradient solve on
 * K + Kuf^T diag(iv) Kuf needs.  A gather: a block owns a tile of mesh points (the tiles of
 * hgp_kuf_win_bins) and tests all lines against it in chunks of 256, the survivors in line order;
 * products are added in dtype over a chunk, the chunks in fp64.  The tests cost tiles * nobs cheap
 * comparisons.  No atomics, no scratch: the same bits on every call with the same arguments.
 * nobs = 0: out is set to zero; nc = 0: nothing written; both return 0.  Errors as the matvec. */
int hgp_kuf_semi_mc_rmatvec_win(int dtype, int kind, int ndim, const int64_t* m, const void* const* grids,
                                const void* x, int64_t nobs, double sig2, double ell, double rho, int npts,
                                const void* u, const int* pieces, int64_t npieces, const void* c, int64_t nc,
                                void* out, void* hip_stream);

/* The same with the analytic SqExp line integral (kernels.py:80-85, 223-237 transposed): the exact
 * transpose of hgp_kuf_semi_sqexp_matvec_win. */
int hgp_kuf_semi_sqexp_rmatvec_win(int dtype, int ndim, const int64_t* m, const void* const* grids, const void* x,
                                   int64_t nobs, double sig2, double ell, double rho, const int* pieces,
                                   int64_t npieces, const void* c, int64_t nc, void* out, void* hip_stream);

/* Product with random Fourier features, never stored:
 *   acc[i, s] = scale * sum_f w[s, f] cos(2 pi (omega_f . p_i + phase_f)),   out = beta * out + acc,
 *   omega: (nfeat, ndim) rows and phase: (nfeat), both in REVOLUTIONS (radians / 2 pi; the caller
 *   divides in fp64 and rounds to dtype), w: (nw, nfeat) rows; all device arrays of dtype.
 * The points p_i are either the nobs explicit rows of x (nobs, ndim) with grids == NULL (m is not
 * read), or, with x == NULL, the mesh of the ndim grids in mesh order (last axis fastest, the
 * coordinates read from grids and m exactly as hgp_kuf_grid reads them; no (M, ndim) array is
 * built; nobs is not read, npoints = prod m).  Exactly one of x and grids is non-null.
 * transposed = 0: out is (npoints, nw) rows, like hgp_kuf_grid_matvec; transposed != 0: out is
 * (nw, npoints) rows, the PCG layout when the points are the mesh.  With beta = 0 out is never read
 * (it may hold anything, NaN included); beta * out + acc is formed in fp64 and rounded once.
 * With w standard normal and scale = sqrt(2 sig2 / nfeat), omega drawn from the kernel's spectral
 * density and phase uniform, acc is a draw of the prior at the points: the prior half of pathwise
 * conditioning (the reference leaves sample() a TODO, hipgp.py:111-115).
 * A block owns 64 points, one per lane, and sweeps a slice of the features in order; omega, phase
 * and w are wave-uniform loads.  fp32 takes the fractional part of the argument and the hardware
 * cosine (which takes revolutions); fp64 calls cos on 2 pi times the fractional part.  Products are
 * summed in dtype over runs of at most 256 features, the runs in fp64 in feature order.  nsplit:
 * slices the features are cut into (whole units of 64), their fp64 partial sums added in slice
 * order by a second kernel.  0: chosen from (npoints, nfeat) and the device's CU count alone (about
 * 16 blocks per CU, a slice at least 256 features); > 0: that many, at most ceil(nfeat / 64).  No
 * atomics: the same bits on every call with the same arguments on the same device.
 * Scratch, nsplit > 1 only: nsplit * npoints * min(nw, 8) fp64, stream-ordered (hipMallocAsync /
 * hipFreeAsync on hip_stream).
 * npoints = 0 or nw = 0: nothing written, 0 returned.  HGP_E_ARG (before any HIP call): x and grids
 * both given or both null, null m / grids[a] or a grid size < 1 in mesh mode, bad dtype / ndim,
 * nobs / nfeat / nw / nsplit < 0, nfeat < 1 with points present, null omega / phase / w / out.
 * HGP_E_HIP: the launch or the scratch allocation failed (more than 2^31 - 1 blocks). */
int hgp_rff_matvec(int dtype, int ndim, const int64_t* m, const void* const* grids,
                   const void* x, int64_t nobs, const void* omega, const void* phase, int64_t nfeat,
                   const void* w, int64_t nw, double scale, int transposed, double beta,
                   int64_t nsplit, void* out, void* hip_stream);

/* Product with the LINE INTEGRALS of the same features, never stored: the integral of each feature
 * along the segment from the origin to x_i, in closed form,
 *   acc[i, s] = scale * |x_i| * sum_f w[s, f] int_0^1 cos(2 pi (a omega_f . x_i + phase_f)) da
 *             = scale * |x_i| * sum_f w[s, f] cos(2 pi (phase_f + t / 2)) sinc(pi t),  t = omega_f . x_i,
 *   out = beta * out + acc,
 * with omega, phase, w, scale, transposed, beta, nsplit and out exactly as hgp_rff_matvec takes
 * them: with the same (omega, phase, w, scale), acc is the line integral of the prior draw that
 * entry evaluates at points.  Explicit rows x (nobs, ndim) only; there is no mesh mode.
 * The kernel is hgp_rff_matvec's (one lane per line, wave-uniform omega / phase / w, runs of
 * features in dtype and the runs in fp64, nsplit slices with fp64 partials, no atomics, the same
 * bits on every call), with runs of 16 features instead of 256: the sum of one line's terms can
 * cancel, and 256-term fp32 runs then miss the fp32 parity bound.  t / 2 is exact; fp32 takes the hardware cosine of fract(phase + t / 2) and,
 * for |t| >= 0.25 revolutions, the hardware sine of fract(t / 2) times a reciprocal of pi t; for
 * |t| < 0.25 sinc is its even polynomial in (pi t)^2 (five terms in fp32, nine in fp64, whose
 * sine and cosine are libm's).  t = 0 gives sinc = 1 exactly, and a row x = 0 gives acc = 0
 * exactly: |x_i| is applied once, where the sums are stored.
 * Scratch as hgp_rff_matvec (nsplit > 1 only, stream-ordered).
 * nobs = 0 or nw = 0: nothing written, 0 returned.  HGP_E_ARG (before any HIP call): null x, bad
 * dtype / ndim, nobs / nfeat / nw / nsplit < 0, nfeat < 1 with lines present, null omega / phase /
 * w / out.  HGP_E_HIP: the launch or the scratch allocation failed (more than 2^31 - 1 blocks). */
int hgp_rff_line_matvec(int dtype, int ndim, const void* x, int64_t nobs, const void* omega,
                        const void* phase, int64_t nfeat, const void* w, int64_t nw, double scale,
                        int transposed, double beta, int64_t nsplit, void* out, void* hip_stream);

/* Doubly-integrated diagonal Knn_diag by table interpolation,
 * KernelDoublyDiagInterpolator.forward (kernels.py:200-220): table = device array of 3*N
 * values in dtype (distance grid, knn, slopes: the reference's float32 table), x: (nobs,
 * ndim), out: (nobs,). */
int hgp_knn_doubly_diag(int dtype, int ndim, const void* x, int64_t nobs, double sig2, double ell,
                        const void* table, int N, void* out, void* hip_stream);

/* Mean-field natural-gradient statistics of a minibatch (the batch sums
 * of MeanFieldToeplitzGP.elbo_and_grad, hipgp.py:234-250, and a_n of compute_batch_an,
 * hipgp.py:370-414), from kn = R^T K^-1 Knm^T (nrhs, Mp) and the variational mean qm / diagonal
 * covariance qS (Mp,), with per-observation y, ivar = 1/noise^2, Knn_diag, log_sd (nrhs,):
 *   an[n]  = -1/2 ivar_n ((kn_n.qm - y_n)^2 + Knn_n - |kn_n|^2 + kn_n^2.qS) - log_sd_n - ln(2 pi)/2
 *   lam[j] = sum_n ivar_n kn_nj^2,   dm[j] = -sum_n ivar_n (kn_n.qm - y_n) kn_nj
 * All device arrays of dtype; deterministic (fixed reduction order), two reads of kn.
 * Per rank these are the partial sums RCCL all-reduces across the RHS shards. */
int hgp_meanfield_stats(int dtype, const void* kn, int64_t nrhs, int64_t Mp, const void* qm,
                        const void* qS, const void* y, const void* ivar, const void* Knn_diag,
                        const void* log_sd, void* an, void* lam, void* dm, void* hip_stream);

/* The two passes of hgp_meanfield_stats apart, for kn held in column slabs over ranks (grid-block
 * sharding, hipgp_amd/slab.py; same reference lines).  hgp_meanfield_rowdots: for the Mp columns
 * of kn given (qm, qS: the matching slices), out3[n*3 + c] = (kn_n.qm, |kn_n|^2, kn_n^2.qS),
 * fixed reduction order.  A caller all-reduces out3 over the slabs and forms
 * bdiff_n = ivar_n (kn_n.qm - y_n) and a_n from the totals; hgp_meanfield_cols then writes the
 * slab's lam[j] = sum_n ivar_n kn_nj^2 and dm[j] = -sum_n bdiff_n kn_nj (Mp = 0: nothing). */
int hgp_meanfield_rowdots(int dtype, const void* kn, int64_t nrhs, int64_t Mp, const void* qm,
                          const void* qS, void* out3, void* hip_stream);
int hgp_meanfield_cols(int dtype, const void* kn, int64_t nrhs, int64_t Mp, const void* ivar,
                       const void* bdiff, void* lam, void* dm, void* hip_stream);

/* Block-diagonal variational family (BlockToeplitzGP, ziggy/hipgp.py:527-691), SURVEY §8(f) row 3.
 * The expanded grid dims[ndim] (ndim 2 or 3, n_a = 2 m_a - 2) is tiled by blocks[ndim] (each n_a
 * divisible by blocks[a]; points per block bs = prod blocks <= 128), blocks enumerated C-order
 * over the block grid and points C-order inside a block (ziggy/misc/util.py:79-119).
 *   gram[nblk][bs][bs] = sum_n ivar_n kn_{n,blk} kn_{n,blk}^T     (hipgp.py:252-256, get_lam :669-685)
 *   knSkn[nrhs]        = sum_blk kn_{n,blk}^T S_blk kn_{n,blk}    (compute_knSkn :661-664; S [nblk][bs][bs])
 *   trSG[1]            = sum_blk <S_blk, gram_blk>_F = sum_n ivar_n knSkn_n   (the ELBO's a_n sum needs only this)
 * kn (nrhs, M') row layout; gram, knSkn, trSG may each be NULL to skip that output (trSG needs
 * gram; ivar may be NULL without gram, S without knSkn/trSG).  gram is the per-shard sum RCCL
 * all-reduces across RHS shards.  Deterministic. */
int hgp_block_stats(int dtype, int ndim, const int64_t* dims, const int64_t* blocks, const void* kn,
                    int64_t nrhs, const void* ivar, const void* S, void* gram, void* knSkn,
                    void* trSG, void* hip_stream);

/* Backward of the solve w.r.t. the Toeplitz column, SURVEY §8(f) row 4.  Replaces gpytorch's
 * sym_toeplitz_derivative_quadratic_form (reference ziggy/misc/gpt_toeplitz.py:169-209) as
 * InvMatmul.backward calls it (ziggy/misc/_inv_matmul.py:52-60, left_vecs = [L; R],
 * right_vecs = -0.5 [R; L] over the FLATTENED column):
 *   out[i] = sum_j sum_k left_j[k] (right_j[k+i] + right_j[k-i])  (i >= 1, out-of-range terms 0)
 *   out[0] = sum_j left_j . right_j
 * left, right: (nvec, n) row layout (the reference's (n, s) input transposed), out: (n,), all
 * device arrays of dtype.  Direct lagged sums (O(nvec n^2)), deterministic. */
int hgp_sym_toeplitz_dqf(int dtype, const void* left, const void* right, int64_t nvec, int64_t n,
                         void* out, void* hip_stream);

/* hgp_sym_toeplitz_dqf for n = the plan's M, through the grid's factorisation: the flattened-index
 * correlation sum_k u[k] v[k+i] is the fold of the d-D correlation over its signed-digit lags,
 * computed as one fp64 FFT per vector pair on the L_K grid (O(nvec prod L_K log)).  left, right
 * (nvec, M) row layout, out (M,), plan dtype.  Synchronises the plan stream. */
int hgp_plan_dqf(hgp_plan* plan, const void* left, const void* right, int64_t nvec, void* out);

/* Gradient of sum(g * op(x)) w.r.t. the plan's column through the operator's spectrum
 * (K: D, CINV: 1/D, RT and R: D_sqrt; D = clamp(Re FFT_n(circulant_embed(column)), clamp_min),
 * reference toeplitz_tensor.py:20-31, ops :70-125).  The x-gradient is the adjoint operator
 * (K, CINV self-adjoint; R <-> RT) through hgp_toeplitz_apply.  x (nrhs, M) or (nrhs, M') for R,
 * g shaped like op(x); column_grad (M,); device arrays of the plan dtype; fp64 chain (DCT-I pair
 * on the m-grid); the filter correlation is one fp64 cross spectrum per RHS on the L_K / L_R grid.
 * Synchronises the plan stream. */
int hgp_plan_column_grad(hgp_plan* plan, int op, const void* x, const void* g, int64_t nrhs,
                         void* column_grad);

/* Sizes of a plan: M, M' and the padded FFT lengths per axis (K-type and R-type ops). */
int hgp_plan_info(const hgp_plan* plan, int64_t* M, int64_t* Mprime, int64_t* L_K,
                  int64_t* L_R);

/* Device memory a plan holds: scratch (operator workspaces, CG vectors, set-up scratch; all
 * re-allocated on demand) and tables (twiddles, Bluestein DCT tables, spectra; HGP_OP_RSQ's
 * spectrum from its first use until the next hgp_plan_set_column).
 * hgp_plan_trim frees the scratch (after synchronising the plan's streams) and keeps the tables,
 * so an idle plan kept for re-use holds only what its next set-up needs. */
int hgp_plan_mem(const hgp_plan* plan, int64_t* scratch_bytes, int64_t* table_bytes);
int hgp_plan_trim(hgp_plan* plan);
int hgp_plan_destroy(hgp_plan* plan);

const char* hgp_last_error(void);

/* Library/ABI version string. */
const char* hgp_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HIPGP_H */
