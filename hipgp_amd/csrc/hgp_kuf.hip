// hgp_kuf.hip — dense point-observation cross covariance Knm = k(x_n, u_m) on a gridded mesh
// (the PCG right-hand sides, `svi_gp.py:72` -> `kernels.py:73-79, 145-158`), written straight
// into the (B, M) row layout the solve reads.
//
// The reference forms the (B, M, D) broadcast x[:, None, :] - y[None, :, :] and reduces it
// (1.6 GB at C2's 32 x 1M, 13 GB per 200-observation minibatch at 4096^2).  Here one thread
// produces outputs directly: the mesh is (outer, inner) with inner = the last axis; a block
// owns one observation n and one outer index o (uniform per block, so the outer axes'
// squared differences are one scalar), threads stride the last axis.  Same per-element
// arithmetic and axis summation order as the reference, in the tensor dtype.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hgp_kuf_eval.hpp"   // KufGrid, scaled_dist, kern_eval: shared with every product kernel
#include "hgp_kuf_launch.hpp" // KufObs, the grid descriptor and the dtype ladder
#include "hgp_kuf_semi.hpp"   // the line-integral element: its one definition

namespace hgp {

constexpr int KUF_THREADS = 256;
constexpr int KUF_PER_THREAD = 4;
constexpr int KUF_CHUNK = KUF_THREADS * KUF_PER_THREAD;

template <typename T>
__global__ __launch_bounds__(KUF_THREADS) void k_kuf_grid(KufGrid g, const T* __restrict__ x, int64_t B, int kind,
                                                         T sig2, KufVec<T> ell, T* __restrict__ out) {
  const int d = g.d;
  const int64_t inner = g.m[d - 1];
  const int64_t nchunk = (inner + KUF_CHUNK - 1) / KUF_CHUNK;
  int64_t outer = 1;
  for (int a = 0; a < d - 1; ++a) outer *= g.m[a];
  const int64_t bid = blockIdx.x;
  const int64_t chunk = bid % nchunk;
  const int64_t rest = bid / nchunk;
  const int64_t o = rest % outer;
  const int64_t n = rest / outer;
  if (n >= B) return;
  const bool sq = scaled_dist(kind);
  // outer axes: one scalar per block, summed in axis order (as the reference's sum over D)
  auto sqd = [&](int a, int64_t ia, T el) -> T {
    T dv = x[n * d + a] - reinterpret_cast<const T*>(g.g[a])[ia];
    if (sq) dv = dv / el;
    return dv * dv;
  };
  T so = 0;
  if (d == 2) so = sqd(0, o, ell.v[0]);
  if (d == 3) so = sqd(0, o / g.m[1], ell.v[0]) + sqd(1, o % g.m[1], ell.v[1]);
  const T xl = x[n * d + d - 1];
  const T ell_l = kuf_last(ell, d);
  const T* gl = reinterpret_cast<const T*>(g.g[d - 1]);
  T* orow = out + (n * outer + o) * inner;
#pragma unroll
  for (int k = 0; k < KUF_PER_THREAD; ++k) {
    const int64_t i = chunk * KUF_CHUNK + k * KUF_THREADS + threadIdx.x;
    if (i < inner) {
      T dv = xl - gl[i];
      if (sq) dv = dv / ell_l;
      const T s = (d == 1) ? dv * dv : so + dv * dv;
      orow[i] = kern_eval<T>(kind, s, sig2, ell.v[0]);
    }
  }
}


// ---- line-integral (semi-integrated) cross covariance, SURVEY §8(f) row 2 -----------------
// Observation n is the segment from the origin to x_n; Knm[n, j] = |x_n| * int_0^1 k(u_j, a x_n) da.

// Monte-Carlo estimate of `Kernel.k_semi_mc` (kernels.py:19-39, transposed as svi_gp.py:61-64
// uses it): Knm[n, j] = |x_n| * (1/npts) sum_a k(u_j, alpha_a x_n), alpha_a = a/npts + u/npts.
// The reference builds the (M, nobs*npts, D) broadcast; here a block owns (n, outer index o):
// the sample points alpha_a x_n and their outer-axis squared distances are block constants in
// LDS, threads stride the last axis and sum the npts kernel values in registers.  The arithmetic
// is hgp_kuf_semi.hpp's (semi_mc_*), shared with the products.
template <typename T>
__global__ __launch_bounds__(KUF_THREADS) void k_kuf_semi_mc(KufGrid g, const T* __restrict__ x, int64_t B, int kind,
                                                            T sig2, T ell, T kp, int npts,
                                                            const T* __restrict__ u, T* __restrict__ out) {
  __shared__ T so_s[SEMI_MAX_NPTS];   // outer-axis sum of squared distances of sample a
  __shared__ T xl_s[SEMI_MAX_NPTS];   // last coordinate of sample a
  const int d = g.d;
  const int64_t inner = g.m[d - 1];
  const int64_t nchunk = (inner + KUF_CHUNK - 1) / KUF_CHUNK;
  int64_t outer = 1;
  for (int a = 0; a < d - 1; ++a) outer *= g.m[a];
  const int64_t bid = blockIdx.x;
  const int64_t chunk = bid % nchunk;
  const int64_t rest = bid / nchunk;
  const int64_t o = rest % outer;
  const int64_t n = rest / outer;
  if (n >= B) return;
  const bool sq = scaled_dist(kind);
  const T uoff = semi_mc_offset<T>(u, npts);
  for (int a = threadIdx.x; a < npts; a += KUF_THREADS) {
    const T al = semi_mc_alpha<T>(a, npts, uoff);
    so_s[a] = semi_mc_outer<T>(d, [&](int ax) -> T {
      const int64_t ia = d == 2 ? o : (ax == 0 ? o / g.m[1] : o % g.m[1]);
      return semi_mc_sqd<T>(reinterpret_cast<const T*>(g.g[ax])[ia], x[n * d + ax], al, sq, ell);
    });
    xl_s[a] = x[n * d + d - 1] * al;
  }
  __syncthreads();
  const T dist = semi_dist<T>(x, n, d);
  const T* gl = reinterpret_cast<const T*>(g.g[d - 1]);
  T* orow = out + (n * outer + o) * inner;
#pragma unroll
  for (int k = 0; k < KUF_PER_THREAD; ++k) {
    const int64_t i = chunk * KUF_CHUNK + k * KUF_THREADS + threadIdx.x;
    if (i < inner)
      orow[i] = semi_mc_elem<T>(kind, d, gl[i], npts, sq, sig2, ell, kp, dist, [&](int a, T& xl, T& so) {
        xl = xl_s[a];
        so = so_s[a];
      });
  }
}

// Analytic SqExp line integral, `SqExp.k_semi` -> `semi_integrated_sqe` (kernels.py:80-85,
// 223-237) with Sinv = I / ell^2:  a = x S x, b = x S u, c = u S u, scale = sqrt(1/a),
// loc = b/a, Knm = sig2 exp(b^2/(2a) - c/2) sqrt(2 pi) scale (Phi(1) - Phi(0)) |x|, with the
// normal CDFs of ziggy/misc/stats.py:74-76.  Same formula and rounding steps; |x| = 0 gives
// NaN exactly where the reference does.  The arithmetic is hgp_kuf_semi.hpp's (semi_sq_*).
template <typename T>
__global__ __launch_bounds__(KUF_THREADS) void k_kuf_semi_sqexp(KufGrid g, const T* __restrict__ x, int64_t B,
                                                               T sig2, T ell, T* __restrict__ out) {
  const int d = g.d;
  const int64_t inner = g.m[d - 1];
  const int64_t nchunk = (inner + KUF_CHUNK - 1) / KUF_CHUNK;
  int64_t outer = 1;
  for (int a = 0; a < d - 1; ++a) outer *= g.m[a];
  const int64_t bid = blockIdx.x;
  const int64_t chunk = bid % nchunk;
  const int64_t rest = bid / nchunk;
  const int64_t o = rest % outer;
  const int64_t n = rest / outer;
  if (n >= B) return;
  const T sinv = (T)1 / (ell * ell);
  T xs[3];
  const T av = semi_sq_line<T>(x, n, d, sinv, xs);           // xs = xintegrated @ Sinv
  int64_t oi[2] = {0, 0};
  if (d == 2) oi[0] = o;
  if (d == 3) { oi[0] = o / g.m[1]; oi[1] = o % g.m[1]; }
  T bo, co;
  semi_sq_outer<T>(d, xs, sinv, [&](int ax) -> T { return reinterpret_cast<const T*>(g.g[ax])[oi[ax]]; }, bo, co);
  const T dist = semi_dist<T>(x, n, d);
  const T scale = sqrt((T)1 / av);
  const T* gl = reinterpret_cast<const T*>(g.g[d - 1]);
  T* orow = out + (n * outer + o) * inner;
#pragma unroll
  for (int k = 0; k < KUF_PER_THREAD; ++k) {
    const int64_t i = chunk * KUF_CHUNK + k * KUF_THREADS + threadIdx.x;
    if (i < inner) orow[i] = semi_sq_elem<T>(d, bo, co, xs[d - 1], gl[i], sinv, av, scale, sig2, dist);
  }
}

// Doubly-integrated diagonal by table interpolation, `KernelDoublyDiagInterpolator.forward`
// (kernels.py:200-220): r = |x / ell|, lo = #(r > grid) - 1 (-1 wraps to the last entry, as
// torch indexing does), knn[lo] + slopes[lo] (r - grid[lo]), times ell^2 sig2.
template <typename T>
__global__ __launch_bounds__(256) void k_doubly_diag(const T* __restrict__ x, int64_t B, int d, T sig2, T ell,
                                                    const T* __restrict__ tab, int N, T* __restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= B) return;
  T s = 0;
  for (int ax = 0; ax < d; ++ax) {
    const T v = x[n * d + ax] / ell;
    s += v * v;
  }
  const T r = sqrt(s);
  const T* grid = tab;
  const T* knn = tab + N;
  const T* slopes = tab + 2 * N;
  int lo = -1;
  for (int j = 0; j < N; ++j) lo += (r > grid[j]) ? 1 : 0;
  if (lo < 0) lo += N;
  const T iv = knn[lo] + slopes[lo] * (r - grid[lo]);
  out[n] = ell * ell * sig2 * iv;
}

// g from the record; the forwards' tiles: (observation, outer index, chunk of the last axis)
static int64_t kuf_fwd_tiles(const KufObs& o, KufGrid& g) {
  int64_t outer;
  kuf_fill_grid(g, o.ndim, o.m, o.grids, nullptr, &outer);
  return o.nobs * outer * ((o.m[o.ndim - 1] + KUF_CHUNK - 1) / KUF_CHUNK);
}

// launcher behind hgp_kuf_semi_mc (mode 1) / hgp_kuf_semi_sqexp (mode 2)
hipError_t kuf_semi(const KufObs& o, void* out) {
  KufGrid g{};
  const int64_t nb = kuf_fwd_tiles(o, g);
  if (nb > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  return kuf_with_dtype(o.dtype, [&](auto t) {
    using T = decltype(t);
    const T* x = reinterpret_cast<const T*>(o.x);
    if (o.mode == 1)
      hipLaunchKernelGGL((k_kuf_semi_mc<T>), dim3((unsigned)nb), dim3(KUF_THREADS), 0, o.stream, g, x, o.nobs, o.kind,
                         (T)o.sig2, (T)o.ell[0], (T)o.kp, o.npts, reinterpret_cast<const T*>(o.u),
                         reinterpret_cast<T*>(out));
    else
      hipLaunchKernelGGL((k_kuf_semi_sqexp<T>), dim3((unsigned)nb), dim3(KUF_THREADS), 0, o.stream, g, x, o.nobs,
                         (T)o.sig2, (T)o.ell[0], reinterpret_cast<T*>(out));
    return hipGetLastError();
  });
}

hipError_t doubly_diag(int dtype, int ndim, const void* x, int64_t nobs, double sig2, double ell, const void* tab,
                       int N, void* out, hipStream_t s) {
  const unsigned nb = (unsigned)((nobs + 255) / 256);
  if (dtype == HGP_F32)
    hipLaunchKernelGGL((k_doubly_diag<float>), dim3(nb), dim3(256), 0, s, reinterpret_cast<const float*>(x), nobs,
                       ndim, (float)sig2, (float)ell, reinterpret_cast<const float*>(tab), N,
                       reinterpret_cast<float*>(out));
  else
    hipLaunchKernelGGL((k_doubly_diag<double>), dim3(nb), dim3(256), 0, s, reinterpret_cast<const double*>(x), nobs,
                       ndim, sig2, ell, reinterpret_cast<const double*>(tab), N, reinterpret_cast<double*>(out));
  return hipGetLastError();
}

// launcher behind hgp_kuf_grid / hgp_kuf_grid_ard (argument checks in hgp_kuf_api.hip)
hipError_t kuf_grid(const KufObs& o, void* out) {
  KufGrid g{};
  const int64_t nb = kuf_fwd_tiles(o, g);
  if (nb > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  return kuf_with_dtype(o.dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_kuf_grid<T>), dim3((unsigned)nb), dim3(KUF_THREADS), 0, o.stream, g,
                       reinterpret_cast<const T*>(o.x), o.nobs, o.kind, (T)o.sig2, kuf_vec<T>(o.ell),
                       reinterpret_cast<T*>(out));
    return hipGetLastError();
  });
}

// ---- backward of the three cross covariances with respect to (sig2, ell) ---------------------
// With G the upstream gradient (nobs, M) the hyper-parameter gradients are two scalar sums
//   grad2[0] = sum_nj G[n,j] dK[n,j]/dsig2,   grad2[1] = sum_nj G[n,j] dK[n,j]/dell
// (the autograd of kernels.py:73-79, 145-158, 19-39, 80-85, 223-237 builds and keeps the
// (B, M, D) difference, its square, the distance and the exponential for them).  K is recomputed
// per element with the forward's arithmetic, so nothing is stored between forward and backward.
//
// Block map: the forward's tiles (n, outer index o, chunk of the last axis), numbered as the
// forward's blockIdx; at most KUF_GRAD_BLOCKS blocks, block b takes tiles b, b + nblk, ... in
// that order.  Reduction, all in fp64 whatever the tensor dtype and with no atomics, so the
// result is the same bits on every call: a thread adds its terms in tile order; the 64 lanes of
// a wave by the xor butterfly (32, 16, ..., 1); the 4 waves of a block in wave order through
// LDS; one (d/dsig2, d/dell) pair per block to `part`; k_kuf_grad_finish sums the pairs
// (thread t takes pairs t, t + 256, ..., then the same wave and block steps) and writes grad2.
//
// Every kernel is K = sig2 * k0, so dK/dsig2 = k0: the kernel value without the sig2 factor.
// dK/dell = sig2 * kl with, for r = |x - u| and s as in kern_eval:
//   SqExp       k0 = e^{-s/2}, s = r^2/ell^2, ds/dell = -2 s/ell     -> kl = k0 s / ell
//   Matern 1/2  k0 = e^{-r/ell}                                      -> kl = k0 r / ell^2
//   Matern 3/2  k0 = (1 + dp) e^{-dp}, dp = sqrt3 r/ell: dk0/ddp = -dp e^{-dp},
//               ddp/dell = -dp/ell                                   -> kl = dp^2 e^{-dp} / ell
//   Matern 5/2  k0 = (1 + dp + dp^2/3) e^{-dp}, dp = sqrt5 r/ell:
//               dk0/ddp = -dp (1 + dp) e^{-dp} / 3                   -> kl = dp^2 (1 + dp) e^{-dp} / (3 ell)
// all finite and zero at r = 0 (torch's autograd agrees: the squared distance carries no graph
// when x does not require grad, so sqrt'(0) is never multiplied in).
constexpr int KUF_GRAD_BLOCKS = 2048;

template <typename T>
__device__ __forceinline__ void kern_grad_terms(int kind, T s, T ell, T& k0, T& kl) {
  if (kind == HGP_KERN_SQEXP) {
    k0 = exp(-s / (T)2);
    kl = k0 * s / ell;
    return;
  }
  const T r = sqrt(s);
  if (kind == HGP_KERN_MATERN12) {
    k0 = exp(-r / ell);
    kl = k0 * r / (ell * ell);
    return;
  }
  if (kind == HGP_KERN_MATERN32) {
    const T dp = (T)1.7320508075688772935 * r / ell;
    const T e = exp(-dp);
    k0 = ((T)1 + dp) * e;
    kl = dp * dp * e / ell;
    return;
  }
  const T dp = (T)2.2360679774997896964 * r / ell;       // Matern 5/2
  const T e = exp(-dp);
  k0 = ((T)1 + dp + ((T)5 / (T)3) * s / (ell * ell)) * e;
  kl = dp * dp * ((T)1 + dp) * e / ((T)3 * ell);
}

// wave (xor butterfly) then block (wave order) sum of a pair; thread 0 / 1 of the block write it
__device__ __forceinline__ void kuf_block_sum2(double a0, double a1, double* __restrict__ pair) {
  __shared__ double red[2][KUF_THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a0 += __shfl_xor(a0, off, 64);
    a1 += __shfl_xor(a1, off, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = a0; red[1][w] = a1; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = 0;
    for (int k = 0; k < KUF_THREADS / 64; ++k) s += red[threadIdx.x][k];
    pair[threadIdx.x] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(KUF_THREADS) void k_kuf_grid_grad(KufGrid g, const T* __restrict__ x, int kind, T ell,
                                                              const T* __restrict__ gup, int64_t ntile,
                                                              double* __restrict__ part) {
  const int d = g.d;
  const int64_t inner = g.m[d - 1];
  const int64_t nchunk = (inner + KUF_CHUNK - 1) / KUF_CHUNK;
  int64_t outer = 1;
  for (int a = 0; a < d - 1; ++a) outer *= g.m[a];
  const bool sq = scaled_dist(kind);
  const T* gl = reinterpret_cast<const T*>(g.g[d - 1]);
  double a0 = 0, a1 = 0;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t chunk = t % nchunk;
    const int64_t rest = t / nchunk;
    const int64_t o = rest % outer;
    const int64_t n = rest / outer;                         // < nobs: t < ntile = nobs * outer * nchunk
    auto sqd = [&](int a, int64_t ia) -> T {
      T dv = x[n * d + a] - reinterpret_cast<const T*>(g.g[a])[ia];
      if (sq) dv = dv / ell;
      return dv * dv;
    };
    T so = 0;
    if (d == 2) so = sqd(0, o);
    if (d == 3) so = sqd(0, o / g.m[1]) + sqd(1, o % g.m[1]);
    const T xl = x[n * d + d - 1];
    const T* grow = gup + (n * outer + o) * inner;
#pragma unroll
    for (int k = 0; k < KUF_PER_THREAD; ++k) {
      const int64_t i = chunk * KUF_CHUNK + k * KUF_THREADS + threadIdx.x;
      if (i < inner) {
        T dv = xl - gl[i];
        if (sq) dv = dv / ell;
        const T s = (d == 1) ? dv * dv : so + dv * dv;
        T k0, kl;
        kern_grad_terms<T>(kind, s, ell, k0, kl);
        const T gv = grow[i];
        a0 += (double)(gv * k0);
        a1 += (double)(gv * kl);
      }
    }
  }
  kuf_block_sum2(a0, a1, part + 2 * (int64_t)blockIdx.x);
}

// ---- the same backward for SqExp with one length scale per axis (`kernels.py:73-79`) ------------
// K = sig2 k0, k0 = e^{-s/2}, s = sum_a q_a, q_a = ((x_a - u_a) / ell_a)^2 formed as the forward
// forms it.  dq_a/dell_a = -2 q_a / ell_a, so dK/dell_a = sig2 k0 q_a / ell_a: 1 + d sums
//   part[0] = sum G k0,   part[1 + a] = sum G (k0 q_a / ell_a)
// with the tiles, the block map and the fixed-order fp64 reduction of k_kuf_grid_grad.  k0 and the
// first sum have that kernel's bits; with equal ell_a the per-axis sums add up to its dK/dell sum
// to rounding (k0 s / ell there, the axes added here).
constexpr int KUF_ARD_SUMS = 4;   // 1 + the most axes; a grid of fewer leaves the rest zero

// wave (xor butterfly) then block (wave order) sum of KUF_ARD_SUMS values, as kuf_block_sum2
__device__ __forceinline__ void kuf_block_sum4(double (&a)[KUF_ARD_SUMS], double* __restrict__ quad) {
  __shared__ double red[KUF_ARD_SUMS][KUF_THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int q = 0; q < KUF_ARD_SUMS; ++q) a[q] += __shfl_xor(a[q], off, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < KUF_ARD_SUMS; ++q) red[q][w] = a[q];
  }
  __syncthreads();
  if (threadIdx.x < KUF_ARD_SUMS) {
    double s = 0;
    for (int k = 0; k < KUF_THREADS / 64; ++k) s += red[threadIdx.x][k];
    quad[threadIdx.x] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(KUF_THREADS) void k_kuf_grid_grad_ard(KufGrid g, const T* __restrict__ x, KufVec<T> ell,
                                                                  const T* __restrict__ gup, int64_t ntile,
                                                                  double* __restrict__ part) {
  const int d = g.d;
  const int64_t inner = g.m[d - 1];
  const int64_t nchunk = (inner + KUF_CHUNK - 1) / KUF_CHUNK;
  int64_t outer = 1;
  for (int a = 0; a < d - 1; ++a) outer *= g.m[a];
  const T* gl = reinterpret_cast<const T*>(g.g[d - 1]);
  const T ell_l = kuf_last(ell, d);
  double acc[KUF_ARD_SUMS] = {0, 0, 0, 0};
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t chunk = t % nchunk;
    const int64_t rest = t / nchunk;
    const int64_t o = rest % outer;
    const int64_t n = rest / outer;                         // < nobs: t < ntile = nobs * outer * nchunk
    auto sqd = [&](int a, int64_t ia, T el) -> T {
      const T dv = (x[n * d + a] - reinterpret_cast<const T*>(g.g[a])[ia]) / el;
      return dv * dv;
    };
    T q0 = 0, q1 = 0, so = 0;
    if (d == 2) {
      q0 = sqd(0, o, ell.v[0]);
      so = q0;
    }
    if (d == 3) {
      q0 = sqd(0, o / g.m[1], ell.v[0]);
      q1 = sqd(1, o % g.m[1], ell.v[1]);
      so = q0 + q1;
    }
    const T xl = x[n * d + d - 1];
    const T* grow = gup + (n * outer + o) * inner;
#pragma unroll
    for (int k = 0; k < KUF_PER_THREAD; ++k) {
      const int64_t i = chunk * KUF_CHUNK + k * KUF_THREADS + threadIdx.x;
      if (i < inner) {
        const T dv = (xl - gl[i]) / ell_l;
        const T ql = dv * dv;
        const T s = (d == 1) ? ql : so + ql;
        const T k0 = exp(-s / (T)2);
        const T gv = grow[i];
        acc[0] += (double)(gv * k0);
        if (d >= 2) acc[1] += (double)(gv * (k0 * q0 / ell.v[0]));
        if (d == 3) acc[2] += (double)(gv * (k0 * q1 / ell.v[1]));
        const double tl = (double)(gv * (k0 * ql / ell_l));   // the last axis: slot d
        if (d == 1)
          acc[1] += tl;
        else if (d == 2)
          acc[2] += tl;
        else
          acc[3] += tl;
      }
    }
  }
  kuf_block_sum4(acc, part + KUF_ARD_SUMS * (int64_t)blockIdx.x);
}

// the sums of all blocks in a fixed order (fp64), times sig2 for the d/dell_a, in the tensor dtype
template <typename T>
__global__ __launch_bounds__(KUF_THREADS) void k_kuf_grad_finish_ard(const double* __restrict__ part, int np, int d,
                                                                    double sig2, T* __restrict__ grad) {
  __shared__ double tot[KUF_ARD_SUMS];
  double acc[KUF_ARD_SUMS] = {0, 0, 0, 0};
  for (int p = threadIdx.x; p < np; p += KUF_THREADS) {
#pragma unroll
    for (int q = 0; q < KUF_ARD_SUMS; ++q) acc[q] += part[KUF_ARD_SUMS * p + q];
  }
  kuf_block_sum4(acc, tot);
  __syncthreads();
  if (threadIdx.x == 0) grad[0] = (T)tot[0];
  if (threadIdx.x >= 1 && (int)threadIdx.x <= d) grad[threadIdx.x] = (T)(sig2 * tot[threadIdx.x]);
}

// nblk blocks over the forwards' ntile tiles leave one row of `sums` fp64 partials each; finish(part) adds them up
template <typename L, typename F>
static hipError_t kuf_grad_run(const KufObs& o, int sums, L&& launch, F&& finish) {
  KufGrid g{};
  const int64_t ntile = kuf_fwd_tiles(o, g);
  const int nblk = (int)(ntile < KUF_GRAD_BLOCKS ? ntile : KUF_GRAD_BLOCKS);
  double* part = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&part), (size_t)nblk * sums * sizeof(double), o.stream);
  if (e != hipSuccess) return e;
  launch(g, ntile, nblk, part);
  finish(nblk, part);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipFreeAsync(part, o.stream);
}

template <typename T>
static hipError_t kuf_grad_ard_t(const KufObs& o, const void* gup, void* grad) {
  hipStream_t s = o.stream;
  if (o.nobs == 0) return hipMemsetAsync(grad, 0, (size_t)(1 + o.ndim) * sizeof(T), s);
  return kuf_grad_run(
      o, KUF_ARD_SUMS,
      [&](const KufGrid& g, int64_t ntile, int nblk, double* part) {
        hipLaunchKernelGGL((k_kuf_grid_grad_ard<T>), dim3((unsigned)nblk), dim3(KUF_THREADS), 0, s, g,
                           reinterpret_cast<const T*>(o.x), kuf_vec<T>(o.ell), reinterpret_cast<const T*>(gup), ntile,
                           part);
      },
      [&](int nblk, double* part) {
        hipLaunchKernelGGL((k_kuf_grad_finish_ard<T>), dim3(1), dim3(KUF_THREADS), 0, s, part, nblk, o.ndim, o.sig2,
                           reinterpret_cast<T*>(grad));
      });
}

// launcher behind hgp_kuf_grid_grad_ard: SqExp, point observations, grad holds 1 + ndim values
hipError_t kuf_grad_ard(const KufObs& o, const void* gup, void* grad) {
  return kuf_with_dtype(o.dtype, [&](auto t) { return kuf_grad_ard_t<decltype(t)>(o, gup, grad); });
}

// k_semi_mc is |x_n| mean_a k(u_j, alpha_a x_n) and neither |x_n| nor alpha_a depends on the
// hyper-parameters, so both derivatives are |x_n| mean_a of the point terms at the samples.
template <typename T>
__global__ __launch_bounds__(KUF_THREADS) void k_kuf_semi_mc_grad(KufGrid g, const T* __restrict__ x, int kind, T ell,
                                                                 int npts, const T* __restrict__ u,
                                                                 const T* __restrict__ gup, int64_t ntile,
                                                                 double* __restrict__ part) {
  __shared__ T so_s[SEMI_MAX_NPTS];
  __shared__ T xl_s[SEMI_MAX_NPTS];
  const int d = g.d;
  const int64_t inner = g.m[d - 1];
  const int64_t nchunk = (inner + KUF_CHUNK - 1) / KUF_CHUNK;
  int64_t outer = 1;
  for (int a = 0; a < d - 1; ++a) outer *= g.m[a];
  const bool sq = scaled_dist(kind);
  const T uoff = u[0] * (T)(1.0 / (double)npts);
  const T* gl = reinterpret_cast<const T*>(g.g[d - 1]);
  double a0 = 0, a1 = 0;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {   // the same trip count for every thread
    const int64_t chunk = t % nchunk;
    const int64_t rest = t / nchunk;
    const int64_t o = rest % outer;
    const int64_t n = rest / outer;
    __syncthreads();                                          // the last tile's readers are done
    for (int a = threadIdx.x; a < npts; a += KUF_THREADS) {
      const T al = (T)a / (T)npts + uoff;
      auto sqd = [&](int ax, int64_t ia) -> T {
        T dv = reinterpret_cast<const T*>(g.g[ax])[ia] - x[n * d + ax] * al;
        if (sq) dv = dv / ell;
        return dv * dv;
      };
      T so = 0;
      if (d == 2) so = sqd(0, o);
      if (d == 3) so = sqd(0, o / g.m[1]) + sqd(1, o % g.m[1]);
      so_s[a] = so;
      xl_s[a] = x[n * d + d - 1] * al;
    }
    __syncthreads();
    T xn2 = 0;
    for (int ax = 0; ax < d; ++ax) xn2 += x[n * d + ax] * x[n * d + ax];
    const T dist = sqrt(xn2);
    const T* grow = gup + (n * outer + o) * inner;
#pragma unroll
    for (int k = 0; k < KUF_PER_THREAD; ++k) {
      const int64_t i = chunk * KUF_CHUNK + k * KUF_THREADS + threadIdx.x;
      if (i < inner) {
        const T ui = gl[i];
        T acc0 = 0, accl = 0;
        for (int a = 0; a < npts; ++a) {
          T dv = ui - xl_s[a];
          if (sq) dv = dv / ell;
          const T s = (d == 1) ? dv * dv : so_s[a] + dv * dv;
          T k0, kl;
          kern_grad_terms<T>(kind, s, ell, k0, kl);
          acc0 += k0;
          accl += kl;
        }
        const T gv = grow[i];
        a0 += (double)(gv * (acc0 / (T)npts * dist));
        a1 += (double)(gv * (accl / (T)npts * dist));
      }
    }
  }
  kuf_block_sum2(a0, a1, part + 2 * (int64_t)blockIdx.x);
}

// Analytic SqExp line integral: with Sinv = I / ell^2 the forward's terms are
//   a = |x|^2/ell^2, b = x.u/ell^2, c = |u|^2/ell^2,  loc = b/a = x.u/|x|^2   (no ell in it),
//   E = b^2/(2a) - c/2 = -q/(2 ell^2),  q = c ell^2 - b^2 ell^2/a = |u|^2 - (x.u)^2/|x|^2
//   (the squared distance of u from the line), scale = sqrt(1/a) = ell/|x|,
//   za = (1 - loc)/(scale sqrt2) = A/ell, zb = -loc/(scale sqrt2) = B0/ell,
//   A = (1 - loc)|x|/sqrt2, B0 = -loc |x|/sqrt2,
//   K = sig2 k0,  k0 = e^E sqrt(2 pi) scale (erf(za) - erf(zb))/2 |x|
//                    = sqrt(2 pi) ell e^{-q/(2 ell^2)} (erf(A/ell) - erf(B0/ell))/2.
// Differentiating the three factors that hold ell:
//   d(ell)/dell                 -> k0/ell
//   d e^{-q/(2 ell^2)}/dell     -> k0 q/ell^3 = k0 (-2E)/ell
//   d erf(A/ell)/dell = -(2/sqrt pi) e^{-za^2} A/ell^2, likewise B0:
//     sqrt(2 pi) ell e^E (1/2)(2/sqrt pi)(-za e^{-za^2} + zb e^{-zb^2})/ell
//                               -> -sqrt2 e^E (za e^{-za^2} - zb e^{-zb^2})
//   kl = k0 (1 - 2E)/ell - sqrt2 e^E (za e^{-za^2} - zb e^{-zb^2}).
// a, b, c, loc, E, za, zb are formed exactly as in k_kuf_semi_sqexp.
template <typename T>
__global__ __launch_bounds__(KUF_THREADS) void k_kuf_semi_sqexp_grad(KufGrid g, const T* __restrict__ x, T ell,
                                                                    const T* __restrict__ gup, int64_t ntile,
                                                                    double* __restrict__ part) {
  const int d = g.d;
  const int64_t inner = g.m[d - 1];
  const int64_t nchunk = (inner + KUF_CHUNK - 1) / KUF_CHUNK;
  int64_t outer = 1;
  for (int a = 0; a < d - 1; ++a) outer *= g.m[a];
  const T sinv = (T)1 / (ell * ell);
  const T sqrt2 = (T)1.4142135623730950488, sqrt2pi = (T)2.5066282746310005024;
  const T* gl = reinterpret_cast<const T*>(g.g[d - 1]);
  double a0 = 0, a1 = 0;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t chunk = t % nchunk;
    const int64_t rest = t / nchunk;
    const int64_t o = rest % outer;
    const int64_t n = rest / outer;
    T xs[3], ua[3];
    T av = 0, xn2 = 0;
    int64_t oi[2] = {0, 0};
    if (d == 2) oi[0] = o;
    if (d == 3) { oi[0] = o / g.m[1]; oi[1] = o % g.m[1]; }
    for (int ax = 0; ax < d; ++ax) {
      const T xv = x[n * d + ax];
      xs[ax] = xv * sinv;
      av += xs[ax] * xv;
      xn2 += xv * xv;
      if (ax < d - 1) ua[ax] = reinterpret_cast<const T*>(g.g[ax])[oi[ax]];
    }
    T bo = 0, co = 0;
    for (int ax = 0; ax < d - 1; ++ax) {
      bo += xs[ax] * ua[ax];
      co += (ua[ax] * sinv) * ua[ax];
    }
    const T xdist = sqrt(xn2);
    const T scale = sqrt((T)1 / av);
    const T* grow = gup + (n * outer + o) * inner;
#pragma unroll
    for (int k = 0; k < KUF_PER_THREAD; ++k) {
      const int64_t i = chunk * KUF_CHUNK + k * KUF_THREADS + threadIdx.x;
      if (i < inner) {
        const T ui = gl[i];
        const T b = (d == 1) ? xs[0] * ui : bo + xs[d - 1] * ui;
        const T c = (d == 1) ? (ui * sinv) * ui : co + (ui * sinv) * ui;
        const T loc = b / av;
        const T E = (b * b) / ((T)2 * av) - c / (T)2;
        const T eE = exp(E);
        const T za = ((T)1 - loc) / (scale * sqrt2);
        const T zb = ((T)0 - loc) / (scale * sqrt2);
        const T ca = (T)0.5 * ((T)1 + erf(za));
        const T cb = (T)0.5 * ((T)1 + erf(zb));
        const T k0 = eE * sqrt2pi * scale * (ca - cb) * xdist;
        const T kl = k0 * ((T)1 - (T)2 * E) / ell - sqrt2 * eE * (za * exp(-za * za) - zb * exp(-zb * zb));
        const T gv = grow[i];
        a0 += (double)(gv * k0);
        a1 += (double)(gv * kl);
      }
    }
  }
  kuf_block_sum2(a0, a1, part + 2 * (int64_t)blockIdx.x);
}

// the pairs of all blocks in a fixed order (fp64), times sig2 for d/dell, in the tensor dtype
template <typename T>
__global__ __launch_bounds__(KUF_THREADS) void k_kuf_grad_finish(const double* __restrict__ part, int np,
                                                                double sig2, T* __restrict__ grad2) {
  __shared__ double tot[2];
  double a0 = 0, a1 = 0;
  for (int p = threadIdx.x; p < np; p += KUF_THREADS) {
    a0 += part[2 * p];
    a1 += part[2 * p + 1];
  }
  kuf_block_sum2(a0, a1, tot);
  __syncthreads();
  if (threadIdx.x == 0) {
    grad2[0] = (T)tot[0];
    grad2[1] = (T)(sig2 * tot[1]);
  }
}

template <typename T>
static hipError_t kuf_grad_t(const KufObs& o, const void* gup, void* grad2) {
  hipStream_t s = o.stream;
  if (o.nobs == 0) return hipMemsetAsync(grad2, 0, 2 * sizeof(T), s);
  return kuf_grad_run(
      o, 2,
      [&](const KufGrid& g, int64_t ntile, int nblk, double* part) {
        const T* xt = reinterpret_cast<const T*>(o.x);
        const T* gt = reinterpret_cast<const T*>(gup);
        if (o.mode == 0)
          hipLaunchKernelGGL((k_kuf_grid_grad<T>), dim3((unsigned)nblk), dim3(KUF_THREADS), 0, s, g, xt, o.kind,
                             (T)o.ell[0], gt, ntile, part);
        else if (o.mode == 1)
          hipLaunchKernelGGL((k_kuf_semi_mc_grad<T>), dim3((unsigned)nblk), dim3(KUF_THREADS), 0, s, g, xt, o.kind,
                             (T)o.ell[0], o.npts, reinterpret_cast<const T*>(o.u), gt, ntile, part);
        else
          hipLaunchKernelGGL((k_kuf_semi_sqexp_grad<T>), dim3((unsigned)nblk), dim3(KUF_THREADS), 0, s, g, xt,
                             (T)o.ell[0], gt, ntile, part);
      },
      [&](int nblk, double* part) {
        hipLaunchKernelGGL((k_kuf_grad_finish<T>), dim3(1), dim3(KUF_THREADS), 0, s, part, nblk, o.sig2,
                           reinterpret_cast<T*>(grad2));
      });
}

// launcher behind hgp_kuf_grid_grad / hgp_kuf_semi_mc_grad / hgp_kuf_semi_sqexp_grad
hipError_t kuf_grad(const KufObs& o, const void* gup, void* grad2) {
  return kuf_with_dtype(o.dtype, [&](auto t) { return kuf_grad_t<decltype(t)>(o, gup, grad2); });
}

}  // namespace hgp
