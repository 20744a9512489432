// hgp_kuf_semi.hpp — the element of the line-integral cross covariances, Kuf[n, j] = |x_n| *
// int_0^1 k(u_j, a x_n) da by the Monte-Carlo mean (semi_mc_*) or SqExp's closed form (semi_sq_*):
// its one definition, operations and their order.  The forwards (k_kuf_semi_mc, k_kuf_semi_sqexp:
// hgp_kuf.hip), the dense products (k_kuf_semi_mv, k_kuf_semi_rmv) and the windowed ones
// (hgp_kuf_line_win.hip) all form it through these functions, so it has the same bits in all.
//
// hipcc contracts a product and a sum into one fused multiply-add where both meet in one basic
// block.  The forwards and the dense products form the per-row terms (so, xl of a Monte-Carlo
// node; bo, co of the analytic form) ahead of the element, in LDS or ahead of the last-axis loop,
// so there they arrive as finished, rounded values.  A kernel that forms them next to the element
// itself passes them through semi_rounded first: the compiler then sees a finished value too, and
// pairs the same operations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hgp_kuf_eval.hpp"

namespace hgp {

// v as a finished value: no operation that formed it is contracted with one that uses it
__device__ __forceinline__ float semi_rounded(float v) {
  asm("" : "+v"(v));
  return v;
}
__device__ __forceinline__ double semi_rounded(double v) {
  asm("" : "+v"(v));
  return v;
}

// |x_n|, the axes added in order (d is the kernel's argument, not a constant: one fused
// multiply-add per axis, as the forwards)
template <typename T>
__device__ __forceinline__ T semi_dist(const T* __restrict__ x, int64_t n, int d) {
  T xn2 = 0;
  for (int ax = 0; ax < d; ++ax) xn2 += x[n * d + ax] * x[n * d + ax];
  return sqrt(xn2);
}

// ---- Monte-Carlo nodes: alpha_a = a / npts + u / npts ----------------------------------------
template <typename T>
__device__ __forceinline__ T semi_mc_offset(const T* __restrict__ u, int npts) {
  return u[0] * (T)(1.0 / (double)npts);                    // torch.rand(1) * delta
}

template <typename T>
__device__ __forceinline__ T semi_mc_alpha(int a, int npts, T uoff) {
  return (T)a / (T)npts + uoff;                             // arange(npts) / npts + rand * delta
}

// one axis' squared (SqExp: scaled) distance of the node alpha x to the coordinate gv
template <typename T>
__device__ __forceinline__ T semi_mc_sqd(T gv, T xv, T al, bool sq, T ell) {
  T dv = gv - xv * al;                                      // u - alpha x
  if (sq) dv = dv / ell;
  return dv * dv;
}

// the outer axes' sum of a node; sqd(ax) is semi_mc_sqd of axis ax at the row's index
template <typename T, typename F>
__device__ __forceinline__ T semi_mc_outer(int d, F&& sqd) {
  T so = 0;
  if (d == 2) so = sqd(0);
  if (d == 3) so = sqd(0) + sqd(1);
  return so;
}

// |x| * mean_a k(u, alpha_a x) for the last-axis coordinate ui; node(a, xl, so) hands out the
// node's last coordinate alpha_a x_l and its outer sum, both finished values
template <typename T, typename F>
__device__ __forceinline__ T semi_mc_elem(int kind, int d, T ui, int npts, bool sq, T sig2, T ell, T kp, T dist,
                                          F&& node) {
  T ka = 0;
  for (int a = 0; a < npts; ++a) {
    T xl, so;
    node(a, xl, so);
    T dv = ui - xl;
    if (sq) dv = dv / ell;
    const T sv = (d == 1) ? dv * dv : so + dv * dv;
    ka += kern_eval<T>(kind, sv, sig2, ell, kp);
  }
  return ka / (T)npts * dist;                               // mean(dim=-1) * dists
}

// ---- the analytic SqExp form: a = x S x, b = x S u, c = u S u, S = I / ell^2 -------------------
// xs = x S and a, the axes in order
template <typename T>
__device__ __forceinline__ T semi_sq_line(const T* __restrict__ x, int64_t n, int d, T sinv, T (&xs)[3]) {
  T av = 0;
  for (int ax = 0; ax < d; ++ax) {
    const T xv = x[n * d + ax];
    xs[ax] = xv * sinv;
    av += xs[ax] * xv;
  }
  return av;
}

// The analytic form's sums of products, with their roundings spelled out: one fused multiply-add
// per axis onto the finished sum of the axes before it.  That pairing is the definition: contraction
// is off here and every fused multiply-add is written out, so the element does not depend on how
// hipcc would pair the products of a kernel that holds the coordinates in registers (hoisted,
// selected or fused another way from kernel to kernel).
__device__ __forceinline__ float semi_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double semi_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the outer axes' terms of b and c, in axis order; ua(ax) is the row's coordinate on axis ax
template <typename T, typename F>
__device__ __forceinline__ void semi_sq_outer(int d, const T (&xs)[3], T sinv, F&& ua, T& bo, T& co) {
#pragma clang fp contract(off)
  bo = 0;
  co = 0;
  for (int ax = 0; ax < d - 1; ++ax) {
    const T uv = ua(ax);
    bo = semi_fma(xs[ax], uv, bo);
    co = semi_fma(uv * sinv, uv, co);
  }
}

// the element for the last-axis coordinate ui; xsl = xs[d - 1], scale = sqrt(1 / a)
template <typename T>
__device__ __forceinline__ T semi_sq_elem(int d, T bo, T co, T xsl, T ui, T sinv, T av, T scale, T sig2, T dist) {
  const T sqrt2 = (T)1.4142135623730950488, sqrt2pi = (T)2.5066282746310005024;
  T b, c;
  {
#pragma clang fp contract(off)
    b = (d == 1) ? xsl * ui : semi_fma(xsl, ui, bo);
    c = (d == 1) ? (ui * sinv) * ui : semi_fma(ui * sinv, ui, co);
  }
  const T loc = b / av;
  const T coef = sig2 * exp((b * b) / ((T)2 * av) - c / (T)2) * sqrt2pi * scale;
  const T ca = (T)0.5 * ((T)1 + erf(((T)1 - loc) / (scale * sqrt2)));
  const T cb = (T)0.5 * ((T)1 + erf(((T)0 - loc) / (scale * sqrt2)));
  return coef * (ca - cb) * dist;
}

// ---- sums of a block of 256 threads in a fixed order --------------------------------------------
constexpr int SEMI_THREADS = 256;

// the NW sums of a block: lanes by the xor butterfly, waves in wave order
template <int NW>
__device__ __forceinline__ void semi_block_sum(double (&a)[NW], double* __restrict__ dst, int nwv) {
  __shared__ double red[SEMI_THREADS / 64][NW];
#pragma unroll
  for (int s = 0; s < NW; ++s)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a[s] += __shfl_xor(a[s], off, 64);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int s = 0; s < NW; ++s) red[wv][s] = a[s];
  }
  __syncthreads();
  if ((int)threadIdx.x < nwv) {
    double t = 0;
    for (int k = 0; k < SEMI_THREADS / 64; ++k) t += red[k][threadIdx.x];
    dst[threadIdx.x] = t;
  }
}

// out[n, s] = sum over the slices, in slice order, of part[slice][n][s]  (s < nwv of NW slots)
template <typename T>
__global__ __launch_bounds__(256) void k_kuf_mv_finish(const double* __restrict__ part, int nsplit, int64_t B, int NW,
                                                    int nwv, T* __restrict__ out, int64_t ldo) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= B * NW) return;
  const int64_t n = t / NW;
  const int s = (int)(t % NW);
  if (s >= nwv) return;
  double a = 0;
  for (int k = 0; k < nsplit; ++k) a += part[((int64_t)k * B + n) * NW + s];
  out[n * ldo + s] = (T)a;
}

}  // namespace hgp
