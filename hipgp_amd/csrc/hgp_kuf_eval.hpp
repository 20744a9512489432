// hgp_kuf_eval.hpp — the per-element arithmetic of the grid cross covariances, shared by the
// kernels that write Kuf (hgp_kuf.hip) and the ones that multiply by it without storing it, dense
// (hgp_kuf_mv.hip, hgp_kuf_rmv.hip) or over a window of pairs (hgp_kuf_win.hip,
// hgp_kuf_line_win.hip through hgp_kuf_semi.hpp), so all produce the same element values.  The
// grid descriptor KufGrid is also what hgp_rff.hip reads its mesh points from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hipgp.h"

namespace hgp {

struct KufGrid {
  int d;
  int64_t m[3];
  const void* g[3];
};

// One value per axis, by value in the kernel arguments: the length scales of the point kernels
// (SqExp divides axis a by v[a], `kernels.py:73-79` with a vector ell; Matern reads v[0] alone, its
// one ell) and the radii of the window.  A scalar caller's value stands in all three, and then
// every kernel forms what it formed from the one value.
template <typename T>
struct KufVec {
  T v[3];
};

// v[d - 1] of a d-axis grid without a run-time index into the kernel arguments
template <typename T>
__host__ __device__ __forceinline__ T kuf_last(const KufVec<T>& e, int d) {
  return d == 1 ? e.v[0] : (d == 2 ? e.v[1] : e.v[2]);
}

// v[a] likewise, a in {0, 1, 2}
template <typename T>
__host__ __device__ __forceinline__ T kuf_at(const KufVec<T>& e, int a) {
  return a == 0 ? e.v[0] : (a == 1 ? e.v[1] : e.v[2]);
}

// from three host doubles, each rounded once to T
template <typename T>
inline KufVec<T> kuf_vec(const double* p) {
  KufVec<T> e;
  for (int a = 0; a < 3; ++a) e.v[a] = (T)p[a];
  return e;
}

// s: SqExp / Gneiting -> sum ((x - y) / ell)^2 ; Matern -> sum (x - y)^2   (as the reference)
__host__ __device__ inline bool scaled_dist(int kind) { return kind == HGP_KERN_SQEXP || kind == HGP_KERN_GNEITING; }

template <typename T>
__device__ __forceinline__ T kern_eval(int kind, T s, T sig2, T ell, T kp = (T)1) {
  if (kind == HGP_KERN_SQEXP) return sig2 * exp(-s / (T)2);
  const T r = sqrt(s);
  if (kind == HGP_KERN_MATERN12) return sig2 * exp(-r / ell);
  if (kind == HGP_KERN_MATERN32) {
    const T dp = (T)1.7320508075688772935 * r / ell;
    return sig2 * (((T)1 + dp) * exp(-dp));
  }
  if (kind == HGP_KERN_GNEITING) {   // kernels.py:108-117: r = t, kp = alpha, zero beyond t = 1
    const T pit = (T)3.14159265358979323846 * r;
    T c = ((T)1 - r) * cos(pit) + ((T)1 / (T)3.14159265358979323846) * sin(pit);
    c = pow((T)1 + pow(r, kp), (T)-3) * c;
    return r > (T)1 ? (T)0 * sig2 : sig2 * c;
  }
  const T dp = (T)2.2360679774997896964 * r / ell;       // Matern 5/2
  return sig2 * (((T)1 + dp + ((T)5 / (T)3) * s / (ell * ell)) * exp(-dp));
}

// ---- the point squared distance with its roundings spelled out ----------------------------------
// In k_kuf_grid and k_kuf_grid_mv the outer axes' sum is a finished value formed ahead of the
// last-axis term, and hipcc contracts what is left in one way only: so = d0^2 (2-D) or
// fma(d0, d0, d1^2) (3-D), s = fma(dl, dl, so), s = dl^2 (1-D; fma(dl, dl, 0) has the same bits).
// A kernel in which all three products meet in one expression could get them paired differently
// (SqExp at s = 60 turns one ulp of s into 4e-6 of the value), so there contraction is off and
// that pairing is written with explicit fused multiply-adds.
__device__ __forceinline__ float kuf_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double kuf_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the (SqExp: scaled) difference of one axis, as k_kuf_grid forms it
template <typename T, int KIND>
__device__ __forceinline__ T kuf_axis(T x, T u, T ell) {
  constexpr bool sq = KIND == HGP_KERN_SQEXP || KIND == HGP_KERN_GNEITING;
  T dv = x - u;
  if (sq) dv = dv / ell;
  return dv;
}

// the outer axes' squared distance from their differences d0, d1 (d axes in all)
template <typename T>
__device__ __forceinline__ T kuf_outer(int d, T d0, T d1) {
#pragma clang fp contract(off)
  if (d == 1) return (T)0;
  if (d == 2) return d0 * d0;
  return kuf_fma(d0, d0, d1 * d1);
}

// the whole squared distance; dl is the last axis' difference
template <typename T>
__device__ __forceinline__ T kuf_sqdist(int d, T d0, T d1, T dl) {
  return kuf_fma(dl, dl, kuf_outer<T>(d, d0, d1));
}

constexpr int SEMI_MAX_NPTS = 1024;

}  // namespace hgp
