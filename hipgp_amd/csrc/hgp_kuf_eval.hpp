// hgp_kuf_eval.hpp — the per-element arithmetic of the grid cross covariances, shared by the
// kernels that write Kuf (hgp_kuf.hip) and the ones that multiply by it without storing it
// (hgp_kuf_mv.hip), so both produce the same element values.
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

constexpr int SEMI_MAX_NPTS = 1024;

}  // namespace hgp
