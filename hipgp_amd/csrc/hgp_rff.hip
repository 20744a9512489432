// hgp_rff.hip — products with random Fourier features without storing them:
//   acc[i, s] = scale * sum_f w[s, f] cos(2 pi (omega_f . p_i + phase_f)),
//   omega (nfeat, ndim) and phase (nfeat) in REVOLUTIONS (radians / 2 pi), w (nw, nfeat) rows,
//   out = beta * out + acc, as (npoints, nw) rows or, transposed, (nw, npoints) rows (the PCG layout).
// With w standard normal and scale = sqrt(2 sig2 / nfeat) this is a draw of the prior at the points
// p (pathwise conditioning: `ToeplitzInducingGP.predict_samples`); the points are explicit rows or
// the mesh of the inducing grids, whose coordinates are read from the grids as hgp_kuf_grid does.
//
// The structure is hgp_kuf_mv.hip's point kernel with the roles of the mesh and the features
// exchanged.  A block is ONE wave and owns 64 points, one per lane: the lane's coordinates and up to
// 8 accumulators sit in registers.  The block sweeps a slice of the features in order; everything
// indexed by the feature (omega, phase, the w values) is the same for all lanes, so those loads are
// wave-uniform (scalar loads, no LDS).  One cosine feeds NW fused multiply-adds.  nw > 8 runs in
// groups of weight rows (8, 4 or 1 wide; a group's unused slots repeat its last row and are not
// written).  The host scaffold (CU count, row groups, partials, the width ladder) is
// hgp_kuf_launch.hpp's; what the two products here share beyond it is rff_products.
//
// The cosine: the argument is formed in revolutions, reduced to [0, 1) by its fractional part (one
// instruction, exact) and handed to the hardware cosine, which takes revolutions.  At a length
// scale of 0.01 the argument is hundreds of radians; libm's cosf would go through its slow range
// reduction there.  fp64 reduces the same way and calls cos on 2 pi times the fraction.
//
// Summation: products are added in the tensor dtype over runs of at most RFF_RUN consecutive
// features, the runs in fp64 in feature order.  Few points: the features are cut into nsplit slices
// of whole RFF_UNIT-feature units, partial sums part[slice][n][slot] (fp64) are added in slice order
// by k_rff_finish.  No atomics: equal arguments give equal bits.
//
// Line integrals (hgp_rff_line_matvec, k_rff_line_mv): the same draw of the prior integrated along
// the segment from the origin to x_i,
//   acc[i, s] = scale * |x_i| * sum_f w[s, f] int_0^1 cos(2 pi (a omega_f . x_i + phase_f)) da
//             = scale * |x_i| * sum_f w[s, f] cos(2 pi (phase_f + t / 2)) sinc(pi t),   t = omega_f . x_i,
// the product form of [sin(2 pi (t + b)) - sin(2 pi b)] / (2 pi t): no cancellation, and cos(2 pi b)
// as t -> 0.  Same structure (runs of RFF_LINE_RUN features), explicit points only.  h = t / 2 is exact; the cosine is cos_rev(b + h),
// sin(pi t) the hardware sine of fract(h) (revolutions again), the quotient a reciprocal.  The
// hardware sine's error is absolute, so below |t| < RFF_TAU sinc is its even polynomial in (pi t)^2
// (both are evaluated and one is selected: no divergent branch).  t = 0 gives sinc = 1 exactly.
// |x_i| is the lane's own: computed once, applied where the lane's sums are stored, so a row x = 0
// gives exactly 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hgp_kuf_eval.hpp"
#include "hgp_kuf_launch.hpp"

namespace hgp {

constexpr int RFF_TILE = 64;       // points per block (one wave)
constexpr int RFF_UNIT = 64;       // features per unit of the split
constexpr int RFF_RUN = 256;       // longest run summed in the tensor dtype
constexpr int RFF_MIN_UNITS = 4;   // nsplit = 0 leaves a slice at least this many units

// cos(2 pi t) for t in revolutions
__device__ __forceinline__ float cos_rev(float t) { return __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(t)); }
__device__ __forceinline__ double cos_rev(double t) { return cos(6.283185307179586476925 * (t - floor(t))); }

// where the result goes: out[n * sn + s * ss] = beta * (the same element) + scale * sum
struct RffOut {
  int64_t sn, ss;
  double scale, beta;
};

template <typename T>
__device__ __forceinline__ void rff_store(T* __restrict__ out, const RffOut& o, int64_t n, int s, double a) {
  T* p = out + n * o.sn + s * o.ss;
  double v = o.scale * a;
  if (o.beta != 0) v += o.beta * (double)*p;                // beta = 0: out is never read
  *p = (T)v;
}

// x == nullptr: the points are the mesh of g in mesh order (last axis fastest)
template <typename T, int NW>
__global__ __launch_bounds__(RFF_TILE) void k_rff_mv(KufGrid g, const T* __restrict__ x, int64_t B,
                                                     const T* __restrict__ omega, const T* __restrict__ phase,
                                                     int64_t F, const T* __restrict__ w, int nwv, int nsplit,
                                                     int64_t nunit, double* __restrict__ part, T* __restrict__ out,
                                                     RffOut o) {
  const int d = g.d;
  const int64_t slice = (int64_t)blockIdx.x % nsplit;
  const int64_t tile = (int64_t)blockIdx.x / nsplit;
  const int64_t nl = tile * RFF_TILE + threadIdx.x;
  const bool live = nl < B;
  const int64_t n = live ? nl : B - 1;                      // a tail lane repeats the last point
  const int64_t f0 = (slice * nunit / nsplit) * RFF_UNIT;
  int64_t f1 = ((slice + 1) * nunit / nsplit) * RFF_UNIT;
  if (f1 > F) f1 = F;
  T xv[3] = {0, 0, 0};
  if (x != nullptr) {
    xv[0] = x[n * d];
    if (d > 1) xv[1] = x[n * d + 1];
    if (d > 2) xv[2] = x[n * d + 2];
  } else {
    const T* g0 = reinterpret_cast<const T*>(g.g[0]);
    const T* g1 = reinterpret_cast<const T*>(g.g[1]);
    const T* g2 = reinterpret_cast<const T*>(g.g[2]);
    if (d == 1) {
      xv[0] = g0[n];
    } else if (d == 2) {
      xv[0] = g0[n / g.m[1]];
      xv[1] = g1[n % g.m[1]];
    } else {
      const int64_t q = n / g.m[2];
      xv[0] = g0[q / g.m[1]];
      xv[1] = g1[q % g.m[1]];
      xv[2] = g2[n % g.m[2]];
    }
  }
  const T* wp[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) wp[s] = w + (int64_t)(s < nwv ? s : nwv - 1) * F;
  double acc[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) acc[s] = 0;
  for (int64_t i0 = f0; i0 < f1; i0 += RFF_RUN) {
    const int64_t i1 = i0 + RFF_RUN < f1 ? i0 + RFF_RUN : f1;
    T run[NW];
#pragma unroll
    for (int s = 0; s < NW; ++s) run[s] = 0;
#pragma unroll 4
    for (int64_t f = i0; f < i1; ++f) {
      T t = phase[f];                                       // axes added in axis order
      if (d == 1) {
        t += omega[f] * xv[0];
      } else if (d == 2) {
        t += omega[2 * f] * xv[0];
        t += omega[2 * f + 1] * xv[1];
      } else {
        t += omega[3 * f] * xv[0];
        t += omega[3 * f + 1] * xv[1];
        t += omega[3 * f + 2] * xv[2];
      }
      const T c = cos_rev(t);
#pragma unroll
      for (int s = 0; s < NW; ++s) run[s] += c * wp[s][f];
    }
#pragma unroll
    for (int s = 0; s < NW; ++s) acc[s] += (double)run[s];
  }
  if (!live) return;
  if (part != nullptr) {
    double* p = part + (slice * B + n) * NW;
#pragma unroll
    for (int s = 0; s < NW; ++s) p[s] = acc[s];
  } else {
#pragma unroll
    for (int s = 0; s < NW; ++s)
      if (s < nwv) rff_store<T>(out, o, n, s, acc[s]);
  }
}

// the sum over the slices, in slice order, of part[slice][n][s]  (s < nwv of NW slots), stored as above
template <typename T>
__global__ __launch_bounds__(256) void k_rff_finish(const double* __restrict__ part, int nsplit, int64_t B, int NW,
                                                   int nwv, T* __restrict__ out, RffOut o) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= B * NW) return;
  const int64_t n = t / NW;
  const int s = (int)(t % NW);
  if (s >= nwv) return;
  double a = 0;
  for (int k = 0; k < nsplit; ++k) a += part[((int64_t)k * B + n) * NW + s];
  rff_store<T>(out, o, n, s, a);
}

// What the two products share on the host: the split (a pure function of (B, F) and the CU count
// unless the caller forces it), the partials and the groups of weight rows.  launch(W, nb, s0, nwv,
// nsplit, nunit, part, og, o) starts the product's kernel for the group of rows from s0 on, W the
// group's width as a constant.  B > 0, F > 0, nw > 0, nsplit >= 0.
template <typename T, typename L>
static hipError_t rff_products(int64_t B, int64_t F, int64_t nw, double scale, int transposed, double beta,
                               int64_t nsplit_in, T* out, hipStream_t s, L&& launch) {
  const int64_t nunit = (F + RFF_UNIT - 1) / RFF_UNIT;
  const int64_t nrow = (B + RFF_TILE - 1) / RFF_TILE;                          // blocks per slice
  int64_t nsplit = nsplit_in;
  if (nsplit == 0) {
    hipError_t e = hipSuccess;
    const int64_t target = (int64_t)16 * kuf_cus(&e);                          // blocks that fill the device
    if (e != hipSuccess) return e;
    nsplit = (target + nrow - 1) / nrow;
    if (nsplit > nunit / RFF_MIN_UNITS) nsplit = nunit / RFF_MIN_UNITS;
    if (nsplit < 1) nsplit = 1;
  }
  if (nsplit > nunit) nsplit = nunit;
  if (nrow * nsplit > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const unsigned nb = (unsigned)(nrow * nsplit);
  RffOut o{};
  o.sn = transposed ? 1 : nw;
  o.ss = transposed ? B : 1;
  o.scale = scale;
  o.beta = beta;
  return kuf_row_groups(
      nw, nsplit > 1 ? (size_t)nsplit * (size_t)B : 0, s,
      [&](int64_t s0, int NW, int nwv, double* part) {
        kuf_with_width(NW, [&](auto W) { launch(W, nb, s0, nwv, (int)nsplit, nunit, part, out + s0 * o.ss, o); });
      },
      [&](int64_t s0, int NW, int nwv, double* part) {
        const int64_t tot = B * NW;
        hipLaunchKernelGGL((k_rff_finish<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, part, (int)nsplit,
                           B, NW, nwv, out + s0 * o.ss, o);
      });
}

// x == nullptr: the mesh of (m, grids)
template <typename T>
static hipError_t rff_matvec_t(int ndim, const int64_t* m, const void* const* grids, const void* xv, int64_t B,
                               const void* omv, const void* phv, int64_t F, const void* wv, int64_t nw, double scale,
                               int transposed, double beta, int64_t nsplit, void* outv, hipStream_t s) {
  KufGrid g{};
  g.d = ndim;
  if (xv == nullptr) kuf_fill_grid(g, ndim, m, grids);
  const T* x = reinterpret_cast<const T*>(xv);
  const T* omega = reinterpret_cast<const T*>(omv);
  const T* phase = reinterpret_cast<const T*>(phv);
  const T* w = reinterpret_cast<const T*>(wv);
  return rff_products<T>(B, F, nw, scale, transposed, beta, nsplit, reinterpret_cast<T*>(outv), s,
                         [&](auto W, unsigned nb, int64_t s0, int nwv, int ns, int64_t nunit, double* part, T* og,
                             const RffOut& o) {
                           hipLaunchKernelGGL((k_rff_mv<T, decltype(W)::value>), dim3(nb), dim3(RFF_TILE), 0, s, g, x,
                                              B, omega, phase, F, w + s0 * F, nwv, ns, nunit, part, og, o);
                         });
}

// launcher behind hgp_rff_matvec
hipError_t rff_matvec(int dtype, int ndim, const int64_t* m, const void* const* grids, const void* x, int64_t npoints,
                      const void* omega, const void* phase, int64_t nfeat, const void* w, int64_t nw, double scale,
                      int transposed, double beta, int64_t nsplit, void* out, hipStream_t s) {
  if (dtype == HGP_F32)
    return rff_matvec_t<float>(ndim, m, grids, x, npoints, omega, phase, nfeat, w, nw, scale, transposed, beta,
                               nsplit, out, s);
  return rff_matvec_t<double>(ndim, m, grids, x, npoints, omega, phase, nfeat, w, nw, scale, transposed, beta, nsplit,
                              out, s);
}


// ---- line integrals ------------------------------------------------------------------------------
// below |t| < RFF_TAU revolutions sinc(pi t) is a polynomial in u = (pi t)^2 <= 0.617: five terms leave
// u^5 / 11! = 2.2e-9 in fp32, nine terms u^9 / 19! = 1e-19 in fp64; at |t| >= RFF_TAU the quotient
// divides the sine's absolute error by pi t >= 0.785
constexpr double RFF_TAU = 0.25;
// the line kernel's runs in the tensor dtype are 16 features, not RFF_RUN: one line's sum of F terms can
// cancel to a few times one term, and 256-term fp32 runs then leave 5e-6 of it where torch leaves 3e-7
// (measured, F = 1000); the rounding of fp32 runs grows as sqrt(F * run), 16 brings it down 4 x
constexpr int RFF_LINE_RUN = 16;

// sin(2 pi t) for t in revolutions
__device__ __forceinline__ float sin_rev(float t) { return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(t)); }
__device__ __forceinline__ double sin_rev(double t) { return sin(6.283185307179586476925 * (t - floor(t))); }

// sinc(pi t) = sin(pi t) / (pi t) from t and h = t / 2, both in revolutions
__device__ __forceinline__ float sinc_rev(float t, float h) {
  const float p = 3.14159265358979323846f * t;
  const float u = p * p;
  float q = fmaf(u, 1.f / 362880.f, -1.f / 5040.f);
  q = fmaf(u, q, 1.f / 120.f);
  q = fmaf(u, q, -1.f / 6.f);
  q = fmaf(u, q, 1.f);
  const float r = sin_rev(h) * __builtin_amdgcn_rcpf(p);
  return fabsf(t) < (float)RFF_TAU ? q : r;
}
__device__ __forceinline__ double sinc_rev(double t, double h) {
  const double p = 3.14159265358979323846 * t;
  if (fabs(t) >= RFF_TAU) return sin_rev(h) / p;
  const double u = p * p;
  double q = fma(u, 1. / 355687428096000., -1. / 1307674368000.);       // 1/17!, -1/15!
  q = fma(u, q, 1. / 6227020800.);                                      // 1/13!
  q = fma(u, q, -1. / 39916800.);                                       // -1/11!
  q = fma(u, q, 1. / 362880.);
  q = fma(u, q, -1. / 5040.);
  q = fma(u, q, 1. / 120.);
  q = fma(u, q, -1. / 6.);
  return fma(u, q, 1.);
}

// k_rff_mv for line integrals to the rows of x (B, d); `part` and `out` as there
template <typename T, int NW>
__global__ __launch_bounds__(RFF_TILE) void k_rff_line_mv(int d, const T* __restrict__ x, int64_t B,
                                                          const T* __restrict__ omega, const T* __restrict__ phase,
                                                          int64_t F, const T* __restrict__ w, int nwv, int nsplit,
                                                          int64_t nunit, double* __restrict__ part,
                                                          T* __restrict__ out, RffOut o) {
  const int64_t slice = (int64_t)blockIdx.x % nsplit;
  const int64_t tile = (int64_t)blockIdx.x / nsplit;
  const int64_t nl = tile * RFF_TILE + threadIdx.x;
  const bool live = nl < B;
  const int64_t n = live ? nl : B - 1;                      // a tail lane repeats the last point
  const int64_t f0 = (slice * nunit / nsplit) * RFF_UNIT;
  int64_t f1 = ((slice + 1) * nunit / nsplit) * RFF_UNIT;
  if (f1 > F) f1 = F;
  T xv[3] = {0, 0, 0};
  xv[0] = x[n * d];
  if (d > 1) xv[1] = x[n * d + 1];
  if (d > 2) xv[2] = x[n * d + 2];
  const T len = sqrt(xv[0] * xv[0] + xv[1] * xv[1] + xv[2] * xv[2]);
  const T* wp[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) wp[s] = w + (int64_t)(s < nwv ? s : nwv - 1) * F;
  double acc[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) acc[s] = 0;
  for (int64_t i0 = f0; i0 < f1; i0 += RFF_LINE_RUN) {
    const int64_t i1 = i0 + RFF_LINE_RUN < f1 ? i0 + RFF_LINE_RUN : f1;
    T run[NW];
#pragma unroll
    for (int s = 0; s < NW; ++s) run[s] = 0;
#pragma unroll 4
    for (int64_t f = i0; f < i1; ++f) {
      T t;                                                  // axes added in axis order
      if (d == 1) {
        t = omega[f] * xv[0];
      } else if (d == 2) {
        t = omega[2 * f] * xv[0];
        t += omega[2 * f + 1] * xv[1];
      } else {
        t = omega[3 * f] * xv[0];
        t += omega[3 * f + 1] * xv[1];
        t += omega[3 * f + 2] * xv[2];
      }
      const T h = (T)0.5 * t;
      const T c = cos_rev(phase[f] + h) * sinc_rev(t, h);
#pragma unroll
      for (int s = 0; s < NW; ++s) run[s] += c * wp[s][f];
    }
#pragma unroll
    for (int s = 0; s < NW; ++s) acc[s] += (double)run[s];
  }
  if (!live) return;
  if (part != nullptr) {
    double* p = part + (slice * B + n) * NW;
#pragma unroll
    for (int s = 0; s < NW; ++s) p[s] = acc[s] * (double)len;
  } else {
#pragma unroll
    for (int s = 0; s < NW; ++s)
      if (s < nwv) rff_store<T>(out, o, n, s, acc[s] * (double)len);
  }
}

// B > 0 rows of x; the rest as rff_matvec_t
template <typename T>
static hipError_t rff_line_matvec_t(int ndim, const void* xv, int64_t B, const void* omv, const void* phv, int64_t F,
                                    const void* wv, int64_t nw, double scale, int transposed, double beta,
                                    int64_t nsplit, void* outv, hipStream_t s) {
  const T* x = reinterpret_cast<const T*>(xv);
  const T* omega = reinterpret_cast<const T*>(omv);
  const T* phase = reinterpret_cast<const T*>(phv);
  const T* w = reinterpret_cast<const T*>(wv);
  return rff_products<T>(B, F, nw, scale, transposed, beta, nsplit, reinterpret_cast<T*>(outv), s,
                         [&](auto W, unsigned nb, int64_t s0, int nwv, int ns, int64_t nunit, double* part, T* og,
                             const RffOut& o) {
                           hipLaunchKernelGGL((k_rff_line_mv<T, decltype(W)::value>), dim3(nb), dim3(RFF_TILE), 0, s,
                                              ndim, x, B, omega, phase, F, w + s0 * F, nwv, ns, nunit, part, og, o);
                         });
}

// launcher behind hgp_rff_line_matvec
hipError_t rff_line_matvec(int dtype, int ndim, const void* x, int64_t nobs, const void* omega, const void* phase,
                           int64_t nfeat, const void* w, int64_t nw, double scale, int transposed, double beta,
                           int64_t nsplit, void* out, hipStream_t s) {
  if (dtype == HGP_F32)
    return rff_line_matvec_t<float>(ndim, x, nobs, omega, phase, nfeat, w, nw, scale, transposed, beta, nsplit, out, s);
  return rff_line_matvec_t<double>(ndim, x, nobs, omega, phase, nfeat, w, nw, scale, transposed, beta, nsplit, out, s);
}

}  // namespace hgp
