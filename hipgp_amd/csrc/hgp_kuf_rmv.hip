// hgp_kuf_rmv.hip — products with the TRANSPOSED grid cross covariances without storing them:
//   out[s, j] = sum_n Kuf[n, j] c[s, n],   Kuf (nobs, M) as hgp_kuf.hip writes it, c (nc, nobs) rows.
// The sibling of hgp_kuf_mv.hip (out = Kuf w^T).  With both, the operator of
//   (K + Kuf^T diag(iv) Kuf) beta = Kuf^T (iv o y)
// runs matrix-free, which is the optimal variational mean of all observations at once
// (`ToeplitzInducingGP.fit_mean`).  Element values come from the same device functions as the
// forwards (hgp_kuf_eval.hpp; line integrals: hgp_kuf_semi.hpp), the host scaffold from
// hgp_kuf_launch.hpp.
//
// Point observations (k_kuf_grid_rmv), the hot path: compute bound, nobs * M kernel values each
// used nc times.  The roles of k_kuf_grid_mv turned round: a block is ONE wave and owns a tile of
// 64 mesh points, one per lane: the lane's grid coordinates and up to 8 accumulators sit in
// registers.  The block sweeps a slice of the observations in order; everything indexed by the
// observation (its coordinates, the nc coefficients) is the same for all lanes, so those loads
// are wave-uniform (scalar loads, no LDS, no barrier, no vector load in the loop).  One kernel
// evaluation feeds NC fused multiply-adds.  nc > 8 runs in groups of coefficient rows (8, 4 or 1
// wide; a group's unused slots repeat its last row and are not written).
//
// Summation: products are added in the tensor dtype over runs of at most RMV_RUN consecutive
// observations, the runs in fp64 in observation order.  Few mesh points: the observations are cut
// into nsplit slices of whole runs, partial sums part[slice][s][j] (fp64) are added in slice
// order by k_kuf_rmv_finish.  No atomics: equal arguments give equal bits.
//
// Line-integral observations (k_kuf_semi_rmv): a block is one wave and owns one outer mesh index
// and 64 points of the last axis, one per lane; it walks its slice of the observations in order
// and every lane adds (double)(Kuf * c) to its own fp64 sums.  For the Monte-Carlo integral the
// sample table of (observation, outer index) is rebuilt in LDS between two barriers, as the
// forward's product does per outer index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hgp_kuf_eval.hpp"
#include "hgp_kuf_launch.hpp"
#include "hgp_kuf_semi.hpp"

namespace hgp {

constexpr int RMV_TILE = 64;      // mesh points per block (one wave), both kernels
constexpr int RMV_RUN = 256;      // longest run summed in the tensor dtype; the unit of the split

// One run [r0, r1) of observations for the lane's mesh point (u0, u1, ul): run[s] += Kuf * c.
// D is the number of axes.  All three axes' products meet in one expression here, so the squared
// distance is kuf_sqdist's, with the forward's roundings spelled out.
template <typename T, int KIND, int NC, int D>
__device__ __forceinline__ void rmv_run(const T* __restrict__ x, int64_t r0, int64_t r1, T u0, T u1, T ul, T sig2,
                                        const KufVec<T>& ell, const T* const (&cp)[NC], T (&run)[NC]) {
#pragma unroll 4
  for (int64_t n = r0; n < r1; ++n) {
    const T d0 = D >= 2 ? kuf_axis<T, KIND>(x[n * D], u0, ell.v[0]) : (T)0;
    const T d1 = D == 3 ? kuf_axis<T, KIND>(x[n * D + 1], u1, ell.v[1]) : (T)0;
    const T dv = kuf_axis<T, KIND>(x[n * D + D - 1], ul, ell.v[D - 1]);
    const T sv = kuf_sqdist<T>(D, d0, d1, dv);
    const T kv = kern_eval<T>(KIND, sv, sig2, ell.v[0]);
#pragma unroll
    for (int s = 0; s < NC; ++s) run[s] += kv * cp[s][n];
  }
}

template <typename T, int KIND, int NC>
__global__ __launch_bounds__(RMV_TILE) void k_kuf_grid_rmv(KufGrid g, const T* __restrict__ x, int64_t B, T sig2,
                                                          KufVec<T> ell, const T* __restrict__ c, int ncv, int64_t M,
                                                          int nsplit, int64_t nrun, double* __restrict__ part,
                                                          T* __restrict__ out) {
  const int d = g.d;
  const int64_t slice = (int64_t)blockIdx.x % nsplit;
  const int64_t tile = (int64_t)blockIdx.x / nsplit;
  const int64_t jl = tile * RMV_TILE + threadIdx.x;
  const bool live = jl < M;
  const int64_t j = live ? jl : M - 1;                      // a tail lane repeats the last mesh point
  const int64_t n0 = (slice * nrun / nsplit) * RMV_RUN;
  int64_t n1 = ((slice + 1) * nrun / nsplit) * RMV_RUN;
  if (n1 > B) n1 = B;
  // the lane's mesh point: C order, last axis fastest
  const int64_t inner = g.m[d - 1];
  const int64_t o = j / inner;
  const T ul = reinterpret_cast<const T*>(g.g[d - 1])[j % inner];
  T u0 = 0, u1 = 0;
  if (d == 2) u0 = reinterpret_cast<const T*>(g.g[0])[o];
  if (d == 3) {
    u0 = reinterpret_cast<const T*>(g.g[0])[o / g.m[1]];
    u1 = reinterpret_cast<const T*>(g.g[1])[o % g.m[1]];
  }
  const T* cp[NC];
#pragma unroll
  for (int s = 0; s < NC; ++s) cp[s] = c + (int64_t)(s < ncv ? s : ncv - 1) * B;
  double acc[NC];
#pragma unroll
  for (int s = 0; s < NC; ++s) acc[s] = 0;
  for (int64_t r0 = n0; r0 < n1; r0 += RMV_RUN) {
    const int64_t r1 = r0 + RMV_RUN < n1 ? r0 + RMV_RUN : n1;
    T run[NC];
#pragma unroll
    for (int s = 0; s < NC; ++s) run[s] = 0;
    if (d == 1)
      rmv_run<T, KIND, NC, 1>(x, r0, r1, u0, u1, ul, sig2, ell, cp, run);
    else if (d == 2)
      rmv_run<T, KIND, NC, 2>(x, r0, r1, u0, u1, ul, sig2, ell, cp, run);
    else
      rmv_run<T, KIND, NC, 3>(x, r0, r1, u0, u1, ul, sig2, ell, cp, run);
#pragma unroll
    for (int s = 0; s < NC; ++s) acc[s] += (double)run[s];
  }
  if (!live) return;
  if (part != nullptr) {
    double* p = part + slice * NC * M + j;
#pragma unroll
    for (int s = 0; s < NC; ++s) p[(int64_t)s * M] = acc[s];
  } else {
#pragma unroll
    for (int s = 0; s < NC; ++s)
      if (s < ncv) out[(int64_t)s * M + j] = (T)acc[s];
  }
}

// out[s, j] = sum over the slices, in slice order, of part[slice][s][j]  (s < ncv of NC slots)
template <typename T>
__global__ __launch_bounds__(256) void k_kuf_rmv_finish(const double* __restrict__ part, int nsplit, int64_t M, int NC,
                                                       int ncv, T* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * ncv) return;                                 // t = s * M + j with s < ncv
  const int64_t stride = (int64_t)NC * M;
  double a = 0;
  for (int k = 0; k < nsplit; ++k) a += part[k * stride + t];
  out[t] = (T)a;
}

// MODE 1: the Monte-Carlo line integral of k_kuf_semi_mc; MODE 2: the analytic SqExp one of
// k_kuf_semi_sqexp.  Block (outer index o, 64 points of the last axis, slice of the observations);
// element values by hgp_kuf_semi.hpp (MODE 1; MODE 2 see below).
template <typename T, int MODE, int NC>
__global__ __launch_bounds__(RMV_TILE) void k_kuf_semi_rmv(KufGrid g, const T* __restrict__ x, int64_t B, int kind,
                                                          T sig2, T ell, T kp, int npts, const T* __restrict__ u,
                                                          const T* __restrict__ c, int ncv, int64_t M, int nsplit,
                                                          int64_t nrun, int64_t nchunk, double* __restrict__ part,
                                                          T* __restrict__ out) {
  __shared__ T so_s[MODE == 1 ? SEMI_MAX_NPTS : 1];
  __shared__ T xl_s[MODE == 1 ? SEMI_MAX_NPTS : 1];
  const int d = g.d;
  const int64_t inner = g.m[d - 1];
  const int64_t slice = (int64_t)blockIdx.x % nsplit;
  const int64_t tile = (int64_t)blockIdx.x / nsplit;
  const int64_t o = tile / nchunk;                          // < outer: the grid is outer * nchunk * nsplit blocks
  const int64_t il = (tile % nchunk) * RMV_TILE + threadIdx.x;
  const bool live = il < inner;
  const int64_t i = live ? il : inner - 1;                  // a tail lane repeats the row's last point
  const int64_t n0 = (slice * nrun / nsplit) * RMV_RUN;
  int64_t n1 = ((slice + 1) * nrun / nsplit) * RMV_RUN;
  if (n1 > B) n1 = B;
  const T ui = reinterpret_cast<const T*>(g.g[d - 1])[i];
  const T* cp[NC];
#pragma unroll
  for (int s = 0; s < NC; ++s) cp[s] = c + (int64_t)(s < ncv ? s : ncv - 1) * B;
  double acc[NC];
#pragma unroll
  for (int s = 0; s < NC; ++s) acc[s] = 0;

  if (MODE == 1) {
    const bool sq = scaled_dist(kind);
    const T uoff = semi_mc_offset<T>(u, npts);
    for (int64_t n = n0; n < n1; ++n) {                       // the same trip count for every lane
      __syncthreads();                                        // the last observation's readers are done
      for (int a = threadIdx.x; a < npts; a += RMV_TILE) {
        const T al = semi_mc_alpha<T>(a, npts, uoff);
        so_s[a] = semi_mc_outer<T>(d, [&](int ax) -> T {
          const int64_t ia = d == 2 ? o : (ax == 0 ? o / g.m[1] : o % g.m[1]);
          return semi_mc_sqd<T>(reinterpret_cast<const T*>(g.g[ax])[ia], x[n * d + ax], al, sq, ell);
        });
        xl_s[a] = x[n * d + d - 1] * al;
      }
      __syncthreads();
      const T dist = semi_dist<T>(x, n, d);
      const T kv = semi_mc_elem<T>(kind, d, ui, npts, sq, sig2, ell, kp, dist, [&](int a, T& xl, T& so) {
        xl = xl_s[a];
        so = so_s[a];
      });
#pragma unroll
      for (int s = 0; s < NC; ++s) acc[s] += (double)(kv * cp[s][n]);
    }
  } else {
    // This branch keeps its own spelling of the analytic form.  Here the product (ui sinv) ui feeds
    // both arms of the d == 1 choice, so hipcc leaves c = co + (ui sinv) ui as a product and a sum,
    // where semi_sq_elem fuses them: from two axes on the bits would differ in c's last place.
    const T sinv = (T)1 / (ell * ell);
    const T sqrt2 = (T)1.4142135623730950488, sqrt2pi = (T)2.5066282746310005024;
    int64_t oi[2] = {0, 0};
    if (d == 2) oi[0] = o;
    if (d == 3) { oi[0] = o / g.m[1]; oi[1] = o % g.m[1]; }
    T ua[2] = {0, 0};
    for (int ax = 0; ax < d - 1; ++ax) ua[ax] = reinterpret_cast<const T*>(g.g[ax])[oi[ax]];
    for (int64_t n = n0; n < n1; ++n) {
      T xs[3];
      T av = 0, xn2 = 0;
      for (int ax = 0; ax < d; ++ax) {
        const T xv = x[n * d + ax];
        xs[ax] = xv * sinv;
        av += xs[ax] * xv;
        xn2 += xv * xv;
      }
      T bo = 0, co = 0;                                       // outer-axis terms of b and c, in axis order
      for (int ax = 0; ax < d - 1; ++ax) {
        bo += xs[ax] * ua[ax];
        co += (ua[ax] * sinv) * ua[ax];
      }
      const T dist = sqrt(xn2);
      const T scale = sqrt((T)1 / av);
      const T b = (d == 1) ? xs[0] * ui : bo + xs[d - 1] * ui;
      const T cc = (d == 1) ? (ui * sinv) * ui : co + (ui * sinv) * ui;
      const T loc = b / av;
      const T coef = sig2 * exp((b * b) / ((T)2 * av) - cc / (T)2) * sqrt2pi * scale;
      const T ca = (T)0.5 * ((T)1 + erf(((T)1 - loc) / (scale * sqrt2)));
      const T cb = (T)0.5 * ((T)1 + erf(((T)0 - loc) / (scale * sqrt2)));
      const T kv = coef * (ca - cb) * dist;
#pragma unroll
      for (int s = 0; s < NC; ++s) acc[s] += (double)(kv * cp[s][n]);
    }
  }
  if (!live) return;
  const int64_t j = o * inner + i;
  if (part != nullptr) {
    double* p = part + slice * NC * M + j;
#pragma unroll
    for (int s = 0; s < NC; ++s) p[(int64_t)s * M] = acc[s];
  } else {
#pragma unroll
    for (int s = 0; s < NC; ++s)
      if (s < ncv) out[(int64_t)s * M + j] = (T)acc[s];
  }
}

// nobs >= 0, nc > 0, nsplit >= 0
template <typename T>
static hipError_t kuf_rmatvec_t(const KufObs& o, const void* cv, int64_t nc, int64_t nsplit_in, void* outv) {
  const int mode = o.mode;
  const int64_t nobs = o.nobs;
  hipStream_t s = o.stream;
  KufGrid g{};
  int64_t M, outer;
  kuf_fill_grid(g, o.ndim, o.m, o.grids, &M, &outer);
  T* out = reinterpret_cast<T*>(outv);
  if (nobs == 0) return hipMemsetAsync(out, 0, (size_t)nc * (size_t)M * sizeof(T), s);   // an empty sum
  const T* x = reinterpret_cast<const T*>(o.x);
  const T* c = reinterpret_cast<const T*>(cv);
  const T* u = reinterpret_cast<const T*>(o.u);
  // the split: a pure function of (nobs, M) and the CU count unless the caller forces it; one
  // slice whenever the mesh alone gives the blocks that fill the device
  const int64_t nchunk = (o.m[o.ndim - 1] + RMV_TILE - 1) / RMV_TILE;
  const int64_t ntile = mode == 0 ? (M + RMV_TILE - 1) / RMV_TILE : outer * nchunk;   // blocks per slice
  const int64_t nrun = (nobs + RMV_RUN - 1) / RMV_RUN;
  int64_t nsplit = nsplit_in;
  if (nsplit == 0) {
    hipError_t e = hipSuccess;
    const int64_t target = (int64_t)16 * kuf_cus(&e);        // one-wave blocks that fill the device
    if (e != hipSuccess) return e;
    nsplit = ntile >= target ? 1 : (target + ntile - 1) / ntile;
  }
  if (nsplit > nrun) nsplit = nrun;
  if (ntile * nsplit > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const unsigned nb = (unsigned)(ntile * nsplit);
  return kuf_row_groups(
      nc, nsplit > 1 ? (size_t)nsplit * (size_t)M : 0, s,
      [&](int64_t s0, int NC, int ncv, double* part) {
        const T* cg = c + s0 * nobs;
        T* og = out + s0 * M;
        kuf_with_width(NC, [&](auto W) {
          if (mode == 0)
            kuf_with_kind(o.kind, [&](auto K) {
              hipLaunchKernelGGL((k_kuf_grid_rmv<T, decltype(K)::value, decltype(W)::value>), dim3(nb), dim3(RMV_TILE),
                                 0, s, g, x, nobs, (T)o.sig2, kuf_vec<T>(o.ell), cg, ncv, M, (int)nsplit, nrun, part,
                                 og);
            });
          else
            kuf_with_mode(mode, [&](auto MD) {
              hipLaunchKernelGGL((k_kuf_semi_rmv<T, decltype(MD)::value, decltype(W)::value>), dim3(nb),
                                 dim3(RMV_TILE), 0, s, g, x, nobs, o.kind, (T)o.sig2, (T)o.ell[0], (T)o.kp, o.npts, u, cg,
                                 ncv, M, (int)nsplit, nrun, nchunk, part, og);
            });
        });
      },
      [&](int64_t s0, int NC, int ncv, double* part) {
        const int64_t tot = M * ncv;
        hipLaunchKernelGGL((k_kuf_rmv_finish<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, part,
                           (int)nsplit, M, NC, ncv, out + s0 * M);
      });
}

// launcher behind hgp_kuf_grid_rmatvec(_ard) / hgp_kuf_semi_mc_rmatvec / hgp_kuf_semi_sqexp_rmatvec
hipError_t kuf_rmatvec(const KufObs& o, const void* c, int64_t nc, int64_t nsplit, void* out) {
  return kuf_with_dtype(o.dtype, [&](auto t) { return kuf_rmatvec_t<decltype(t)>(o, c, nc, nsplit, out); });
}

}  // namespace hgp
