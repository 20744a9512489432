// hgp_kuf_mv.hip — products with the grid cross covariances without storing them:
//   out[n, s] = sum_j Kuf[n, j] w[s, j],   Kuf (nobs, M) as hgp_kuf.hip writes it, w (nw, M) rows.
// With w = K^-1 R qm this is the posterior mean at nobs points from ONE solve (the reference
// solves once per point: hipgp.py:416-446 through svi_gp.py:72 and hipgp.py:117-146); with
// several weight rows, joint draws of the projected process.  The element values come from the
// same device functions as the forwards (hgp_kuf_eval.hpp; line integrals: hgp_kuf_semi.hpp), the
// host scaffold (CU count, row groups, partials, the kind / width ladders) from hgp_kuf_launch.hpp.
//
// Point observations (k_kuf_grid_mv), the hot path: compute bound, nobs * M kernel values each
// used nw times.  A block is ONE wave and owns a tile of 64 points, one per lane: the lane's
// coordinates and up to 8 accumulators sit in registers.  The block sweeps a slice of the grid
// in mesh order; everything indexed by the grid point (its coordinates, the w values) is the
// same for all lanes, so those loads are wave-uniform (scalar loads, no LDS), and the outer
// axes' squared distances are hoisted out of the last-axis loop.  One kernel evaluation feeds
// NW fused multiply-adds.  nw > 8 runs in groups of weight rows (8, 4 or 1 wide; a group's
// unused slots repeat its last row and are not written).
//
// Summation: products are added in the tensor dtype over runs of at most MV_RUN consecutive
// points of the last axis, the runs in fp64 in mesh order.  Few points: the grid is cut into
// nsplit slices of whole MV_UNIT-point units, partial sums part[slice][n][slot] (fp64) are
// added in slice order by k_kuf_mv_finish.  No atomics: equal arguments give equal bits.
//
// Line-integral observations (k_kuf_semi_mv) keep the forwards' structure: a block owns one
// observation and a range of outer indices, threads stride the last axis, the per-thread fp64
// sums go through a fixed-order block reduction.  Slices are ranges of outer indices.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hgp_kuf_eval.hpp"
#include "hgp_kuf_launch.hpp"
#include "hgp_kuf_semi.hpp"

namespace hgp {

constexpr int MV_TILE = 64;       // points per block of the point kernel (one wave)
constexpr int MV_UNIT = 64;       // grid points per unit of the split
constexpr int MV_RUN = 256;       // longest run summed in the tensor dtype
constexpr int MV_THREADS = SEMI_THREADS;   // block of the line-integral kernels
constexpr int MV_MIN_UNITS = 4;   // nsplit = 0 leaves a slice at least this many units

template <typename T, int KIND, int NW>
__global__ __launch_bounds__(MV_TILE) void k_kuf_grid_mv(KufGrid g, const T* __restrict__ x, int64_t B, T sig2,
                                                        KufVec<T> ell,
                                                        const T* __restrict__ w, int nwv, int64_t M, int nsplit,
                                                        int64_t nunit, double* __restrict__ part,
                                                        T* __restrict__ out, int64_t ldo) {
  const int d = g.d;
  const int64_t inner = g.m[d - 1];
  const int64_t slice = (int64_t)blockIdx.x % nsplit;
  const int64_t tile = (int64_t)blockIdx.x / nsplit;
  const int64_t nl = tile * MV_TILE + threadIdx.x;
  const bool live = nl < B;
  const int64_t n = live ? nl : B - 1;                      // a tail lane repeats the last point
  const int64_t j0 = (slice * nunit / nsplit) * MV_UNIT;
  int64_t j1 = ((slice + 1) * nunit / nsplit) * MV_UNIT;
  if (j1 > M) j1 = M;
  constexpr bool sq = KIND == HGP_KERN_SQEXP || KIND == HGP_KERN_GNEITING;
  T xv[3] = {0, 0, 0};
  for (int a = 0; a < d; ++a) xv[a] = x[n * d + a];
  const T xl = xv[d - 1];
  const T ell_l = kuf_last(ell, d);                          // the last axis' length scale
  const T* g0 = reinterpret_cast<const T*>(g.g[0]);
  const T* g1 = reinterpret_cast<const T*>(g.g[d > 1 ? 1 : 0]);
  const T* gl = reinterpret_cast<const T*>(g.g[d - 1]);
  const T* wp[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) wp[s] = w + (int64_t)(s < nwv ? s : nwv - 1) * M;
  double acc[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) acc[s] = 0;
  for (int64_t o = j0 / inner; o * inner < j1; ++o) {
    const int64_t base = o * inner;
    const int64_t ia = j0 > base ? j0 - base : 0;
    const int64_t ib = j1 - base < inner ? j1 - base : inner;
    // outer axes: summed in axis order, as k_kuf_grid
    T so = 0;
    if (d == 2) {
      T dv = xv[0] - g0[o];
      if (sq) dv = dv / ell.v[0];
      so = dv * dv;
    } else if (d == 3) {
      T dv = xv[0] - g0[o / g.m[1]];
      if (sq) dv = dv / ell.v[0];
      T dw = xv[1] - g1[o % g.m[1]];
      if (sq) dw = dw / ell.v[1];
      so = dv * dv + dw * dw;
    }
    for (int64_t i0 = ia; i0 < ib; i0 += MV_RUN) {
      const int64_t i1 = i0 + MV_RUN < ib ? i0 + MV_RUN : ib;
      T run[NW];
#pragma unroll
      for (int s = 0; s < NW; ++s) run[s] = 0;
#pragma unroll 4
      for (int64_t i = i0; i < i1; ++i) {
        T dv = xl - gl[i];
        if (sq) dv = dv / ell_l;
        const T sv = so + dv * dv;                           // d = 1: so = 0, the same bits as dv * dv
        const T kv = kern_eval<T>(KIND, sv, sig2, ell.v[0]);
#pragma unroll
        for (int s = 0; s < NW; ++s) run[s] += kv * wp[s][base + i];
      }
#pragma unroll
      for (int s = 0; s < NW; ++s) acc[s] += (double)run[s];
    }
  }
  if (!live) return;
  if (part != nullptr) {
    double* p = part + (slice * B + n) * NW;
#pragma unroll
    for (int s = 0; s < NW; ++s) p[s] = acc[s];
  } else {
#pragma unroll
    for (int s = 0; s < NW; ++s)
      if (s < nwv) out[n * ldo + s] = (T)acc[s];
  }
}

// MODE 1: the Monte-Carlo line integral of k_kuf_semi_mc; MODE 2: the analytic SqExp one of
// k_kuf_semi_sqexp.  Block (n, slice of outer indices); element values formed as the forwards do.
template <typename T, int MODE, int NW>
__global__ __launch_bounds__(MV_THREADS) void k_kuf_semi_mv(KufGrid g, const T* __restrict__ x, int64_t B, int kind,
                                                           T sig2, T ell, T kp, int npts, const T* __restrict__ u,
                                                           const T* __restrict__ w, int nwv, int64_t M, int nsplit,
                                                           double* __restrict__ part, T* __restrict__ out,
                                                           int64_t ldo) {
  __shared__ T so_s[MODE == 1 ? SEMI_MAX_NPTS : 1];
  __shared__ T xl_s[MODE == 1 ? SEMI_MAX_NPTS : 1];
  const int d = g.d;
  const int64_t inner = g.m[d - 1];
  int64_t outer = 1;
  for (int a = 0; a < d - 1; ++a) outer *= g.m[a];
  const int64_t slice = (int64_t)blockIdx.x % nsplit;
  const int64_t n = (int64_t)blockIdx.x / nsplit;           // < B: the grid is B * nsplit blocks
  const int64_t o0 = slice * outer / nsplit, o1 = (slice + 1) * outer / nsplit;
  const T* gl = reinterpret_cast<const T*>(g.g[d - 1]);
  const T* wp[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) wp[s] = w + (int64_t)(s < nwv ? s : nwv - 1) * M;
  double acc[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) acc[s] = 0;
  const T dist = semi_dist<T>(x, n, d);

  if (MODE == 1) {
    const bool sq = scaled_dist(kind);
    const T uoff = semi_mc_offset<T>(u, npts);
    for (int64_t o = o0; o < o1; ++o) {                       // the same trip count for every thread
      __syncthreads();                                        // the last row's readers are done
      for (int a = threadIdx.x; a < npts; a += MV_THREADS) {
        const T al = semi_mc_alpha<T>(a, npts, uoff);
        so_s[a] = semi_mc_outer<T>(d, [&](int ax) -> T {
          const int64_t ia = d == 2 ? o : (ax == 0 ? o / g.m[1] : o % g.m[1]);
          return semi_mc_sqd<T>(reinterpret_cast<const T*>(g.g[ax])[ia], x[n * d + ax], al, sq, ell);
        });
        xl_s[a] = x[n * d + d - 1] * al;
      }
      __syncthreads();
      for (int64_t i = threadIdx.x; i < inner; i += MV_THREADS) {
        const T kv = semi_mc_elem<T>(kind, d, gl[i], npts, sq, sig2, ell, kp, dist, [&](int a, T& xl, T& so) {
          xl = xl_s[a];
          so = so_s[a];
        });
#pragma unroll
        for (int s = 0; s < NW; ++s) acc[s] += (double)(kv * wp[s][o * inner + i]);
      }
    }
  } else {
    const T sinv = (T)1 / (ell * ell);
    T xs[3];
    const T av = semi_sq_line<T>(x, n, d, sinv, xs);
    const T scale = sqrt((T)1 / av);
    for (int64_t o = o0; o < o1; ++o) {
      int64_t oi[2] = {0, 0};
      if (d == 2) oi[0] = o;
      if (d == 3) { oi[0] = o / g.m[1]; oi[1] = o % g.m[1]; }
      T bo, co;
      semi_sq_outer<T>(d, xs, sinv, [&](int ax) -> T { return reinterpret_cast<const T*>(g.g[ax])[oi[ax]]; }, bo, co);
      for (int64_t i = threadIdx.x; i < inner; i += MV_THREADS) {
        const T kv = semi_sq_elem<T>(d, bo, co, xs[d - 1], gl[i], sinv, av, scale, sig2, dist);
#pragma unroll
        for (int s = 0; s < NW; ++s) acc[s] += (double)(kv * wp[s][o * inner + i]);
      }
    }
  }
  if (part != nullptr) {
    semi_block_sum<NW>(acc, part + (slice * B + n) * NW, NW);
  } else {
    __shared__ double row[NW];
    semi_block_sum<NW>(acc, row, nwv);
    __syncthreads();
    if ((int)threadIdx.x < nwv) out[n * ldo + threadIdx.x] = (T)row[threadIdx.x];
  }
}

// nobs > 0, nw > 0, nsplit >= 0
template <typename T>
static hipError_t kuf_matvec_t(const KufObs& o, const void* wv, int64_t nw, int64_t nsplit_in, void* outv) {
  const int mode = o.mode;
  const int64_t nobs = o.nobs;
  hipStream_t s = o.stream;
  KufGrid g{};
  int64_t M, outer;
  kuf_fill_grid(g, o.ndim, o.m, o.grids, &M, &outer);
  const T* x = reinterpret_cast<const T*>(o.x);
  const T* w = reinterpret_cast<const T*>(wv);
  const T* u = reinterpret_cast<const T*>(o.u);
  T* out = reinterpret_cast<T*>(outv);
  // the split: a pure function of (nobs, M, nw) and the CU count unless the caller forces it
  const int64_t nunit = mode == 0 ? (M + MV_UNIT - 1) / MV_UNIT : outer;
  const int64_t nrow = mode == 0 ? (nobs + MV_TILE - 1) / MV_TILE : nobs;      // blocks per slice
  int64_t nsplit = nsplit_in;
  if (nsplit == 0) {
    hipError_t e = hipSuccess;
    const int64_t target = (int64_t)(mode == 0 ? 16 : 4) * kuf_cus(&e);         // blocks that fill the device
    if (e != hipSuccess) return e;
    const int64_t most = mode == 0 ? nunit / MV_MIN_UNITS : nunit;
    nsplit = (target + nrow - 1) / nrow;
    if (nsplit > most) nsplit = most;
    if (nsplit < 1) nsplit = 1;
  }
  if (nsplit > nunit) nsplit = nunit;
  if (nrow * nsplit > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const unsigned nb = (unsigned)(nrow * nsplit);
  return kuf_row_groups(
      nw, nsplit > 1 ? (size_t)nsplit * (size_t)nobs : 0, s,
      [&](int64_t s0, int NW, int nwv, double* part) {
        const T* wg = w + s0 * M;
        T* og = out + s0;
        kuf_with_width(NW, [&](auto W) {
          if (mode == 0)
            kuf_with_kind(o.kind, [&](auto K) {
              hipLaunchKernelGGL((k_kuf_grid_mv<T, decltype(K)::value, decltype(W)::value>), dim3(nb), dim3(MV_TILE),
                                 0, s, g, x, nobs, (T)o.sig2, kuf_vec<T>(o.ell), wg, nwv, M, (int)nsplit, nunit, part,
                                 og, nw);
            });
          else
            kuf_with_mode(mode, [&](auto MD) {
              hipLaunchKernelGGL((k_kuf_semi_mv<T, decltype(MD)::value, decltype(W)::value>), dim3(nb),
                                 dim3(MV_THREADS), 0, s, g, x, nobs, o.kind, (T)o.sig2, (T)o.ell[0], (T)o.kp, o.npts, u,
                                 wg, nwv, M, (int)nsplit, part, og, nw);
            });
        });
      },
      [&](int64_t s0, int NW, int nwv, double* part) {
        const int64_t tot = nobs * NW;
        hipLaunchKernelGGL((k_kuf_mv_finish<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, part,
                           (int)nsplit, nobs, NW, nwv, out + s0, nw);
      });
}

// launcher behind hgp_kuf_grid_matvec(_ard) / hgp_kuf_semi_mc_matvec / hgp_kuf_semi_sqexp_matvec
hipError_t kuf_matvec(const KufObs& o, const void* w, int64_t nw, int64_t nsplit, void* out) {
  return kuf_with_dtype(o.dtype, [&](auto t) { return kuf_matvec_t<decltype(t)>(o, w, nw, nsplit, out); });
}

}  // namespace hgp
