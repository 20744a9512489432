// hgp_kuf_win.hip — the two products with the point-observation cross covariances restricted to a
// WINDOW of pairs, for kernels that are far shorter than the grid:
//   matvec   out[n, s] = sum_{j in window(n)} k(x_n, u_j) w[s, j]      (k_kuf_win_mv)
//   rmatvec  out[s, j] = sum_{n: (n, j) in window} c[s, n] k(x_n, u_j)  (k_kuf_win_rmv)
// The dense twins (hgp_kuf_mv.hip, hgp_kuf_rmv.hip) evaluate all nobs * M kernel values; these
// evaluate the pairs of the window alone.
//
// The window.  Pair (n, j) belongs to it iff fabs(x[n][a] - g_a[j_a]) <= rho[a] on every axis a, in
// the tensor dtype, each rho[a] rounded once to that dtype (win_in).  A box, not a ball: with rho the
// distance from which k(r) <= tol sig2 on, every dropped pair is farther than rho and its value
// under tol sig2.  A SqExp with one length scale per axis has one radius per axis, rho[a] the
// distance from which axis a's factor alone is <= tol: a dropped pair has such an axis and the other
// factors are <= 1.  The scalar entries put their one radius on every axis.  The rounded difference x - g_a[i] does not increase with i on a strictly
// increasing axis, so per axis the box is an index range [lo, hi) and two binary searches with
// the predicate's own comparisons find exactly the set the predicate describes (win_first).  The
// matvec finds the ranges that way, the rmatvec applies the predicate pair by pair: one set, so
// the two products are exact transposes.  The element value is formed in one way in both
// (kuf_axis, kuf_outer, one fused multiply-add for the last axis: hgp_kuf_eval.hpp), so it has the
// same bits in both.
//
// k_kuf_win_mv: one wave per point, four points a block, no LDS and no barrier.  Lanes 0 .. 2d-1
// run the 2d searches side by side and the wave reads their results.  The wave then walks the
// outer rows of the box with the outer squared distance hoisted, lanes across the last-axis range
// (the w loads of a row are one contiguous run).  A lane adds its products of a row in the tensor
// dtype, the rows in fp64; the lanes are added by the fixed xor butterfly.  Weight rows in groups
// of 8, 4 or 1 as the dense kernel.  No atomics.
//
// k_kuf_win_rmv: a gather.  A block owns a tile of mesh points (KufTile, hgp_kuf_tile.hpp), one
// per thread.  The observations come sorted by BIN: per axis the cell of x is the number of nodes
// <= x (0 .. m), its bin is cell / tile, bins are numbered in C order (kuf_win_bins).
// Only x in [g[first] - rho, g[last] + rho] can reach a tile on an axis; the block finds the cells of
// those two ends (the interval widened by 1e-6 rho and 1e-15 |g|, far more than the predicate's
// rounding, in fp64) and visits the bins between.  The bins of one last-axis row are neighbours in
// the sorted list, so a row is one contiguous range of `order`; it is staged in LDS in chunks of
// 256 observations (coordinates and coefficients), and every thread applies the predicate and
// kern_eval to every staged observation.  A thread adds its products of a chunk in the tensor
// dtype, the chunks in fp64, in the order of the list: the result is a function of the arguments
// alone.  No atomics.  An order[k] outside [0, nobs) is staged as NaN coordinates (never in a
// window); a range of bin_start outside 0 <= s0 <= s1 <= nobs is skipped.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <limits>

#include "hgp_kuf_eval.hpp"
#include "hgp_kuf_launch.hpp"
#include "hgp_kuf_tile.hpp"

namespace hgp {

constexpr int WIN_THREADS = KUF_TILE_THREADS;   // block of both kernels: 4 points (mv), one tile of mesh points (rmv)
constexpr int WIN_CHUNK = 256;     // observations staged at once (rmv); the longest run summed in dtype

// the window's predicate on one axis
template <typename T>
__device__ __forceinline__ bool win_in(T x, T u, T rho) {
  return fabs(x - u) <= rho;
}

// first i in [0, m] with x - g[i] <= rho (upper = false: the window's lo) or with x - g[i] < -rho
// (upper = true: its hi).  NaN x: m for both, an empty range.
template <typename T>
__device__ __forceinline__ int64_t win_first(const T* __restrict__ g, int64_t m, T x, T rho, bool upper) {
  int64_t a = 0, b = m;
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    const T dv = x - g[mid];
    if (upper ? dv < -rho : dv <= rho)
      b = mid;
    else
      a = mid + 1;
  }
  return a;
}

template <typename T, int KIND, int NW>
__global__ __launch_bounds__(WIN_THREADS) void k_kuf_win_mv(KufGrid g, const T* __restrict__ x, int64_t B, T sig2,
                                                           KufVec<T> ell, KufVec<T> rho, const T* __restrict__ w,
                                                           int nwv, int64_t M, T* __restrict__ out, int64_t ldo) {
  const int d = g.d;
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * (WIN_THREADS / 64) + (threadIdx.x >> 6);
  if (n >= B) return;                                         // the whole wave: no barrier below
  const T x0 = x[n * d];
  const T x1 = d > 1 ? x[n * d + 1] : (T)0;
  const T x2 = d > 2 ? x[n * d + 2] : (T)0;
  const T* g0 = reinterpret_cast<const T*>(g.g[0]);
  const T* g1 = reinterpret_cast<const T*>(g.g[d > 1 ? 1 : 0]);
  const T* g2 = reinterpret_cast<const T*>(g.g[d > 2 ? 2 : 0]);
  const int64_t m0 = g.m[0], m1 = d > 1 ? g.m[1] : 1, m2 = d > 2 ? g.m[2] : 1;
  // lane q < 2 d: the search of axis q / 2, its lo (q even) or hi (q odd); the others repeat lane 0's
  const int q = lane < 2 * d ? lane : 0;
  const int qa = q >> 1;
  const long long r = win_first<T>(qa == 0 ? g0 : (qa == 1 ? g1 : g2), qa == 0 ? m0 : (qa == 1 ? m1 : m2),
                                   qa == 0 ? x0 : (qa == 1 ? x1 : x2), kuf_at(rho, qa), (q & 1) != 0);
  const int64_t lo0 = __shfl(r, 0, 64), hi0 = __shfl(r, 1, 64);
  const int64_t lo1 = d > 1 ? __shfl(r, 2, 64) : 0, hi1 = d > 1 ? __shfl(r, 3, 64) : 0;
  const int64_t lo2 = d > 2 ? __shfl(r, 4, 64) : 0, hi2 = d > 2 ? __shfl(r, 5, 64) : 0;
  // the last axis (lanes) and up to two outer ones (rows); an absent outer axis is one row
  const T xl = d == 1 ? x0 : (d == 2 ? x1 : x2);
  const T ell_l = kuf_last(ell, d);
  const T* gl = d == 1 ? g0 : (d == 2 ? g1 : g2);
  const int64_t inner = d == 1 ? m0 : (d == 2 ? m1 : m2);
  const int64_t loL = d == 1 ? lo0 : (d == 2 ? lo1 : lo2), hiL = d == 1 ? hi0 : (d == 2 ? hi1 : hi2);
  const int64_t a0 = d >= 2 ? lo0 : 0, b0 = d >= 2 ? hi0 : 1;
  const int64_t a1 = d == 3 ? lo1 : 0, b1 = d == 3 ? hi1 : 1;
  const T* wp[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) wp[s] = w + (int64_t)(s < nwv ? s : nwv - 1) * M;
  double acc[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) acc[s] = 0;
  for (int64_t o0 = a0; o0 < b0; ++o0) {
    const T d0 = d >= 2 ? kuf_axis<T, KIND>(x0, g0[o0], ell.v[0]) : (T)0;
    for (int64_t o1 = a1; o1 < b1; ++o1) {
      const T d1 = d == 3 ? kuf_axis<T, KIND>(x1, g1[o1], ell.v[1]) : (T)0;
      const T so = kuf_outer<T>(d, d0, d1);
      const int64_t base = (d == 3 ? o0 * m1 + o1 : (d == 2 ? o0 : 0)) * inner;
      T run[NW];
#pragma unroll
      for (int s = 0; s < NW; ++s) run[s] = 0;
      for (int64_t i = loL + lane; i < hiL; i += 64) {
        const T dv = kuf_axis<T, KIND>(xl, gl[i], ell_l);
        const T kv = kern_eval<T>(KIND, kuf_fma(dv, dv, so), sig2, ell.v[0]);
#pragma unroll
        for (int s = 0; s < NW; ++s) run[s] += kv * wp[s][base + i];
      }
#pragma unroll
      for (int s = 0; s < NW; ++s) acc[s] += (double)run[s];
    }
  }
#pragma unroll
  for (int s = 0; s < NW; ++s)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[s] += __shfl_xor(acc[s], off, 64);
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < NW; ++s)
      if (s < nwv) out[n * ldo + s] = (T)acc[s];
  }
}

// number of nodes of the axis with g[i] <= v, in fp64: the cell of v
template <typename T>
__device__ __forceinline__ int64_t win_cell(const T* __restrict__ g, int64_t m, double v) {
  int64_t a = 0, b = m;
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if ((double)g[mid] <= v)
      a = mid + 1;
    else
      b = mid;
  }
  return a;
}

template <typename T, int KIND, int NC, int D>
__global__ __launch_bounds__(WIN_THREADS) void k_kuf_win_rmv(KufGrid g, const T* __restrict__ x, int64_t B, T sig2,
                                                            KufVec<T> ell, KufVec<T> rho, const T* __restrict__ c,
                                                            int ncv, int64_t M, const int64_t* __restrict__ order,
                                                            const int64_t* __restrict__ bin_start,
                                                            T* __restrict__ out) {
  __shared__ T xs[D][WIN_CHUNK];
  __shared__ T cs[NC][WIN_CHUNK];
  __shared__ int64_t cell_s[2 * D];
  constexpr int T0 = KufTile<D>::T0, T1 = KufTile<D>::T1, T2 = KufTile<D>::T2;
  const int tid = threadIdx.x;
  // the block's tile and the thread's mesh point in it
  const KufTilePos tp = kuf_tile_pos<D>(g);
  const int64_t m0 = tp.m0, m1 = tp.m1, m2 = tp.m2, i0 = tp.i0, i1 = tp.i1, i2 = tp.i2;
  const bool live = tp.live;
  const T* g0 = reinterpret_cast<const T*>(g.g[0]);
  const T* g1 = reinterpret_cast<const T*>(g.g[D > 1 ? 1 : 0]);
  const T* g2 = reinterpret_cast<const T*>(g.g[D > 2 ? 2 : 0]);
  const T u0 = g0[i0 < m0 ? i0 : m0 - 1];
  const T u1 = D > 1 ? g1[i1 < m1 ? i1 : m1 - 1] : (T)0;
  const T u2 = D > 2 ? g2[i2 < m2 ? i2 : m2 - 1] : (T)0;
  // the cells that can reach the tile on each axis: thread q < 2 D finds one end
  if (tid < 2 * D) {
    const int a = tid >> 1;
    const T* ga = a == 0 ? g0 : (a == 1 ? g1 : g2);
    const int64_t ma = a == 0 ? m0 : (a == 1 ? m1 : m2);
    const int64_t first = a == 0 ? tp.t0 * T0 : (a == 1 ? tp.t1 * T1 : tp.t2 * T2);
    int64_t last = first + (a == 0 ? T0 : (a == 1 ? T1 : T2)) - 1;
    if (last > ma - 1) last = ma - 1;
    const double rw = (double)kuf_at(rho, a) * (1.0 + 1e-6);
    const double ge = (double)ga[(tid & 1) ? last : first];
    const double slack = 1e-15 * fabs(ge);
    cell_s[tid] = win_cell<T>(ga, ma, (tid & 1) ? ge + rw + slack : ge - rw - slack);
  }
  __syncthreads();
  const int64_t nb1 = m1 / T1 + 1, nb2 = m2 / T2 + 1;        // bins of axes 1, 2 (read only where the axis exists)
  const int64_t bl0 = cell_s[0] / T0, bh0 = cell_s[1] / T0;
  const int64_t bl1 = D > 1 ? cell_s[D > 1 ? 2 : 0] / T1 : 0, bh1 = D > 1 ? cell_s[D > 1 ? 3 : 0] / T1 : 0;
  const int64_t bl2 = D > 2 ? cell_s[D > 2 ? 4 : 0] / T2 : 0, bh2 = D > 2 ? cell_s[D > 2 ? 5 : 0] / T2 : 0;
  // rows of bins: the last axis' bins of a row are one contiguous range of the sorted list
  const int64_t ra0 = D >= 2 ? bl0 : 0, rb0 = D >= 2 ? bh0 : 0;
  const int64_t ra1 = D == 3 ? bl1 : 0, rb1 = D == 3 ? bh1 : 0;
  const int64_t rowlen = D == 1 ? m0 / T0 + 1 : (D == 2 ? nb1 : nb2);
  const int64_t cl = D == 1 ? bl0 : (D == 2 ? bl1 : bl2), ch = D == 1 ? bh0 : (D == 2 ? bh1 : bh2);
  // the thread's last-axis coordinate and the two outer ones, as the matvec names them
  const T ul = D == 1 ? u0 : (D == 2 ? u1 : u2);
  double acc[NC];
#pragma unroll
  for (int s = 0; s < NC; ++s) acc[s] = 0;
  for (int64_t r0 = ra0; r0 <= rb0; ++r0) {
    for (int64_t r1 = ra1; r1 <= rb1; ++r1) {
      const int64_t row = (D == 3 ? r0 * nb1 + r1 : (D == 2 ? r0 : 0)) * rowlen;
      const int64_t s0 = bin_start[row + cl], s1 = bin_start[row + ch + 1];
      if (!(s0 >= 0 && s0 <= s1 && s1 <= B)) continue;        // the same for every thread of the block
      for (int64_t k0 = s0; k0 < s1; k0 += WIN_CHUNK) {
        const int cnt = (int)(s1 - k0 < WIN_CHUNK ? s1 - k0 : WIN_CHUNK);
        __syncthreads();                                      // the last chunk's readers are done
        if (tid < cnt) {
          const int64_t n = order[k0 + tid];
          const bool ok = n >= 0 && n < B;
          const T nan = std::numeric_limits<T>::quiet_NaN();
#pragma unroll
          for (int a = 0; a < D; ++a) xs[a][tid] = ok ? x[n * D + a] : nan;
#pragma unroll
          for (int s = 0; s < NC; ++s) cs[s][tid] = ok ? c[(int64_t)(s < ncv ? s : ncv - 1) * B + n] : (T)0;
        }
        __syncthreads();
        if (live) {
          T run[NC];
#pragma unroll
          for (int s = 0; s < NC; ++s) run[s] = 0;
          for (int k = 0; k < cnt; ++k) {
            const T p0 = xs[0][k];
            const T p1 = D > 1 ? xs[D > 1 ? 1 : 0][k] : (T)0;
            const T p2 = D > 2 ? xs[D > 2 ? 2 : 0][k] : (T)0;
            bool in = win_in<T>(p0, u0, rho.v[0]);
            if (D > 1) in = in && win_in<T>(p1, u1, rho.v[1]);
            if (D > 2) in = in && win_in<T>(p2, u2, rho.v[2]);
            if (in) {
              const T d0 = D >= 2 ? kuf_axis<T, KIND>(p0, u0, ell.v[0]) : (T)0;
              const T d1 = D == 3 ? kuf_axis<T, KIND>(p1, u1, ell.v[1]) : (T)0;
              const T dv = kuf_axis<T, KIND>(D == 1 ? p0 : (D == 2 ? p1 : p2), ul, ell.v[D - 1]);
              const T kv = kern_eval<T>(KIND, kuf_sqdist<T>(D, d0, d1, dv), sig2, ell.v[0]);
#pragma unroll
              for (int s = 0; s < NC; ++s) run[s] += kv * cs[s][k];
            }
          }
#pragma unroll
          for (int s = 0; s < NC; ++s) acc[s] += (double)run[s];
        }
      }
    }
  }
  if (!live) return;
  const int64_t j = tp.flat<D>();
#pragma unroll
  for (int s = 0; s < NC; ++s)
    if (s < ncv) out[(int64_t)s * M + j] = (T)acc[s];
}

// nobs > 0, nw > 0
template <typename T>
static hipError_t kuf_matvec_win_t(const KufObs& o, const void* wv, int64_t nw, void* outv) {
  const int64_t nobs = o.nobs;
  hipStream_t s = o.stream;
  KufGrid g{};
  int64_t M;
  kuf_fill_grid(g, o.ndim, o.m, o.grids, &M);
  const T* x = reinterpret_cast<const T*>(o.x);
  const T* w = reinterpret_cast<const T*>(wv);
  T* out = reinterpret_cast<T*>(outv);
  const int64_t per = WIN_THREADS / 64;
  const int64_t nblk = (nobs + per - 1) / per;
  if (nblk > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const unsigned nb = (unsigned)nblk;
  return kuf_row_groups(nw, s, [&](int64_t s0, int NW, int nwv, double*) {
    kuf_with_kind(o.kind, [&](auto K) {
      kuf_with_width(NW, [&](auto W) {
        hipLaunchKernelGGL((k_kuf_win_mv<T, decltype(K)::value, decltype(W)::value>), dim3(nb), dim3(WIN_THREADS), 0,
                           s, g, x, nobs, (T)o.sig2, kuf_vec<T>(o.ell), kuf_vec<T>(o.rho), w + s0 * M, nwv, M,
                           out + s0, nw);
      });
    });
  });
}

// nobs >= 0 (0: out zeroed), nc > 0
template <typename T>
static hipError_t kuf_rmatvec_win_t(const KufObs& o, const void* cv, int64_t nc, const int64_t* order,
                                    const int64_t* bin_start, void* outv) {
  const int64_t nobs = o.nobs;
  hipStream_t s = o.stream;
  KufGrid g{};
  int64_t M;
  kuf_fill_grid(g, o.ndim, o.m, o.grids, &M);
  T* out = reinterpret_cast<T*>(outv);
  if (nobs == 0) return hipMemsetAsync(out, 0, (size_t)nc * (size_t)M * sizeof(T), s);   // an empty sum
  const T* x = reinterpret_cast<const T*>(o.x);
  const T* c = reinterpret_cast<const T*>(cv);
  const int64_t ntile = kuf_tile_count(o.ndim, o.m);
  if (ntile > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const unsigned nb = (unsigned)ntile;
  return kuf_row_groups(nc, s, [&](int64_t s0, int NC, int ncv, double*) {
    kuf_with_kind(o.kind, [&](auto K) {
      kuf_with_dim(o.ndim, [&](auto D) {
        kuf_with_width(NC, [&](auto W) {
          hipLaunchKernelGGL((k_kuf_win_rmv<T, decltype(K)::value, decltype(W)::value, decltype(D)::value>), dim3(nb),
                             dim3(WIN_THREADS), 0, s, g, x, nobs, (T)o.sig2, kuf_vec<T>(o.ell), kuf_vec<T>(o.rho),
                             c + s0 * nobs, ncv, M, order, bin_start, out + s0 * M);
        });
      });
    });
  });
}

// launchers behind hgp_kuf_grid_matvec_win(_ard) and hgp_kuf_grid_rmatvec_win(_ard)
hipError_t kuf_matvec_win(const KufObs& o, const void* w, int64_t nw, void* out) {
  return kuf_with_dtype(o.dtype, [&](auto t) { return kuf_matvec_win_t<decltype(t)>(o, w, nw, out); });
}

hipError_t kuf_rmatvec_win(const KufObs& o, const void* c, int64_t nc, const int64_t* order,
                           const int64_t* bin_start, void* out) {
  return kuf_with_dtype(o.dtype,
                        [&](auto t) { return kuf_rmatvec_win_t<decltype(t)>(o, c, nc, order, bin_start, out); });
}

// the geometry behind hgp_kuf_win_bins: tile[a] mesh points of a tile along axis a, nbins[a] =
// m[a] / tile[a] + 1 bins of tile[a] cells (cells 0 .. m[a]); axes >= ndim: 1 and 1
void kuf_win_geometry(int ndim, const int64_t* m, int64_t* tile, int64_t* nbins) {
  for (int a = 0; a < 3; ++a) {
    tile[a] = a < ndim ? kuf_tile(ndim, a) : 1;
    nbins[a] = a < ndim ? m[a] / tile[a] + 1 : 1;
  }
}

}  // namespace hgp
