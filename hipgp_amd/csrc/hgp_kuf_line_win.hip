// hgp_kuf_line_win.hip — the two products with the LINE-INTEGRAL cross covariances restricted to a
// window of pairs, for kernels that are far shorter than the grid:
//   matvec   out[n, s] = sum_{j in window(n)} Kuf[n, j] w[s, j]       (k_kuf_line_win_mv)
//   rmatvec  out[s, j] = sum_{n: (n, j) in window} c[s, n] Kuf[n, j]   (k_kuf_line_win_rmv)
// Kuf[n, j] = |x_n| int_0^1 k(u_j, a x_n) da, by the Monte-Carlo mean (MODE 1) or SqExp's closed
// form (MODE 2), the element that hgp_kuf_semi.hpp defines for the forwards and every product.
// The dense twins (k_kuf_semi_mv, k_kuf_semi_rmv) sweep the whole mesh for every line; a line only
// sees the nodes within the kernel's reach rho of its segment {a x_n : a in [0, 1]}.  The host
// scaffold is hgp_kuf_launch.hpp's.
//
// The window.  The segment is cut into P equal pieces, piece p from x (p / P) to x ((p + 1) / P)
// (lw_end; P = pieces[n] clamped to 1 .. 64, one number per line that both kernels read).  Pair
// (n, j) is in the window iff the node lies in the bounding box of SOME piece widened by rho on
// every axis: lo - u <= rho and u - hi <= rho, in the tensor dtype, contraction off (lw_near).
// Every point of the segment lies in a piece, so the window holds every node within Chebyshev
// distance rho of the segment: each dropped pair has k(u, a x) <= tol sig2 for all a.  A line with
// x = 0 has no window (its element is |x| times a mean: 0); NaN coordinates fail every comparison.
//
// One set in both kernels.  A piece is monotone on every axis and consecutive pieces share their
// end point bit for bit.  So (1) the pieces whose box admits a coordinate on one axis are a
// contiguous run of p, and so are those that admit several axes at once; (2) for one outer row
// the admitted pieces p_a .. p_b have last-axis boxes that chain, and their union is exactly
// { u : L - u <= rho and u - H <= rho } with L, H the smaller and larger of the run's two outer
// ends (rounded subtraction is monotone, so this holds in floating point too); (3) on a strictly
// increasing axis that set is an index range found by two binary searches with lw_near's own
// comparisons (lw_first).  The matvec walks rows and ranges that way, the rmatvec applies lw_in
// pair by pair: the same set, so the two products are exact transposes.
//
// k_kuf_line_win_mv: a block is ONE wave and owns (line, slice of the rows of the line's outer
// bounding range).  Lane p tests piece p against the row's outer coordinates, a ballot gives the
// run, the wave covers the last-axis range.  Per-lane fp64 sums, the xor butterfly, fp64 partials
// per slice added in slice order (k_kuf_mv_finish).  No atomics.
//
// k_kuf_line_win_rmv: a gather.  A block owns a tile of mesh points (KufTile, hgp_kuf_tile.hpp: the
// tiles of hgp_kuf_win_bins), one per thread, and walks ALL lines in chunks of 256: thread t tests
// line k0 + t against the tile's box (first the whole segment's box, then the pieces, keeping the run
// of pieces that can reach the tile), the survivors are compacted into LDS in line order by a wave
// ballot and a prefix over the waves, and every thread applies lw_in and the element function to
// every survivor.  Products are added in the tensor dtype over a chunk, the chunks in fp64, in
// line order: a function of the arguments alone.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hgp_kuf_launch.hpp"
#include "hgp_kuf_semi.hpp"
#include "hgp_kuf_tile.hpp"

namespace hgp {

constexpr int LW_WAVE = 64;         // block of the matvec: one wave
constexpr int LW_THREADS = KUF_TILE_THREADS;   // block of the rmatvec: one tile of mesh points
constexpr int LW_CHUNK = 256;       // lines tested at once (rmatvec); the longest run summed in dtype
constexpr int LW_MAX_PIECES = 64;   // pieces of a line: one lane each in the matvec

__device__ __forceinline__ int lw_pieces(int p) { return p < 1 ? 1 : (p > LW_MAX_PIECES ? LW_MAX_PIECES : p); }

// end p of the pieces on one axis: 0 for p = 0 and x for p = P exactly
template <typename T>
__device__ __forceinline__ T lw_end(T xa, int p, int P) {
#pragma clang fp contract(off)
  return xa * ((T)p / (T)P);
}

// THE predicate, one axis: is [ulo, uhi] within rho of [lo, hi]?  A node is ulo = uhi = u.
template <typename T>
__device__ __forceinline__ bool lw_near(T lo, T hi, T ulo, T uhi, T rho) {
#pragma clang fp contract(off)
  return lo - uhi <= rho && ulo - hi <= rho;
}

// piece p of a line's axis against [ulo, uhi]
template <typename T>
__device__ __forceinline__ bool lw_piece_near(T xa, int p, int P, T ulo, T uhi, T rho) {
  const T e0 = lw_end<T>(xa, p, P), e1 = lw_end<T>(xa, p + 1, P);
  return lw_near<T>(fmin(e0, e1), fmax(e0, e1), ulo, uhi, rho);
}

// the whole segment's axis (ends 0 and x) against [ulo, uhi]
template <typename T>
__device__ __forceinline__ bool lw_hull_near(T xa, T ulo, T uhi, T rho) {
  return lw_near<T>(fmin((T)0, xa), fmax((T)0, xa), ulo, uhi, rho);
}

// a line has a window at all: some coordinate is not 0 (NaN counts; it then fails lw_near)
template <typename T>
__device__ __forceinline__ bool lw_live(T x0, T x1, T x2) {
  return x0 != (T)0 || x1 != (T)0 || x2 != (T)0;
}

// membership of (line x with P pieces, box [ulo, uhi]) over the pieces pa .. pb
template <typename T, int D>
__device__ __forceinline__ bool lw_piece_in(const T (&xv)[3], int p, int P, const T (&ulo)[3], const T (&uhi)[3],
                                            T rho) {
  bool in = lw_piece_near<T>(xv[0], p, P, ulo[0], uhi[0], rho);
  if (D > 1) in = in && lw_piece_near<T>(xv[1], p, P, ulo[1], uhi[1], rho);
  if (D > 2) in = in && lw_piece_near<T>(xv[2], p, P, ulo[2], uhi[2], rho);
  return in;
}

template <typename T, int D>
__device__ __forceinline__ bool lw_in(const T (&xv)[3], int P, int pa, int pb, const T (&u)[3], T rho) {
  for (int p = pa; p <= pb; ++p)
    if (lw_piece_in<T, D>(xv, p, P, u, u, rho)) return true;
  return false;
}

// first i in [0, m] from which lo - g[i] <= rho holds (upper = false: the range's begin) or from
// which g[i] - hi <= rho fails (upper = true: its end); g strictly increasing.  NaN: m and 0.
template <typename T>
__device__ __forceinline__ int64_t lw_first(const T* __restrict__ g, int64_t m, T lo, T hi, T rho, bool upper) {
#pragma clang fp contract(off)
  int64_t a = 0, b = m;
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    const T gv = g[mid];
    if (upper ? !(gv - hi <= rho) : lo - gv <= rho)
      b = mid;
    else
      a = mid + 1;
  }
  return a;
}

template <typename T, int MODE, int NW>
__global__ __launch_bounds__(LW_WAVE) void k_kuf_line_win_mv(KufGrid g, const T* __restrict__ x, int64_t B, int kind,
                                                            T sig2, T ell, T kp, T rho, int npts,
                                                            const T* __restrict__ u, const int* __restrict__ pieces,
                                                            const T* __restrict__ w, int nwv, int64_t M, int nsplit,
                                                            double* __restrict__ part, T* __restrict__ out,
                                                            int64_t ldo) {
  __shared__ T so_s[MODE == 1 ? SEMI_MAX_NPTS : 1];
  __shared__ T xl_s[MODE == 1 ? SEMI_MAX_NPTS : 1];
  const int d = g.d;
  const int lane = threadIdx.x;
  const int64_t inner = g.m[d - 1];
  const int64_t slice = (int64_t)blockIdx.x % nsplit;
  const int64_t n = (int64_t)blockIdx.x / nsplit;           // < B: the grid is B * nsplit blocks
  const T* g0 = reinterpret_cast<const T*>(g.g[0]);
  const T* g1 = reinterpret_cast<const T*>(g.g[d > 1 ? 1 : 0]);
  const T* gl = reinterpret_cast<const T*>(g.g[d - 1]);
  const int64_t m1 = d == 3 ? g.m[1] : 1;
  const T x0 = x[n * d];
  const T x1 = d > 1 ? x[n * d + 1] : (T)0;
  const T x2 = d > 2 ? x[n * d + 2] : (T)0;
  const T xl = d == 1 ? x0 : (d == 2 ? x1 : x2);
  const int P = lw_pieces(pieces[n]);
  // the outer bounding range: lanes 0 .. 3 search begin / end of outer axes 0 and 1 (absent: [0, 1))
  long long r = lane & 1;
  {
    const int a = (lane & 3) >> 1;
    if (a < d - 1) {
      const T xa = a == 0 ? x0 : x1;
      r = lw_first<T>(a == 0 ? g0 : g1, g.m[a], fmin((T)0, xa), fmax((T)0, xa), rho, (lane & 1) != 0);
    }
    if (!lw_live<T>(x0, x1, x2)) r = 0;
  }
  const int64_t lo0 = __shfl(r, 0, 64), hi0 = __shfl(r, 1, 64), lo1 = __shfl(r, 2, 64), hi1 = __shfl(r, 3, 64);
  const int64_t n0 = hi0 > lo0 ? hi0 - lo0 : 0, n1 = hi1 > lo1 ? hi1 - lo1 : 0;
  const int64_t nrows = n0 * n1;
  const int64_t r0 = slice * nrows / nsplit, r1 = (slice + 1) * nrows / nsplit;
  const T* wp[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) wp[s] = w + (int64_t)(s < nwv ? s : nwv - 1) * M;
  double acc[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) acc[s] = 0;
  const T dist = semi_dist<T>(x, n, d);
  const bool sq = scaled_dist(kind);
  const T uoff = MODE == 1 ? semi_mc_offset<T>(u, npts) : (T)0;
  const T sinv = (T)1 / (ell * ell);
  T xs[3] = {0, 0, 0};
  const T av = MODE == 2 ? semi_sq_line<T>(x, n, d, sinv, xs) : (T)1;
  const T scale = sqrt((T)1 / av);

  for (int64_t row = r0; row < r1; ++row) {                   // the same trips and skips for every lane
    const int64_t i0 = d >= 2 ? lo0 + row / n1 : 0;           // index on axis 0 (an outer axis from d = 2 on)
    const int64_t i1 = d == 3 ? lo1 + row % n1 : 0;           // index on axis 1 (outer for d = 3)
    const T u0 = d >= 2 ? g0[i0] : (T)0;
    const T u1 = d == 3 ? g1[i1] : (T)0;
    // the pieces whose box admits the row's outer coordinates: lane p tests piece p
    bool ok = lane < P;
    if (d >= 2) ok = ok && lw_piece_near<T>(x0, lane, P, u0, u0, rho);
    if (d == 3) ok = ok && lw_piece_near<T>(x1, lane, P, u1, u1, rho);
    const unsigned long long run = __ballot(ok);
    if (run == 0) continue;
    const int pa = __ffsll(run) - 1, pb = 63 - __clzll(run);
    const T ea = lw_end<T>(xl, pa, P), eb = lw_end<T>(xl, pb + 1, P);
    const T L = fmin(ea, eb), H = fmax(ea, eb);
    const int64_t ia = lw_first<T>(gl, inner, L, H, rho, false), ib = lw_first<T>(gl, inner, L, H, rho, true);
    if (ia >= ib) continue;
    const int64_t o = d == 3 ? i0 * m1 + i1 : i0;             // the dense kernels' outer index
    if (MODE == 1) {
      __syncthreads();                                        // the last row's readers are done
      for (int a = lane; a < npts; a += LW_WAVE) {
        const T al = semi_mc_alpha<T>(a, npts, uoff);
        so_s[a] = semi_mc_outer<T>(d, [&](int ax) -> T {
          return semi_mc_sqd<T>(ax == 0 ? u0 : u1, ax == 0 ? x0 : x1, al, sq, ell);
        });
        xl_s[a] = xl * al;
      }
      __syncthreads();
      for (int64_t i = ia + lane; i < ib; i += LW_WAVE) {
        const T kv = semi_mc_elem<T>(kind, d, gl[i], npts, sq, sig2, ell, kp, dist, [&](int a, T& xa, T& so) {
          xa = xl_s[a];
          so = so_s[a];
        });
#pragma unroll
        for (int s = 0; s < NW; ++s) acc[s] += (double)(kv * wp[s][o * inner + i]);
      }
    } else {
      T bo, co;
      semi_sq_outer<T>(d, xs, sinv, [&](int ax) -> T { return ax == 0 ? u0 : u1; }, bo, co);
      for (int64_t i = ia + lane; i < ib; i += LW_WAVE) {
        const T kv = semi_sq_elem<T>(d, bo, co, xs[d - 1], gl[i], sinv, av, scale, sig2, dist);
#pragma unroll
        for (int s = 0; s < NW; ++s) acc[s] += (double)(kv * wp[s][o * inner + i]);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < NW; ++s)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[s] += __shfl_xor(acc[s], off, 64);
  if (lane == 0) {
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
}

template <typename T, int MODE, int NC, int D>
__global__ __launch_bounds__(LW_THREADS) void k_kuf_line_win_rmv(KufGrid g, const T* __restrict__ x, int64_t B,
                                                                int kind, T sig2, T ell, T kp, T rho, int npts,
                                                                const T* __restrict__ u,
                                                                const int* __restrict__ pieces,
                                                                const T* __restrict__ c, int ncv, int64_t M,
                                                                T* __restrict__ out) {
  __shared__ T xv_s[D][LW_CHUNK];                             // a survivor's end point
  __shared__ T cs[NC][LW_CHUNK];                              // its coefficients
  __shared__ T dist_s[LW_CHUNK];                              // |x|
  __shared__ T xq_s[MODE == 2 ? D : 1][MODE == 2 ? LW_CHUNK : 1];   // x S
  __shared__ T av_s[MODE == 2 ? LW_CHUNK : 1];                // x S x
  __shared__ int pc_s[LW_CHUNK];                              // P | pa << 8 | pb << 16
  __shared__ T al_s[MODE == 1 ? SEMI_MAX_NPTS : 1];           // the Monte-Carlo nodes' alpha
  __shared__ int cnt_s[LW_THREADS / 64];
  constexpr int T0 = KufTile<D>::T0, T1 = KufTile<D>::T1, T2 = KufTile<D>::T2;
  const int d = g.d;                                          // = D; an argument, not a constant, for the
  const int tid = threadIdx.x;                                // axis loops of hgp_kuf_semi.hpp
  const int lane = tid & 63, wv = tid >> 6;
  // the block's tile and the thread's mesh point in it
  const KufTilePos tp = kuf_tile_pos<D>(g);
  const int64_t m0 = tp.m0, m1 = tp.m1, m2 = tp.m2, i0 = tp.i0, i1 = tp.i1, i2 = tp.i2;
  const bool live = tp.live;
  const T* g0 = reinterpret_cast<const T*>(g.g[0]);
  const T* g1 = reinterpret_cast<const T*>(g.g[D > 1 ? 1 : 0]);
  const T* g2 = reinterpret_cast<const T*>(g.g[D > 2 ? 2 : 0]);
  T uv[3] = {0, 0, 0}, tlo[3] = {0, 0, 0}, thi[3] = {0, 0, 0};
  uv[0] = g0[i0 < m0 ? i0 : m0 - 1];
  tlo[0] = g0[tp.t0 * T0];
  thi[0] = g0[tp.t0 * T0 + T0 - 1 < m0 ? tp.t0 * T0 + T0 - 1 : m0 - 1];
  if (D > 1) {
    uv[1] = g1[i1 < m1 ? i1 : m1 - 1];
    tlo[1] = g1[tp.t1 * T1];
    thi[1] = g1[tp.t1 * T1 + T1 - 1 < m1 ? tp.t1 * T1 + T1 - 1 : m1 - 1];
  }
  if (D > 2) {
    uv[2] = g2[i2 < m2 ? i2 : m2 - 1];
    tlo[2] = g2[tp.t2 * T2];
    thi[2] = g2[tp.t2 * T2 + T2 - 1 < m2 ? tp.t2 * T2 + T2 - 1 : m2 - 1];
  }
  const bool sq = scaled_dist(kind);
  const T sinv = (T)1 / (ell * ell);
  if (MODE == 1) {
    const T uoff = semi_mc_offset<T>(u, npts);
    for (int a = tid; a < npts; a += LW_THREADS) al_s[a] = semi_mc_alpha<T>(a, npts, uoff);
  }
  T co = 0;                                                   // MODE 2: the node's own outer term of c
  if (MODE == 2) {
    T xz[3] = {0, 0, 0}, bz;
    semi_sq_outer<T>(d, xz, sinv, [&](int ax) -> T { return ax == 0 ? uv[0] : uv[1]; }, bz, co);
    co = semi_rounded(co);
  }
  double acc[NC];
#pragma unroll
  for (int s = 0; s < NC; ++s) acc[s] = 0;
  for (int64_t k0 = 0; k0 < B; k0 += LW_CHUNK) {
    __syncthreads();                                          // the last chunk's readers are done (and al_s stands)
    // cull: thread tid tests line k0 + tid against the tile's box
    const int64_t n = k0 + tid;
    T xn[3] = {0, 0, 0};
    int P = 1, pa = 0, pb = -1;
    if (n < B) {
#pragma unroll
      for (int a = 0; a < D; ++a) xn[a] = x[n * D + a];
      P = lw_pieces(pieces[n]);
      bool near = lw_live<T>(xn[0], xn[1], xn[2]) && lw_hull_near<T>(xn[0], tlo[0], thi[0], rho);
      if (D > 1) near = near && lw_hull_near<T>(xn[1], tlo[1], thi[1], rho);
      if (D > 2) near = near && lw_hull_near<T>(xn[2], tlo[2], thi[2], rho);
      if (near) {
        pa = P;
        for (int p = 0; p < P; ++p)
          if (lw_piece_in<T, D>(xn, p, P, tlo, thi, rho)) {
            pa = p < pa ? p : pa;
            pb = p;
          }
      }
    }
    const bool keep = pb >= pa;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) cnt_s[wv] = __popcll(bal);
    __syncthreads();
    int pos = __popcll(bal & ((1ull << lane) - 1ull)), cnt = 0;
#pragma unroll
    for (int k = 0; k < LW_THREADS / 64; ++k) {
      if (k < wv) pos += cnt_s[k];
      cnt += cnt_s[k];
    }
    if (cnt == 0) continue;                                   // the same for every thread of the block
    if (keep) {                                               // pos < cnt <= LW_CHUNK
#pragma unroll
      for (int a = 0; a < D; ++a) xv_s[a][pos] = xn[a];
#pragma unroll
      for (int s = 0; s < NC; ++s) cs[s][pos] = c[(int64_t)(s < ncv ? s : ncv - 1) * B + n];
      dist_s[pos] = semi_dist<T>(x, n, d);
      pc_s[pos] = P | pa << 8 | pb << 16;
      if (MODE == 2) {
        T xs[3] = {0, 0, 0};
        av_s[pos] = semi_sq_line<T>(x, n, d, sinv, xs);
#pragma unroll
        for (int a = 0; a < D; ++a) xq_s[MODE == 2 ? a : 0][MODE == 2 ? pos : 0] = xs[a];
      }
    }
    __syncthreads();
    if (live) {
      T run[NC];
#pragma unroll
      for (int s = 0; s < NC; ++s) run[s] = 0;
      for (int k = 0; k < cnt; ++k) {
        T pv[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < D; ++a) pv[a] = xv_s[a][k];
        const int pc = pc_s[k];
        if (!lw_in<T, D>(pv, pc & 0xff, (pc >> 8) & 0xff, (pc >> 16) & 0xff, uv, rho)) continue;
        const T dist = dist_s[k];
        T kv;
        if (MODE == 1) {
          kv = semi_mc_elem<T>(kind, D, uv[D - 1], npts, sq, sig2, ell, kp, dist, [&](int a, T& xa, T& so) {
            const T al = al_s[a];
            xa = semi_rounded(pv[D - 1] * al);
            so = semi_rounded(semi_mc_outer<T>(D, [&](int ax) -> T {
              return semi_mc_sqd<T>(ax == 0 ? uv[0] : uv[1], ax == 0 ? pv[0] : pv[1], al, sq, ell);
            }));
          });
        } else {
          T xs[3] = {0, 0, 0};
#pragma unroll
          for (int a = 0; a < D; ++a) xs[a] = xq_s[MODE == 2 ? a : 0][MODE == 2 ? k : 0];
          const T av = av_s[MODE == 2 ? k : 0];
          T bo, cz;
          semi_sq_outer<T>(d, xs, sinv, [&](int ax) -> T { return ax == 0 ? uv[0] : uv[1]; }, bo, cz);
          kv = semi_sq_elem<T>(D, semi_rounded(bo), co, xs[D - 1], uv[D - 1], sinv, av, sqrt((T)1 / av), sig2, dist);
        }
#pragma unroll
        for (int s = 0; s < NC; ++s) run[s] += kv * cs[s][k];
      }
#pragma unroll
      for (int s = 0; s < NC; ++s) acc[s] += (double)run[s];
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
static hipError_t kuf_line_matvec_win_t(const KufObs& o, const void* wv, int64_t nw, void* outv) {
  const int64_t nobs = o.nobs;
  hipStream_t s = o.stream;
  KufGrid g{};
  int64_t M, outer;
  kuf_fill_grid(g, o.ndim, o.m, o.grids, &M, &outer);
  const T* x = reinterpret_cast<const T*>(o.x);
  const T* w = reinterpret_cast<const T*>(wv);
  const T* u = reinterpret_cast<const T*>(o.u);
  T* out = reinterpret_cast<T*>(outv);
  // the split: a pure function of (nobs, the grid) and the CU count; a slice is a share of the rows
  // of the line's own outer bounding range
  hipError_t e = hipSuccess;
  const int64_t target = (int64_t)16 * kuf_cus(&e);
  if (e != hipSuccess) return e;
  int64_t nsplit = (target + nobs - 1) / nobs;
  if (nsplit > outer) nsplit = outer;
  if (nsplit < 1) nsplit = 1;
  if (nobs * nsplit > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const unsigned nb = (unsigned)(nobs * nsplit);
  return kuf_row_groups(
      nw, nsplit > 1 ? (size_t)nsplit * (size_t)nobs : 0, s,
      [&](int64_t s0, int NW, int nwv, double* part) {
        kuf_with_mode(o.mode, [&](auto MD) {
          kuf_with_width(NW, [&](auto W) {
            hipLaunchKernelGGL((k_kuf_line_win_mv<T, decltype(MD)::value, decltype(W)::value>), dim3(nb),
                               dim3(LW_WAVE), 0, s, g, x, nobs, o.kind, (T)o.sig2, (T)o.ell[0], (T)o.kp, (T)o.rho[0],
                               o.npts, u, o.pieces, w + s0 * M, nwv, M, (int)nsplit, part, out + s0, nw);
          });
        });
      },
      [&](int64_t s0, int NW, int nwv, double* part) {
        const int64_t tot = nobs * NW;
        hipLaunchKernelGGL((k_kuf_mv_finish<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, part,
                           (int)nsplit, nobs, NW, nwv, out + s0, nw);
      });
}

// nobs >= 0 (0: out zeroed), nc > 0
template <typename T>
static hipError_t kuf_line_rmatvec_win_t(const KufObs& o, const void* cv, int64_t nc, void* outv) {
  const int64_t nobs = o.nobs;
  hipStream_t s = o.stream;
  KufGrid g{};
  int64_t M;
  kuf_fill_grid(g, o.ndim, o.m, o.grids, &M);
  T* out = reinterpret_cast<T*>(outv);
  if (nobs == 0) return hipMemsetAsync(out, 0, (size_t)nc * (size_t)M * sizeof(T), s);   // an empty sum
  const T* x = reinterpret_cast<const T*>(o.x);
  const T* c = reinterpret_cast<const T*>(cv);
  const T* u = reinterpret_cast<const T*>(o.u);
  const int64_t ntile = kuf_tile_count(o.ndim, o.m);
  if (ntile > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const unsigned nb = (unsigned)ntile;
  return kuf_row_groups(nc, s, [&](int64_t s0, int NC, int ncv, double*) {
    kuf_with_mode(o.mode, [&](auto MD) {
      kuf_with_dim(o.ndim, [&](auto D) {
        kuf_with_width(NC, [&](auto W) {
          hipLaunchKernelGGL(
              (k_kuf_line_win_rmv<T, decltype(MD)::value, decltype(W)::value, decltype(D)::value>), dim3(nb),
              dim3(LW_THREADS), 0, s, g, x, nobs, o.kind, (T)o.sig2, (T)o.ell[0], (T)o.kp, (T)o.rho[0], o.npts, u,
              o.pieces, c + s0 * nobs, ncv, M, out + s0 * M);
        });
      });
    });
  });
}

// launchers behind hgp_kuf_semi_{mc,sqexp}_matvec_win and hgp_kuf_semi_{mc,sqexp}_rmatvec_win
hipError_t kuf_line_matvec_win(const KufObs& o, const void* w, int64_t nw, void* out) {
  return kuf_with_dtype(o.dtype, [&](auto t) { return kuf_line_matvec_win_t<decltype(t)>(o, w, nw, out); });
}

hipError_t kuf_line_rmatvec_win(const KufObs& o, const void* c, int64_t nc, void* out) {
  return kuf_with_dtype(o.dtype, [&](auto t) { return kuf_line_rmatvec_win_t<decltype(t)>(o, c, nc, out); });
}

}  // namespace hgp
