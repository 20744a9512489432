// hgp_kuf_tile.hpp — the tile of mesh points that a block of the two gather kernels owns
// (k_kuf_win_rmv, k_kuf_line_win_rmv), one point per thread of a 256-thread block, and the bins of
// hgp_kuf_win_bins, which are cells in groups of the same widths.  The numbers stand here alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hgp_kuf_eval.hpp"

namespace hgp {

constexpr int KUF_TILE_THREADS = 256;

// mesh points of a tile along axes 0, 1, 2 of a D-axis grid: 256 | 16 x 16 | 4 x 8 x 8
template <int D>
struct KufTile {
  static constexpr int T0 = D == 1 ? 256 : (D == 2 ? 16 : 4);
  static constexpr int T1 = D == 1 ? 1 : (D == 2 ? 16 : 8);
  static constexpr int T2 = D == 3 ? 8 : 1;
  static_assert(T0 * T1 * T2 == KUF_TILE_THREADS, "one mesh point per thread");
};

// the same for a run-time ndim; a < ndim
inline int kuf_tile(int ndim, int a) {
  if (ndim == 1) return KufTile<1>::T0;
  if (ndim == 2) return a == 0 ? KufTile<2>::T0 : KufTile<2>::T1;
  return a == 0 ? KufTile<3>::T0 : (a == 1 ? KufTile<3>::T1 : KufTile<3>::T2);
}

// tiles that cover the mesh: the gather kernels' grid size
inline int64_t kuf_tile_count(int ndim, const int64_t* m) {
  int64_t ntile = 1;
  for (int a = 0; a < ndim; ++a) ntile *= (m[a] + kuf_tile(ndim, a) - 1) / kuf_tile(ndim, a);
  return ntile;
}

// Where a thread stands: t0, t1, t2 the block's tile on each axis (tiles in C order over the axes'
// tiles; the tile's first mesh index on axis a is ta * KufTile<D>::Ta), i0, i1, i2 the thread's own
// mesh point (last axis fastest), live whether that point is on the mesh; an absent axis has one
// node.
struct KufTilePos {
  int64_t m0, m1, m2;
  int64_t t0, t1, t2;
  int64_t i0, i1, i2;
  bool live;
  // the point's index in mesh order
  template <int D>
  __device__ __forceinline__ int64_t flat() const {
    return D == 1 ? i0 : (D == 2 ? i0 * m1 + i1 : (i0 * m1 + i1) * m2 + i2);
  }
};

template <int D>
__device__ __forceinline__ KufTilePos kuf_tile_pos(const KufGrid& g) {
  using Tl = KufTile<D>;
  KufTilePos p;
  p.m0 = g.m[0];
  p.m1 = D > 1 ? g.m[1] : 1;
  p.m2 = D > 2 ? g.m[2] : 1;
  const int tid = threadIdx.x;
  const int64_t nt1 = (p.m1 + Tl::T1 - 1) / Tl::T1, nt2 = (p.m2 + Tl::T2 - 1) / Tl::T2;
  const int64_t bt = blockIdx.x;
  p.t0 = bt / (nt1 * nt2);
  p.t1 = (bt / nt2) % nt1;
  p.t2 = bt % nt2;
  p.i0 = p.t0 * Tl::T0 + tid / (Tl::T1 * Tl::T2);
  p.i1 = p.t1 * Tl::T1 + (tid / Tl::T2) % Tl::T1;
  p.i2 = p.t2 * Tl::T2 + tid % Tl::T2;
  p.live = p.i0 < p.m0 && p.i1 < p.m1 && p.i2 < p.m2;
  return p;
}

}  // namespace hgp
