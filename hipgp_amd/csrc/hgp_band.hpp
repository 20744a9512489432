// hgp_band.hpp — the product-form K matvec of a short-support kernel as two banded matrix products
// on the matrix cores.
//
// Where the 1-D factors t0, t1 of a product-form column (hgp_sep_host.hpp) vanish in fp32 beyond a
// few taps (band_radius), T0 and T1 are banded and K X = T0 X T1^T + sigma X needs no transform:
//   k_band_row : V = X S1            (axis 1, along the rows of one RHS)
//   k_band_col : Y = S0^T V + sigma X (axis 0, down its columns)
// Both build 16 x 16 output blocks with v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate: bit for bit
// an fmaf chain).  A block at outputs j0 .. j0 + 15 needs inputs j0 - r .. j0 + 15 + r, a K depth
// of 16 + 2r; the Toeplitz slab S[k][n] = t[|k - r - n|] is the same for every block, so each lane
// holds its (16 + 2r) / 4 slab values in registers for the whole kernel.  r is a runtime argument,
// even (the host rounds it up; the extra slab rows are zero taps), so that K is a multiple of 4.
//
// Operand maps of the instruction (lane l, h = l >> 4, n = l & 15): A[row n][k = 4s + h],
// B[k = 4s + h][col n] for k-step s; D[row 4h + reg][col n].
//   k_band_row: A = the X tile read from LDS (16 rows x (256 + 2r) columns, pitch = 2 mod 32: the
//               32 lanes of a ds_read_b32 group hit 32 banks), B = the slab.  4 waves, each 64
//               output columns = 4 independent accumulators.
//   k_band_col: A = the slab, B = V rows from LDS ((128 + 2r) rows x 32 columns, pitch 32, odd rows
//               with their two 16-column halves swapped: again 32 banks).  4 waves, each 32 output
//               rows x 32 columns = 4 accumulators; a fragment read serves both of the wave's row
//               blocks (row block 1 at step s reads the rows of row block 0 at step s + 4).
// Inputs outside the grid are zeros (masked loads), outputs outside it are not stored; neither pads,
// transposes nor exchanges anything.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// largest tap radius the banded path takes (the measured crossover with k_sep_pass)
#ifndef HGP_BAND_RMAX
#define HGP_BAND_RMAX 32
#endif

namespace hgp {

struct BandDesc {
  const float* in;            // [Q][m0][m1]
  float* out;                 // [Q][m0][m1]
  const float* add;           // optional, [Q][m0][m1]: out += sigma add
  float sigma;
  const float* taps;          // BAND_TAPS values of this axis' factor, zero beyond its radius
  int m0, m1;
  int r;                      // even, <= BandCfg::RE
  int Q;
  const int* done;
};

constexpr int BAND_TAPS = 64;   // |k - r - n| <= r + 15

template <int RMAX> struct BandCfg {
  static constexpr int RE = (RMAX + 1) / 2 * 2;                   // radius rounded up to even
  static constexpr int KS = (16 + 2 * RE) / 4;                    // k-steps at the largest radius
  static constexpr int THREADS = 256;
  // k_band_row: 16 rows x TW columns per block
  static constexpr int TW = 256;
  static constexpr int PA = (TW + 2 * RE + 31) / 32 * 32 + 2;
  static constexpr int LD_A = (TW + 2 * RE + 63) / 64;            // loads per lane and row
  // k_band_col: TH rows x 32 columns per block
  static constexpr int TH = 128;
  static constexpr int ROWS_B = TH + 2 * RE;
  static constexpr int LD_B = (ROWS_B + 7) / 8;                   // loads per thread
  static_assert(RE + 15 < BAND_TAPS, "tap table too short");
  static_assert(16 * PA * 4 <= 65536 && ROWS_B * 32 * 4 <= 65536, "static LDS");
};

typedef float band_f32x4 __attribute__((ext_vector_type(4)));

// the lane's slab values: t[|4s + h - r - n|] for k-step s (the A operand's [row n][k] and the B
// operand's [k][col n] alike: the slab is symmetric under the swap)
template <int KS>
__device__ __forceinline__ void band_slab(float (&w)[KS], const float* taps, int r, int lane) {
  const int h = lane >> 4, n = lane & 15;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    int j = 4 * s + h - r - n;
    j = j < 0 ? -j : j;
    w[s] = j < BAND_TAPS ? taps[j] : 0.f;
  }
}

template <int RMAX>
__global__ __launch_bounds__(256) void k_band_row(const BandDesc d) {
  using Cfg = BandCfg<RMAX>;
  constexpr int TW = Cfg::TW, PA = Cfg::PA, KS = Cfg::KS, LD = Cfg::LD_A;
  if (d.done != nullptr && *d.done) return;                          // uniform: before any barrier
  __shared__ float tile[16 * PA];
  const int m0 = d.m0, m1 = d.m1, r = d.r;
  const int ncb = (m1 + TW - 1) / TW, nrb = (m0 + 15) / 16;
  int b = blockIdx.x;
  const int cbk = b % ncb;
  b /= ncb;
  const int rbk = b % nrb;
  const int q = b / nrb;
  const int j0 = cbk * TW, i0 = rbk * 16;
  const int W = TW + 2 * r;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int h = lane >> 4, n = lane & 15;
  const int64_t base = (int64_t)q * m0 * m1;

  // rows 4w .. 4w + 3 of the tile, columns j0 - r .. j0 + TW + r: whole-wave row-contiguous loads
  float v[4][LD];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int gi = i0 + 4 * w + rr;
    const float* p = d.in + base + (int64_t)(gi < m0 ? gi : 0) * m1;
#pragma unroll
    for (int u = 0; u < LD; ++u) {
      const int c = lane + 64 * u, gc = j0 - r + c;
      v[rr][u] = (c < W && gi < m0 && gc >= 0 && gc < m1) ? p[gc] : 0.f;
    }
  }
  float bw[KS];
  band_slab<KS>(bw, d.taps, r, lane);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int u = 0; u < LD; ++u) {
      const int c = lane + 64 * u;
      if (c < W) tile[(4 * w + rr) * PA + c] = v[rr][u];
    }
  __syncthreads();

  const int cw = 64 * w;
  if (j0 + cw >= m1) return;                                         // wave-uniform, after the barrier
  const int ks = (16 + 2 * r) / 4;
  band_f32x4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc[cb] = band_f32x4{0.f, 0.f, 0.f, 0.f};
  const float* a0 = tile + n * PA + cw + h;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    if (s < ks) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[16 * cb + 4 * s], bw[s], acc[cb], 0, 0, 0);
    }
  }
  float* o = d.out + base;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int gi = i0 + 4 * h + reg;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int gc = j0 + cw + 16 * cb + n;
      if (gi < m0 && gc < m1) o[(int64_t)gi * m1 + gc] = acc[cb][reg];
    }
  }
}

template <int RMAX>
__global__ __launch_bounds__(256) void k_band_col(const BandDesc d) {
  using Cfg = BandCfg<RMAX>;
  constexpr int TH = Cfg::TH, KS = Cfg::KS, LD = Cfg::LD_B;
  if (d.done != nullptr && *d.done) return;                          // uniform: before any barrier
  __shared__ float tile[Cfg::ROWS_B * 32];
  const int m0 = d.m0, m1 = d.m1, r = d.r;
  const int ncb = (m1 + 31) / 32, nrb = (m0 + TH - 1) / TH;
  int b = blockIdx.x;
  const int cbk = b % ncb;
  b /= ncb;
  const int rbk = b % nrb;
  const int q = b / nrb;
  const int j0 = cbk * 32, i0 = rbk * TH;
  const int R = TH + 2 * r;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int h = lane >> 4, n = lane & 15;
  const int64_t base = (int64_t)q * m0 * m1;

  // rows i0 - r .. i0 + TH + r of 32 columns (one 128-B segment each), 8 rows per sweep
  {
    const int c = threadIdx.x & 31, k0 = threadIdx.x >> 5;
    const int gc = j0 + c;
    const float* p = d.in + base + (gc < m1 ? gc : 0);
    float v[LD];
#pragma unroll
    for (int u = 0; u < LD; ++u) {
      const int k = k0 + 8 * u, gi = i0 - r + k;
      v[u] = (k < R && gi >= 0 && gi < m0 && gc < m1) ? p[(int64_t)gi * m1] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < LD; ++u) {
      const int k = k0 + 8 * u;
      if (k < R) tile[k * 32 + (c ^ ((k & 1) << 4))] = v[u];
    }
  }
  float aw[KS];
  band_slab<KS>(aw, d.taps, r, lane);
  __syncthreads();

  const int rw = 32 * w;
  if (i0 + rw >= m0) return;                                         // wave-uniform, after the barrier
  const int ks = (16 + 2 * r) / 4;
  band_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i >> 1][i & 1] = band_f32x4{0.f, 0.f, 0.f, 0.f};
  // tile row rw + 4u + h: its parity is h's
  const float* p0 = tile + (rw + h) * 32 + (n ^ ((h & 1) << 4));
  const float* p1 = tile + (rw + h) * 32 + ((16 + n) ^ ((h & 1) << 4));
#pragma unroll
  for (int u = 0; u < KS + 4; ++u) {
    if (u < ks + 4) {
      const float f0 = p0[128 * u], f1 = p1[128 * u];
      if (u < KS && u < ks) {                                        // row block 0, k-step u
        const float a = aw[u < KS ? u : 0];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, f0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, f1, acc[0][1], 0, 0, 0);
      }
      if (u >= 4) {                                                  // row block 1, k-step u - 4
        const float a = aw[u >= 4 ? u - 4 : 0];
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, f0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, f1, acc[1][1], 0, 0, 0);
      }
    }
  }
  float* o = d.out + base;
  const bool add = d.add != nullptr;                                 // uniform
  const float* x = add ? d.add + base : nullptr;
  const float sg = d.sigma;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    float xv[4][2];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int gi = i0 + rw + 16 * rb + 4 * h + reg;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const int gc = j0 + 16 * cb + n;
        xv[reg][cb] = (add && gi < m0 && gc < m1) ? x[(int64_t)gi * m1 + gc] : 0.f;
      }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int gi = i0 + rw + 16 * rb + 4 * h + reg;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const int gc = j0 + 16 * cb + n;
        if (gi < m0 && gc < m1) o[(int64_t)gi * m1 + gc] = add ? acc[rb][cb][reg] + sg * xv[reg][cb] : acc[rb][cb][reg];
      }
    }
  }
}

// axis 1: k_band_row, axis 0: k_band_col (hgp_band_f32.hip)
hipError_t launch_band(int axis, const BandDesc& d, hipStream_t s);

}  // namespace hgp
