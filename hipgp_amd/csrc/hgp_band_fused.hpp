// hgp_band_fused.hpp — the two banded products of hgp_band.hpp in one kernel, the
// intermediate V = X S1 kept in LDS:  Y = S0^T (X S1) + sigma X.
//
// A block owns SEG rows x TW columns of one RHS and marches down its segment 16 rows at a time.
// March step t (X rows seg0 - r0 + 16 t .. + 15, which the previous step staged in LDS):
//   1. the global loads of the NEXT 16 X rows (columns j0 - r1 .. j0 + TW + r1, zeros outside the
//      grid) are issued into registers, and so are the x values of this step's sigma x epilogue;
//   2. row product: 16 rows of V for the strip's TW columns, from the accumulators into group
//      t mod NG of a ring of NG 16-row groups;
//   3. from step D = ceil(2 r0 / 16) on, column product: output rows seg0 + 16 (t - D) .. + 15 from
//      the ring's rows 16 (t - D) .. 16 (t - D) + 15 + 2 r0, epilogue as k_band_col, store;
//   4. the registers of 1. go to the other X stage; one block barrier.
// Each of the 4 waves owns TW / 4 columns end to end: its part of the ring is written and read by
// this wave alone, so V needs no block barrier; the only shared LDS is the double-buffered X stage.
// Both summations run in the order of k_band_row / k_band_col (k ascending from a zero accumulator,
// blocks aligned to 16 from index 0, the same epilogue expression): the result is bit for bit the
// two-pass one.  V rows outside the grid are zeros because their X rows are masked to zero.
//
// LDS.  X stage: 16 rows at pitch PA = 2 mod 32, the A operand of the row product as in k_band_row
// (lane (h, n) reads [n][c + h]: banks 2 n + h, 32 of them per 32-lane group).  Ring: NG * 16 rows
// at pitch TW (a multiple of 32), odd rows with the two 16-column halves of every 32 swapped, the B
// operand of the column product as in k_band_col (lane (h, n) reads row k + h: 32 banks).  The D
// layout writes rows 4 h + reg: the two h of a 32-lane group share a parity and 16 banks, a 2-way
// conflict that a ds_write_b32 hides behind its own data transfer.
#pragma once
#include "hgp_band.hpp"

// column strip of a block: 128 (two blocks a CU) or 256 (one)
#ifndef HGP_BAND_FUSED_TW
#define HGP_BAND_FUSED_TW 128
#endif
#ifndef HGP_BAND_FUSED_SEG
#define HGP_BAND_FUSED_SEG 256
#endif

namespace hgp {

struct BandFusedDesc {
  const float* in;            // [Q][m0][m1]
  float* out;                 // [Q][m0][m1]
  float sigma;
  int add;                    // out += sigma in
  const float* taps0;         // BAND_TAPS values of axis 0's factor, zero beyond its radius
  const float* taps1;         // ... of axis 1's
  int m0, m1;
  int r0, r1;                 // even, <= BandFusedCfg::RE
  int Q;
  const int* done;
};

template <int RMAX, int TW_, int SEG_> struct BandFusedCfg {
  static constexpr int RE = (RMAX + 1) / 2 * 2;
  static constexpr int KS = (16 + 2 * RE) / 4;
  static constexpr int THREADS = 256;
  static constexpr int TW = TW_, SEG = SEG_;
  static constexpr int TWW = TW / 4;                               // columns of a wave
  static constexpr int NCB = TWW / 16;                             // 16-column blocks of a wave
  static constexpr int PA = (TW + 2 * RE + 31) / 32 * 32 + 2;
  static constexpr int LD = (TW + 2 * RE + 63) / 64;               // loads per lane and row
  static constexpr int DMAX = (2 * RE + 15) / 16;                  // steps the column product trails
  static constexpr int NG = DMAX + 2;                              // 16 + 2 RE live rows + the 16 being written
  static constexpr int LDS_BYTES = (2 * 16 * PA + NG * 16 * TW) * 4;
  static_assert(TW % 128 == 0 && SEG % 16 == 0 && SEG > 0, "strip and segment");
  static_assert(RE + 15 < BAND_TAPS, "tap table too short");
  static_assert(LDS_BYTES <= 160 * 1024, "static LDS");
};

template <int RMAX, int TW_, int SEG_>
__global__ __launch_bounds__(256) void k_band_fused(const BandFusedDesc d) {
  using Cfg = BandFusedCfg<RMAX, TW_, SEG_>;
  constexpr int TW = Cfg::TW, SEG = Cfg::SEG, PA = Cfg::PA, KS = Cfg::KS, LD = Cfg::LD, NCB = Cfg::NCB, NG = Cfg::NG;
  constexpr int PF = 3;                                              // LDS reads in flight ahead of the MFMAs
  if (d.done != nullptr && *d.done) return;                          // uniform: before any barrier
  __shared__ float stage[2][16 * PA];
  __shared__ float ring[NG * 16 * TW];
  const int m0 = d.m0, m1 = d.m1, r0 = d.r0, r1 = d.r1;
  // strips fastest, then segments, then RHS: the blocks resident together share their halos
  const int ncb = (m1 + TW - 1) / TW, nsg = (m0 + SEG - 1) / SEG;
  int b = blockIdx.x;
  const int cbk = b % ncb;
  b /= ncb;
  const int sbk = b % nsg;
  const int q = b / nsg;
  const int j0 = cbk * TW, seg0 = sbk * SEG;
  const int W = TW + 2 * r1;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar
  const int h = lane >> 4, n = lane & 15;
  const int64_t base = (int64_t)q * m0 * m1;
  const float* xin = d.in + base;
  float* o = d.out + base;
  const int ks0 = (16 + 2 * r0) / 4, ks1 = (16 + 2 * r1) / 4;
  const int D = (2 * r0 + 15) / 16;
  const int nout = (min(SEG, m0 - seg0) + 15) / 16;                  // output row blocks of this segment
  const int T = D + nout;
  const int cw = Cfg::TWW * w;
  const bool live = j0 + cw < m1;                                    // wave-uniform
  const bool add = d.add != 0;                                       // uniform
  const float sg = d.sigma;

  float bw[KS], aw[KS];
  band_slab<KS>(bw, d.taps1, r1, lane);
  band_slab<KS>(aw, d.taps0, r0, lane);

  // rows 4w .. 4w + 3 of a step's 16 X rows, columns j0 - r1 .. j0 + TW + r1: whole-wave
  // row-contiguous loads.  The loads are unconditional from clamped addresses (no branch, no
  // zero-initialised destination: nothing makes the MFMAs between issue and use wait for them);
  // the zeros outside the grid are put in when the registers go to the stage.
  float v[4][LD];
  auto load_rows = [&](int t) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int gi = seg0 - r0 + 16 * t + 4 * w + rr;
      const float* p = xin + (int64_t)min(max(gi, 0), m0 - 1) * m1;
#pragma unroll
      for (int u = 0; u < LD; ++u) v[rr][u] = p[min(max(j0 - r1 + lane + 64 * u, 0), m1 - 1)];
    }
  };
  auto stage_rows = [&](float* tile, int t) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int gi = seg0 - r0 + 16 * t + 4 * w + rr;
      const bool rok = gi >= 0 && gi < m0;
#pragma unroll
      for (int u = 0; u < LD; ++u) {
        const int c = lane + 64 * u, gc = j0 - r1 + c;
        if (c < W) tile[(4 * w + rr) * PA + c] = (rok && gc >= 0 && gc < m1) ? v[rr][u] : 0.f;
      }
    }
  };
  load_rows(0);
  stage_rows(stage[0], 0);
  __syncthreads();

  int tg = 0, ug = 0;                                                // t mod NG, (t - D) mod NG
  for (int t = 0; t < T; ++t) {
    const bool more = t + 1 < T, outp = t >= D;                      // uniform
    // the k-loops' uniform exits compare against these: t >> 30 is 0, but not to the compiler,
    // which otherwise hoists every one of the 2 KS compares out of the march as a mask in two
    // SGPRs and spills them (compiler-dependent: regenerate profiles/band_fused_resource_usage.txt
    // with -Rpass-analysis=kernel-resource-usage when the toolchain changes; it must show no spills)
    const int ks0t = ks0 + (t >> 30), ks1t = ks1 + (t >> 30);
    const int i0 = seg0 + 16 * (t - D);                              // output rows of this step
    // x of the sigma x epilogue, clamped likewise (the stores are masked)
    float xv[4][NCB];                                                // read only where add
    if (live && outp && add) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float* p = xin + (int64_t)min(i0 + 4 * h + reg, m0 - 1) * m1;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) xv[reg][cb] = p[min(j0 + cw + 16 * cb + n, m1 - 1)];
      }
    }
    // after the epilogue's loads: the step never waits for these before it stages them
    if (more) load_rows(t + 1);
    if (live) {
      // row product
      band_f32x4 acc[NCB];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[cb] = band_f32x4{0.f, 0.f, 0.f, 0.f};
      const float* a0 = stage[t & 1] + n * PA + cw + h;
      // fragments are read PF steps ahead of their MFMAs, past the uniform exit too: every index
      // up to KS stays inside the stage; what is read there (columns >= TW + 2 r1, never staged)
      // may be anything and never reaches an MFMA
      float f[KS][NCB];
#pragma unroll
      for (int s = 0; s < PF && s < KS; ++s)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) f[s][cb] = a0[16 * cb + 4 * s];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        if (s >= 4 && s >= ks1t) break;                              // uniform; ks >= 4
        if (s + PF < KS) {
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) f[s + PF][cb] = a0[16 * cb + 4 * (s + PF)];
        }
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[s][cb], bw[s], acc[cb], 0, 0, 0);
      }
      // V rows 16 t + 4 h + reg of the segment's own count: row parity = reg's
      float* vr = ring + (tg * 16 + 4 * h) * TW + cw;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) vr[reg * TW + ((16 * cb + n) ^ ((reg & 1) << 4))] = acc[cb][reg];
    }
    // the ring part of a wave is its own: its LDS operations complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (live && outp) {
      band_f32x4 acc[NCB];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[cb] = band_f32x4{0.f, 0.f, 0.f, 0.f};
      // ring row 16 ug + 4 s + h (mod 16 NG; 4 s + h stays inside a group of 4): its parity is h's
      const float* p0 = ring + h * TW + cw;
      const int sw = (h & 1) << 4;
      auto ring_row = [&](int s) {                                   // uniform
        const int row = ug * 16 + 4 * s;
        return p0 + (row >= NG * 16 ? row - NG * 16 : row) * TW;
      };
      // PF steps ahead, as above: a ring row past the exit (or, in the first steps, a group not
      // yet written) is in bounds by the wrap, may hold anything and never reaches an MFMA
      float g[KS][NCB];
#pragma unroll
      for (int s = 0; s < PF && s < KS; ++s)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) g[s][cb] = ring_row(s)[(16 * cb + n) ^ sw];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        if (s >= 4 && s >= ks0t) break;                              // uniform; ks >= 4
        if (s + PF < KS) {
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) g[s + PF][cb] = ring_row(s + PF)[(16 * cb + n) ^ sw];
        }
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[s], g[s][cb], acc[cb], 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int gi = i0 + 4 * h + reg;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const int gc = j0 + cw + 16 * cb + n;
          if (gi < m0 && gc < m1) o[(int64_t)gi * m1 + gc] = add ? acc[cb][reg] + sg * xv[reg][cb] : acc[cb][reg];
        }
      }
    }
    if (outp) ug = ug + 1 == NG ? 0 : ug + 1;
    tg = tg + 1 == NG ? 0 : tg + 1;
    if (more) {
      stage_rows(stage[(t + 1) & 1], t + 1);
      __syncthreads();                                               // T is uniform
    }
  }
}

// one launch over all d.Q right-hand sides (hgp_band_fused_f32.hip)
hipError_t launch_band_fused(const BandFusedDesc& d, hipStream_t s);
// {SEG, TW} of the built kernel
void band_fused_tile(int tile[2]);

}  // namespace hgp
