// hgp_sep.hpp — one axis pass of the product-form K matvec.
//
// A product kernel on a product grid gives K = T0 (x) T1 + sigma I with T0, T1 symmetric Toeplitz,
// so K X = T0 X T1^T + sigma X: one 1-D Toeplitz matvec along each axis, each zero-padded on its
// own axis only.  k_sep_pass runs one of them on REAL data:
//   load   : real rows (2j, 2j+1) of one RHS as one complex line z = row_2j + i row_2j+1
//   conv   : pad -> FFT -> x real spectrum -> IFFT -> crop, the pruned 2H-point convolution of
//            hgp_pass.hpp (fft_line2 on the line and on its odd-half twist)
//   store  : the spectrum is real and the transform linear, so Re / Im of the result are the two
//            rows' results (no Hermitian split); they leave TRANSPOSED through an LDS tile:
//            out[q][p][row], every position p one contiguous run of the block's 2C rows
// Pass 1 runs it along axis 1 (rows i0 of x, result V[q][i1][i0]); pass 2 along axis 0 (rows i1 of
// V, result y[q][i0][i1] in the (B, M) order) and adds sigma x from the matching tile of x.
//
// Block shape: C = 8 row pairs, a pair's line on TT = H / P threads as in the row-pair kernels
// (hgp_rows.hpp): at H = 1024 fp32 eight waves and 70 KB of LDS, two blocks per CU, 4 waves per
// SIMD -- the register and LDS budget of the 1024-point column conv.  A position's 2C rows are
// then one 64-B segment in fp32 (128 B in fp64).  16 pairs make it 128 B but one 16-wave block of
// 139 KB per CU, whose load, transform and store phases nothing overlaps: measured slower, C2 K op
// 0.231 ms against 0.191 ms with 8 pairs (profiles/sep_pairs_ab.txt).
#pragma once
#include "hgp_pass.hpp"

// row pairs per block (fewer where the exchange images or 1024 threads do not hold them)
#ifndef HGP_SEP_PAIRS
#define HGP_SEP_PAIRS 8
#endif

namespace hgp {

struct SepDesc {
  const void* in;             // real rows: in + q in_q + row in_r, in_len values each
  int64_t in_q, in_r;
  int in_len, nrows;
  void* out;                  // real, transposed: out + q out_q + p out_p + row, p < out_len
  int64_t out_q, out_p;
  int out_len;
  const void* add;            // optional, out's layout: out = conv + sigma add
  double sigma;
  const void* spec;           // real spectrum of the axis, 2H values in the passes' order
  const void* tw;             // W_L^q as PassDesc::tw
  int Q, Rn;                  // right-hand sides, row pairs per RHS
  const int* done;
};

template <typename T, int H> struct SepCfg {
  static constexpr int P = PFor<T, H>::v;
  static constexpr int TT = H / P;
  static constexpr int ex_elems(int c) { return c * H + (c * H) / 16; }
  static constexpr int pitch(int c) { return 2 * c + 1; }          // tile row pitch (pad: banks)
  static constexpr int tile_bytes(int c) { return H * pitch(c) * (int)sizeof(T); }
  static constexpr int area_bytes(int c) {
    return ex_elems(c) * (int)sizeof(C2<T>) > tile_bytes(c) ? ex_elems(c) * (int)sizeof(C2<T>) : tile_bytes(c);
  }
  static constexpr int lds_bytes_for(int c) { return (area_bytes(c) + 15) / 16 * 16 + TwTab<T, H>::BYTES; }
  static constexpr int c_pairs() {
    int c = HGP_SEP_PAIRS;
    if (c * TT < 64) c = 64 / TT;                  // tiny lines: at least one whole wave
    while (c > 1 && (c * TT > 1024 || lds_bytes_for(c) > LDS_CAP)) c >>= 1;
    return c;
  }
  static constexpr int C = c_pairs();
  static constexpr int THREADS = C * TT;
  static constexpr int AREA = (area_bytes(C) + 15) / 16 * 16;
  static constexpr int LDS = lds_bytes_for(C);
  static constexpr int PITCH = pitch(C);
  static constexpr bool WAVE = TT <= 64;
  static constexpr bool FITS = LDS <= LDS_CAP && C * TT <= 1024;
  static constexpr int BLOCKS_BY_LDS = LDS_CAP / (LDS > 0 ? LDS : 1);
  static constexpr int MINW_LDS = (BLOCKS_BY_LDS * (THREADS / 64)) / 4;
  static constexpr int MINW = MINW_LDS < 1 ? 1 : (MINW_LDS > 4 ? 4 : MINW_LDS);
};

template <typename T, int H>
__global__ __launch_bounds__((SepCfg<T, H>::THREADS), (SepCfg<T, H>::MINW)) void k_sep_pass(const SepDesc d) {
  using Cfg = SepCfg<T, H>;
  constexpr int P = Cfg::P, TT = Cfg::TT, C = Cfg::C, PITCH = Cfg::PITCH, THREADS = Cfg::THREADS;
  if (d.done != nullptr && *d.done) return;                          // uniform: before any barrier
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  C2<T>* lds = reinterpret_cast<C2<T>*>(smem_raw);
  C2<T>* tab = reinterpret_cast<C2<T>*>(smem_raw + Cfg::AREA);
  stage_tw<T, H>(tab, reinterpret_cast<const C2<T>*>(d.tw), threadIdx.x, THREADS);

  const int nrb = (d.Rn + C - 1) / C;
  const int q = blockIdx.x / nrb;
  const int rb = blockIdx.x - q * nrb;
  // lines of whole waves: the pair is wave-uniform (scalar row bases)
  const int l = (TT % 64 == 0) ? __builtin_amdgcn_readfirstlane(threadIdx.x / TT) : threadIdx.x / TT;
  const int t = threadIdx.x & (TT - 1);
  const int lbase = l * H;
  const int rp = rb * C + l;
  const bool pvalid = rp < d.Rn;
  const bool has2 = pvalid && (2 * rp + 1 < d.nrows);
  const int in_len = d.in_len;
  const int row0 = 2 * rb * C;                     // first row of the block's tile
  const int nrow_blk = d.nrows - row0 < 2 * C ? d.nrows - row0 : 2 * C;

  C2<T> va[P], vb[P];
  if constexpr (TT % 64 == 0) {
    // raw buffer loads from the rows' scalar bases: past the row length (the zero padding) and
    // for absent rows they return 0
    const T* in_a = reinterpret_cast<const T*>(d.in) + (int64_t)q * d.in_q + (int64_t)(pvalid ? 2 * rp : 0) * d.in_r;
    const T* in_b = has2 ? in_a + d.in_r : in_a;
    const BufRsrc ra = buf_rsrc(in_a, pvalid ? (uint32_t)in_len * (uint32_t)sizeof(T) : 0u);
    const BufRsrc rb_ = buf_rsrc(in_b, has2 ? (uint32_t)in_len * (uint32_t)sizeof(T) : 0u);
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const uint32_t lo = (uint32_t)t * (uint32_t)sizeof(T), so = (uint32_t)(TT * k * (int)sizeof(T));
      va[k] = mk<T>(buf_ld<T>(ra, lo, so), buf_ld<T>(rb_, lo, so));
    }
  } else {
    // several pairs per wave: one resource from the block's first row (its 2C rows lie within
    // 2 GiB of it, checked on the host), per-lane 32-bit offsets; positions past the row, absent
    // pairs and absent second rows read at an offset past the range (returns 0)
    const T* blk = reinterpret_cast<const T*>(d.in) + (int64_t)q * d.in_q + (int64_t)row0 * d.in_r;
    const BufRsrc rbk = buf_rsrc(blk, 0x7fffffffu);
    constexpr uint32_t DROP = 0x80000000u;
    const uint32_t oa = (uint32_t)(2 * l) * (uint32_t)d.in_r, ob = oa + (uint32_t)d.in_r;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int p = t + TT * k;
      const bool ok = p < in_len;
      const T a = buf_ld<T>(rbk, (ok && pvalid) ? (oa + (uint32_t)p) * (uint32_t)sizeof(T) : DROP);
      const T b = buf_ld<T>(rbk, (ok && has2) ? (ob + (uint32_t)p) * (uint32_t)sizeof(T) : DROP);
      va[k] = mk<T>(a, b);
    }
  }
  __syncthreads();   // twiddle table staged
  // rows of at most H values (checked on the host): even half x[p], odd half x[p] W_L^p
#pragma unroll
  for (int k = 0; k < P; ++k) vb[k] = cmul<T>(va[k], tw_at<T, H>(tab, t + TT * k));
  fft_line2<T, H, P, -1, 1, Cfg::WAVE>(va, vb, lds, lbase, t, tab);
  {
    // the axis' real spectrum, the same 2H values for every line (cache resident), loaded after
    // the forward transforms so that no register is held across them
    const BufRsrc rs = buf_rsrc(d.spec, (uint32_t)(2 * H) * (uint32_t)sizeof(T));
    const uint32_t lo = (uint32_t)t * (uint32_t)sizeof(T);
    T s0[P], s1[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      s0[k] = buf_ld<T>(rs, lo, (uint32_t)(TT * k) * (uint32_t)sizeof(T));
      s1[k] = buf_ld<T>(rs, lo, (uint32_t)(H + TT * k) * (uint32_t)sizeof(T));
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
      va[k] = mk<T>(va[k].x * s0[k], va[k].y * s0[k]);
      vb[k] = mk<T>(vb[k].x * s1[k], vb[k].y * s1[k]);
    }
  }
  fft_line2<T, H, P, +1, 1, Cfg::WAVE>(va, vb, lds, lbase, t, tab);

  // y[p] = ye[p] + conj(W_L^p) yo[p] for p < out_len <= H (the crop keeps the first half only);
  // Re -> row 2l, Im -> row 2l + 1 of the tile [p][row], which overlays the exchange images
  const int out_len = d.out_len;
  T* tile = reinterpret_cast<T*>(smem_raw);
  __syncthreads();   // every pair done with its exchange image
  int tt = t;
  asm volatile("" : "+v"(tt));
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const int p = tt + TT * k;
    const C2<T> y = cadd<T>(va[k], cmulc<T>(vb[k], tw_at<T, H>(tab, p)));
    if (p < out_len) {
      tile[p * PITCH + 2 * l] = y.x;
      tile[p * PITCH + 2 * l + 1] = y.y;
    }
  }
  __syncthreads();
  // out[p][row0 + row]: 2C consecutive lanes store one position's 2C rows (one contiguous
  // segment); one < 2 GiB window per RHS (checked on the host), 32-bit lane offsets.  Four
  // elements per thread are loaded before any is stored (x and y never alias).
  const int nel = out_len * 2 * C;
  const int64_t ob = (int64_t)q * d.out_q + row0;
  const BufRsrc ro = buf_rsrc(reinterpret_cast<T*>(d.out) + ob, 0x7fffffffu);
  const bool add = d.add != nullptr;                                 // uniform
  const BufRsrc rx = buf_rsrc(add ? reinterpret_cast<const T*>(d.add) + ob : nullptr, add ? 0x7fffffffu : 0u);
  const T sg = (T)d.sigma;
  for (int e0 = threadIdx.x; e0 < nel; e0 += 4 * THREADS) {
    uint32_t g[4];
    T yv[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * THREADS;
      const int ee = e < nel ? e : nel - 1;
      const int p = ee / (2 * C);
      const int row = ee - p * (2 * C);
      g[u] = (e < nel && row < nrow_blk) ? ((uint32_t)p * (uint32_t)d.out_p + (uint32_t)row) * (uint32_t)sizeof(T) : 0x80000000u;
      yv[u] = tile[p * PITCH + row];
      xv[u] = add ? buf_ld<T>(rx, g[u]) : (T)0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) buf_st<T>(add ? yv[u] + sg * xv[u] : yv[u], ro, g[u]);   // masked: past the range
  }
}

}  // namespace hgp
