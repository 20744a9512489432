// hgp_sep_host.hpp — host-side set-up of the product-form K matvec: the test whether
// a 2-D Toeplitz column is a product of two 1-D ones plus a jitter, and the 1-D operator spectra.
// Plain C++ in fp64, no device code.
#pragma once
#include <cmath>
#include <complex>
#include <cstdint>
#include <limits>
#include <vector>

namespace hgp {

// acceptance bound of sep_detect in units of the column's storage rounding (2^-24 fp32, 2^-53
// fp64) relative to max |c|.  Largest residual measured over the SqExp columns of the tests and
// the benchmark: 2.2 units (DESIGN §20 lists them); a Matern-3/2 column misses by > 1e5 units.
#ifndef HGP_SEP_ACCEPT
#define HGP_SEP_ACCEPT 4.0
#endif

struct SepFactors {
  bool ok = false;
  double k00 = 0, sigma = 0;
  double resid = 0;                 // max |c[i][j] - t0[i] t1[j]| / max |c|, corner excluded
  std::vector<double> t0, t1;       // factor columns, t0[0] t1[0] = k00
};

// c: the m0 x m1 Toeplitz column (row-major, the jitter already on c[0]); eps: the rounding unit
// of the dtype it was stored in.  With u = c[:, 0], v = c[0, :] and k00 = u[i] v[j] / c[i][j] at
// the largest off-corner entry (i, j >= 1; it must be far above the smallest normal number, so
// that underflowed entries never enter the estimate): t0 = u, t1 = v / k00 with t0[0] = k00,
// t1[0] = 1, sigma = c[0][0] - k00.  Accepted when the residual is within HGP_SEP_ACCEPT eps and
// sigma is not negative beyond the same bound.
//
// The acceptance test on the scan's results (shared with the device scan, hgp_kernels.hip
// sep_detect_dev): best = the largest off-corner |c|, rmax = the largest absolute residual
inline bool sep_accept(double cmax, double best, double k00, double sigma, double rmax, double eps, double tiny) {
  const double big = std::numeric_limits<double>::max();
  if (!(cmax > 0) || !(cmax <= big)) return false;                  // empty, NaN or inf
  if (!(best > tiny * 1099511627776.0)) return false;               // 2^40 above the smallest normal
  if (!(k00 > 0) || !(k00 <= big)) return false;
  const double bound = HGP_SEP_ACCEPT * eps;
  return rmax / cmax <= bound && sigma >= -bound * cmax;
}

// rounding unit / smallest normal number of the dtype a column is stored in (0: fp32, 1: fp64)
inline double sep_eps(int dtype) { return dtype == 0 ? 5.9604644775390625e-08 : 1.1102230246251565e-16; }
inline double sep_tiny(int dtype) { return dtype == 0 ? 1.1754943508222875e-38 : 2.2250738585072014e-308; }

inline SepFactors sep_detect(const double* c, int64_t m0, int64_t m1, double eps, double tiny) {
  SepFactors f;
  if (m0 < 2 || m1 < 2) return f;
  double cmax = 0, best = 0;
  int64_t bi = 0, bj = 0;
  for (int64_t i = 0; i < m0; ++i)
    for (int64_t j = 0; j < m1; ++j) {
      const double a = std::fabs(c[i * m1 + j]);
      if (!(a <= std::numeric_limits<double>::max())) return f;   // NaN / inf
      if (a > cmax) cmax = a;
      if (i >= 1 && j >= 1 && a > best) { best = a; bi = i; bj = j; }
    }
  if (!(best > 0)) return f;
  const double k00 = c[bi * m1] * c[bj] / c[bi * m1 + bj];
  if (!(k00 > 0) || !(k00 <= std::numeric_limits<double>::max())) return f;
  f.k00 = k00;
  f.sigma = c[0] - k00;
  f.t0.resize(m0);
  f.t1.resize(m1);
  for (int64_t i = 0; i < m0; ++i) f.t0[i] = c[i * m1];
  for (int64_t j = 0; j < m1; ++j) f.t1[j] = c[j] / k00;
  f.t0[0] = k00;
  f.t1[0] = 1.0;
  double r = 0;
  for (int64_t i = 0; i < m0; ++i)
    for (int64_t j = (i == 0 ? 1 : 0); j < m1; ++j) {
      const double e = std::fabs(c[i * m1 + j] - f.t0[i] * f.t1[j]);
      if (e > r) r = e;
    }
  f.resid = r / cmax;
  f.ok = sep_accept(cmax, best, k00, f.sigma, r, eps, tiny);
  return f;
}

// Tap radius of a factor column t (m values) for the banded passes (hgp_band.hpp): the
// smallest r with 2 sum_{j > r} |t[j]| <= 2^-25 (|t[0]| + 2 sum_{j >= 1} |t[j]|), i.e. the taps
// beyond r hold at most half an fp32 rounding unit of the Toeplitz matrix' row sum.  Dropping them
// on both axes changes K x by at most 2^-24 ||t0||_1 ||t1||_1 max |x|.  Sums run from the small
// end; a NaN keeps every tap (r = m - 1).
inline int64_t band_radius(const double* t, int64_t m) {
  if (m < 1) return 0;
  double total = 0;
  for (int64_t j = m - 1; j >= 1; --j) total += 2.0 * std::fabs(t[j]);
  total += std::fabs(t[0]);
  const double bound = 2.98023223876953125e-08 * total;            // 2^-25
  double tail = 0;
  int64_t r = m - 1;
  while (r > 0 && 2.0 * (tail + std::fabs(t[r])) <= bound) { tail += std::fabs(t[r]); --r; }
  return r;
}

// in-place radix-2 FFT (forward sign), n a power of two
inline void sep_fft(std::vector<std::complex<double>>& a) {
  const size_t n = a.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  const double pi = 3.14159265358979323846264338327950288;
  std::vector<std::complex<double>> w(n / 2 > 0 ? n / 2 : 1);       // W_n^k, every level strides through it
  for (size_t k = 0; k < n / 2; ++k) w[k] = std::polar(1.0, -2.0 * pi * (double)k / (double)n);
  for (size_t len = 2; len <= n; len <<= 1) {
    const size_t step = n / len;
    for (size_t i = 0; i < n; i += len)
      for (size_t k = 0; k < len / 2; ++k) {
        const std::complex<double> u = a[i + k], v = a[i + k + len / 2] * w[k * step];
        a[i + k] = u + v;
        a[i + k + len / 2] = u - v;
      }
  }
}

// Spectrum of the symmetric Toeplitz matrix of column t (m values) embedded evenly in a circulant
// of L >= 2m - 1 points (a power of two): real and even.  Returned with the inverse transform's
// 1 / L and in the order the passes hold a line's frequencies: index half * L/2 + k = frequency
// 2k + half (hgp_fft.hpp).
inline std::vector<double> sep_spectrum(const std::vector<double>& t, int64_t L) {
  const int64_t m = (int64_t)t.size();
  std::vector<std::complex<double>> e((size_t)L, 0.0);
  e[0] = t[0];
  for (int64_t j = 1; j < m; ++j) { e[(size_t)j] = t[(size_t)j]; e[(size_t)(L - j)] = t[(size_t)j]; }
  sep_fft(e);
  std::vector<double> s((size_t)L);
  const int64_t H = L / 2;
  for (int64_t k = 0; k < H; ++k) {
    s[(size_t)k] = e[(size_t)(2 * k)].real() / (double)L;
    s[(size_t)(H + k)] = e[(size_t)(2 * k + 1)].real() / (double)L;
  }
  return s;
}

}  // namespace hgp
