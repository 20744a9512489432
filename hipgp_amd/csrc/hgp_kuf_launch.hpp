// hgp_kuf_launch.hpp — the host side that the product kernels of the Kuf / RFF family share
// (hgp_kuf_mv.hip, hgp_kuf_rmv.hip, hgp_kuf_win.hip, hgp_kuf_line_win.hip, hgp_rff.hip): the CU
// count, the widths of the row groups, the grid descriptor, the run-time -> compile-time ladders
// and the loop over the row groups with its optional fp64 partials.  Host only.
//
// A launcher is one generic lambda with one launch line:
//   kuf_with_kind(kind, [&](auto K) {
//     kuf_with_width(NW, [&](auto W) {
//       hipLaunchKernelGGL((k<T, decltype(K)::value, decltype(W)::value>), ...);
//     });
//   });
// Each ladder calls the lambda once per value it can take, so exactly those kernels exist.
//
// What stays with each product: its split policy (how many slices, of what) and the check of its
// grid size against 2^31 - 1, whose operands differ from product to product.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "hgp_internal.hpp"   // KufObs
#include "hgp_kuf_eval.hpp"

namespace hgp {

// CUs of the current device, asked once per device
inline int kuf_cus(hipError_t* e) {
  static int cus[64] = {0};
  int dev = 0;
  *e = hipGetDevice(&dev);
  if (*e != hipSuccess) return 0;
  if (dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int v = 0;
    *e = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
    if (*e != hipSuccess) return 0;
    cus[dev] = v > 0 ? v : 256;
  }
  return cus[dev];
}

// the width of the next group of weight / coefficient rows when rem are left
inline int kuf_group(int64_t rem) { return rem >= 5 ? 8 : (rem >= 2 ? 4 : 1); }

// g from the caller's arrays; *M mesh points, *outer = *M / m[ndim - 1] rows of the last axis
// (either may be null where the caller has no use for it)
inline void kuf_fill_grid(KufGrid& g, int ndim, const int64_t* m, const void* const* grids, int64_t* M = nullptr,
                          int64_t* outer = nullptr) {
  g.d = ndim;
  int64_t all = 1, rows = 1;
  for (int a = 0; a < ndim; ++a) {
    g.m[a] = m[a];
    g.g[a] = grids[a];
    all *= m[a];
    if (a < ndim - 1) rows *= m[a];
  }
  if (M != nullptr) *M = all;
  if (outer != nullptr) *outer = rows;
}

template <int V>
using KufConst = std::integral_constant<int, V>;

// f(T{}) for the tensor dtype T: what is left of a launcher's dtype wrapper
template <typename F>
inline hipError_t kuf_with_dtype(int dtype, F&& f) {
  return dtype == HGP_F32 ? f(float{}) : f(double{});
}

// f(KufConst<NW>{}) for the group width NW in {8, 4, 1}
template <typename F>
inline void kuf_with_width(int NW, F&& f) {
  if (NW == 8)
    f(KufConst<8>{});
  else if (NW == 4)
    f(KufConst<4>{});
  else
    f(KufConst<1>{});
}

// f(KufConst<kind>{}) for the four kernels of the point products
template <typename F>
inline void kuf_with_kind(int kind, F&& f) {
  switch (kind) {
    case HGP_KERN_SQEXP: f(KufConst<HGP_KERN_SQEXP>{}); break;
    case HGP_KERN_MATERN12: f(KufConst<HGP_KERN_MATERN12>{}); break;
    case HGP_KERN_MATERN32: f(KufConst<HGP_KERN_MATERN32>{}); break;
    default: f(KufConst<HGP_KERN_MATERN52>{});
  }
}

// f(KufConst<mode>{}) for the line integral: 1 Monte-Carlo, 2 (and anything else) analytic SqExp
template <typename F>
inline void kuf_with_mode(int mode, F&& f) {
  if (mode == 1)
    f(KufConst<1>{});
  else
    f(KufConst<2>{});
}

// f(KufConst<D>{}) for the number of axes: 1, 2, 3 (and anything else)
template <typename F>
inline void kuf_with_dim(int ndim, F&& f) {
  if (ndim == 1)
    f(KufConst<1>{});
  else if (ndim == 2)
    f(KufConst<2>{});
  else
    f(KufConst<3>{});
}

// The n weight / coefficient rows in groups: launch(s0, NW, nv, part) for the group that starts at
// row s0, NW = kuf_group(n - s0) slots wide with nv <= NW of them in use.  part_per_slot > 0: the
// product is split, `part` holds part_per_slot fp64 partial sums for each of kuf_group(n) slots
// (the widest group is the first), and finish(s0, NW, nv, part) adds a group's up after its launch.
// part_per_slot == 0: part == nullptr and finish is not called.  The launches' error first, then
// that of the release.
template <typename L, typename F>
inline hipError_t kuf_row_groups(int64_t n, size_t part_per_slot, hipStream_t s, L&& launch, F&& finish) {
  double* part = nullptr;
  if (part_per_slot > 0) {
    const hipError_t e =
        hipMallocAsync(reinterpret_cast<void**>(&part), part_per_slot * (size_t)kuf_group(n) * sizeof(double), s);
    if (e != hipSuccess) return e;
  }
  for (int64_t s0 = 0, nv = 0; s0 < n; s0 += nv) {
    const int NW = kuf_group(n - s0);
    nv = n - s0 < NW ? n - s0 : NW;
    launch(s0, NW, (int)nv, part);
    if (part != nullptr) finish(s0, NW, (int)nv, part);
  }
  hipError_t e = hipGetLastError();
  if (part != nullptr) {
    const hipError_t f = hipFreeAsync(part, s);
    if (e == hipSuccess) e = f;
  }
  return e;
}

// a product that is never split
template <typename L>
inline hipError_t kuf_row_groups(int64_t n, hipStream_t s, L&& launch) {
  return kuf_row_groups(n, 0, s, std::forward<L>(launch), [](int64_t, int, int, double*) {});
}

}  // namespace hgp
