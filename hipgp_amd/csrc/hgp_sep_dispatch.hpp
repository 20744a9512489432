// hgp_sep_dispatch.hpp — instantiation + launch of k_sep_pass for one dtype (included by
// hgp_sep_f32.hip / hgp_sep_f64.hip, translation units of their own so they compile beside the
// pass ones).
#pragma once
#include "hgp_internal.hpp"
#include "hgp_sep.hpp"

namespace hgp {

// power-of-two half-lengths the fp64 set-up passes also hold (the K op's L_K / 2 <= 8192)
#define HGP_SEP_SWITCH(FN, ...)                                                                      \
  switch (H) {                                                                                       \
    case 2: return FN<T, 2>(__VA_ARGS__);       case 4: return FN<T, 4>(__VA_ARGS__);               \
    case 8: return FN<T, 8>(__VA_ARGS__);       case 16: return FN<T, 16>(__VA_ARGS__);             \
    case 32: return FN<T, 32>(__VA_ARGS__);     case 64: return FN<T, 64>(__VA_ARGS__);             \
    case 128: return FN<T, 128>(__VA_ARGS__);   case 256: return FN<T, 256>(__VA_ARGS__);           \
    case 512: return FN<T, 512>(__VA_ARGS__);   case 1024: return FN<T, 1024>(__VA_ARGS__);         \
    case 2048: return FN<T, 2048>(__VA_ARGS__); case 4096: return FN<T, 4096>(__VA_ARGS__);         \
    case 8192: return FN<T, 8192>(__VA_ARGS__);                                                      \
    default: break;                                                                                  \
  }

template <typename T, int H>
static int sep_pairs_h() { return SepCfg<T, H>::FITS ? SepCfg<T, H>::C : 0; }

template <typename T, int H>
static hipError_t launch_sep_h(const SepDesc& d, hipStream_t s) {
  using Cfg = SepCfg<T, H>;
  if constexpr (!Cfg::FITS) {
    return hipErrorNotSupported;
  } else {
    const int64_t nb = (int64_t)d.Q * ((d.Rn + Cfg::C - 1) / Cfg::C);
    if (nb <= 0) return hipSuccess;
    if (nb > 0x7fffffff) return hipErrorInvalidValue;
    static bool attr_set = false;   // opt in to > 64 KB dynamic LDS once per instance
    if (!attr_set) {
      hipError_t e = hipFuncSetAttribute((const void*)k_sep_pass<T, H>, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS);
      if (e != hipSuccess) return e;
      attr_set = true;
    }
    hipLaunchKernelGGL((k_sep_pass<T, H>), dim3((unsigned)nb), dim3(Cfg::THREADS), Cfg::LDS, s, d);
    return hipGetLastError();
  }
}

template <typename T>
int sep_pairs(int H) {
  HGP_SEP_SWITCH(sep_pairs_h)
  return 0;
}

template <typename T>
hipError_t launch_sep(int H, const SepDesc& d, hipStream_t s) {
  HGP_SEP_SWITCH(launch_sep_h, d, s)
  return hipErrorNotSupported;
}

}  // namespace hgp
