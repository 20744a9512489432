// hgp_band_f32.hip — instantiation + launch of the banded product-form passes (hgp_band.hpp), a
// translation unit of its own so that it compiles beside the pass ones.
#include "hgp_band.hpp"

namespace hgp {

hipError_t launch_band(int axis, const BandDesc& d, hipStream_t s) {
  using Cfg = BandCfg<HGP_BAND_RMAX>;
  if (d.r < 0 || d.r > Cfg::RE || (d.r & 1) || d.m0 < 1 || d.m1 < 1) return hipErrorInvalidValue;
  const int64_t nrb = axis == 1 ? (d.m0 + 15) / 16 : (d.m0 + Cfg::TH - 1) / Cfg::TH;
  const int64_t ncb = axis == 1 ? (d.m1 + Cfg::TW - 1) / Cfg::TW : (d.m1 + 31) / 32;
  const int64_t nb = (int64_t)d.Q * nrb * ncb;
  if (nb <= 0) return hipSuccess;
  if (nb > 0x7fffffff) return hipErrorInvalidValue;
  if (axis == 1)
    hipLaunchKernelGGL((k_band_row<HGP_BAND_RMAX>), dim3((unsigned)nb), dim3(Cfg::THREADS), 0, s, d);
  else
    hipLaunchKernelGGL((k_band_col<HGP_BAND_RMAX>), dim3((unsigned)nb), dim3(Cfg::THREADS), 0, s, d);
  return hipGetLastError();
}

}  // namespace hgp
