// hgp_band_fused_f32.hip — instantiation + launch of the fused banded product (hgp_band_fused.hpp),
// a translation unit of its own beside hgp_band_f32.hip.
#include "hgp_band_fused.hpp"

namespace hgp {

using FusedCfg = BandFusedCfg<HGP_BAND_RMAX, HGP_BAND_FUSED_TW, HGP_BAND_FUSED_SEG>;

void band_fused_tile(int tile[2]) {
  tile[0] = FusedCfg::SEG;
  tile[1] = FusedCfg::TW;
}

hipError_t launch_band_fused(const BandFusedDesc& d, hipStream_t s) {
  using Cfg = FusedCfg;
  if (d.r0 < 0 || d.r0 > Cfg::RE || (d.r0 & 1) || d.r1 < 0 || d.r1 > Cfg::RE || (d.r1 & 1) || d.m0 < 1 || d.m1 < 1)
    return hipErrorInvalidValue;
  const int64_t nsg = (d.m0 + Cfg::SEG - 1) / Cfg::SEG;
  const int64_t ncb = (d.m1 + Cfg::TW - 1) / Cfg::TW;
  const int64_t nb = (int64_t)d.Q * nsg * ncb;
  if (nb <= 0) return hipSuccess;
  if (nb > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_band_fused<HGP_BAND_RMAX, HGP_BAND_FUSED_TW, HGP_BAND_FUSED_SEG>), dim3((unsigned)nb),
                     dim3(Cfg::THREADS), 0, s, d);
  return hipGetLastError();
}

}  // namespace hgp
