#include "nbx_registry.h"
#include "nbx_wide.h"
namespace nbx {
// STATS forms of the realigning kernels (kWideShiftedLdsStats), 16-bit
// sources: f16 = 6, bf16 = 9. Called after fillWideStats16.
void fillWideStatsShift16(WideStatsTable& t) {
  addWideShiftedStats<TyF16>(t[6]);
  addWideShiftedStats<TyBF16>(t[9]);
}
}  // namespace nbx
