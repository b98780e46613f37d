#include "nbx_registry.h"
#include "nbx_wide.h"
namespace nbx {
// STATS forms of the realigning kernels (kWideShiftedLdsStats), fp8 sources:
// e4m3 = 10, e5m2 = 11. Called after fillWideStats8.
void fillWideStatsShift8(WideStatsTable& t) {
  addWideShiftedStats<TyE4M3>(t[10]);
  addWideShiftedStats<TyE5M2>(t[11]);
}
}  // namespace nbx
