#include "nbx_registry.h"
#include "nbx_wide.h"
namespace nbx {
// Realigning fp32-accumulating sums (kWideShiftedLds), fp8 sources:
// e4m3 = 10, e5m2 = 11.
void fillWideShift8(WideTable& t) {
  addWideShifted<TyE4M3>(t[10]);
  addWideShifted<TyE5M2>(t[11]);
}
}  // namespace nbx
