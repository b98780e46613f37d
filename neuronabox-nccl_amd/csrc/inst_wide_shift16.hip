#include "nbx_registry.h"
#include "nbx_wide.h"
namespace nbx {
// Realigning fp32-accumulating sums (kWideShiftedLds), 16-bit sources:
// f16 = 6, bf16 = 9.
void fillWideShift16(WideTable& t) {
  addWideShifted<TyF16>(t[6]);
  addWideShifted<TyBF16>(t[9]);
}
}  // namespace nbx
