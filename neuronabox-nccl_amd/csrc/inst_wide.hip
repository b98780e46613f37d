#include "nbx_registry.h"
#include "nbx_wide.h"
namespace nbx {
// fp32-accumulating sums (nbxReduceMultiWide): f16 = 6, bf16 = 9, fp8 e4m3 =
// 10, e5m2 = 11. Two workgroups per CU at the unrolled tile: what the 8-source
// kernels' registers allow (194-214 VGPRs for the 16-bit types, 220-256 for fp8;
// 1 to 4 per CU measured within 0.5 %).
void fillWide(WideTable& t) {
  t[6] = makeWideSet<TyF16>(2);
  t[9] = makeWideSet<TyBF16>(2);
  t[10] = makeWideSet<TyE4M3>(2);
  t[11] = makeWideSet<TyE5M2>(2);
  fillWideShift16(t);
  fillWideShift8(t);
}
}  // namespace nbx
