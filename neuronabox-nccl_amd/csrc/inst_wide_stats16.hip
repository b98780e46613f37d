#include "nbx_registry.h"
#include "nbx_wide.h"
namespace nbx {
// STATS forms of the pack, element and batch kernels (nbxReduceMultiWideStats),
// 16-bit sources: f16 = 6, bf16 = 9. Workgroups per CU as in inst_wide.hip.
void fillWideStats16(WideStatsTable& t) {
  t[6] = makeWideStatsSet<TyF16>(2);
  t[9] = makeWideStatsSet<TyBF16>(2);
}
}  // namespace nbx
