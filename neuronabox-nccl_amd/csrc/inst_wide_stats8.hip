#include "nbx_registry.h"
#include "nbx_wide.h"
namespace nbx {
// STATS forms of the pack, element and batch kernels (nbxReduceMultiWideStats),
// fp8 sources: e4m3 = 10, e5m2 = 11. Workgroups per CU as in inst_wide.hip.
void fillWideStats8(WideStatsTable& t) {
  t[10] = makeWideStatsSet<TyE4M3>(2);
  t[11] = makeWideStatsSet<TyE5M2>(2);
}
}  // namespace nbx
