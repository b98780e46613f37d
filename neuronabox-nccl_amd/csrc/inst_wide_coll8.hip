#include "nbx_registry.h"
#include "nbx_wide_coll.h"
namespace nbx {
// the collectives' fp32-accumulating kernels, fp8: e4m3 = 10, e5m2 = 11
void fillWideColl8(WideCollTable& t) {
  t[10] = makeWideCollSet<TyE4M3>();
  t[11] = makeWideCollSet<TyE5M2>();
}
}  // namespace nbx
