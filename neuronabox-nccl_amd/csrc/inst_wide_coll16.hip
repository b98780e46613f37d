#include "nbx_registry.h"
#include "nbx_wide_coll.h"
namespace nbx {
// the collectives' fp32-accumulating kernels, 16-bit types: f16 = 6, bf16 = 9
void fillWideColl16(WideCollTable& t) {
  t[6] = makeWideCollSet<TyF16>();
  t[9] = makeWideCollSet<TyBF16>();
}
}  // namespace nbx
