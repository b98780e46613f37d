#include "nbx_registry.h"
#include "nbx_mx.h"
namespace nbx {
// MXFP8 block-scaled sums (nbxReduceMultiWideMx): e5m2 sources with block scales (kind 5), which also store fp32.
void fillMxE5M2Scaled(MxTable& t) { t[5] = makeMxSet<TyE5M2, true>(); }
}  // namespace nbx
