#include "nbx_registry.h"
#include "nbx_mx.h"
namespace nbx {
// MXFP8 block-scaled sums (nbxReduceMultiWideMx): e4m3 sources with block scales (kind 4), which also store fp32.
void fillMxE4M3Scaled(MxTable& t) { t[4] = makeMxSet<TyE4M3, true>(); }
}  // namespace nbx
