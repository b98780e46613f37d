#include "nbx_registry.h"
#include "nbx_mx.h"
namespace nbx {
// MXFP8 block-scaled sums (nbxReduceMultiWideMx): plain f16 sources (kind 0).
void fillMxF16(MxTable& t) { t[0] = makeMxSet<TyF16, false>(); }
}  // namespace nbx
