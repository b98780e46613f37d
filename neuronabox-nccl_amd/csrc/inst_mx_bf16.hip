#include "nbx_registry.h"
#include "nbx_mx.h"
namespace nbx {
// MXFP8 block-scaled sums (nbxReduceMultiWideMx): plain bf16 sources (kind 1).
void fillMxBF16(MxTable& t) { t[1] = makeMxSet<TyBF16, false>(); }
}  // namespace nbx
