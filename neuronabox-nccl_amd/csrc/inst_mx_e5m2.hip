#include "nbx_registry.h"
#include "nbx_mx.h"
namespace nbx {
// MXFP8 block-scaled sums (nbxReduceMultiWideMx): plain e5m2 sources (kind 3).
void fillMxE5M2(MxTable& t) { t[3] = makeMxSet<TyE5M2, false>(); }
}  // namespace nbx
