#include "nbx_registry.h"
#include "nbx_mx.h"
namespace nbx {
// MXFP8 block-scaled sums (nbxReduceMultiWideMx): plain e4m3 sources (kind 2).
void fillMxE4M3(MxTable& t) { t[2] = makeMxSet<TyE4M3, false>(); }
}  // namespace nbx
