#include "nbx_registry.h"
#include "nbx_mx4.h"
namespace nbx {
// MXFP4 block-scaled sums (nbxReduceMultiWideMx): plain bf16 sources (kind 7).
void fillMx4BF16(MxTable& t) { t[7] = makeMx4Set<Mx4Src16<TyBF16>>(); }
}  // namespace nbx
