#include "nbx_registry.h"
#include "nbx_mx4.h"
namespace nbx {
// MXFP4 block-scaled sums (nbxReduceMultiWideMx): plain bf16 sources (kind 1).
void fillMx4BF16(Mx4Table& t) { t[1] = makeMx4Set<Mx4Src16<TyBF16>>(); }
}  // namespace nbx
