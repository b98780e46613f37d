#include "nbx_registry.h"
#include "nbx_mx6.h"
namespace nbx {
// MXFP6 block-scaled sums (nbxReduceMultiWideMx): plain bf16 sources (kind 1).
void fillMx6BF16(Mx6Table& t) { t[1] = makeMx6Set<Mx4Src16<TyBF16>>(); }
}  // namespace nbx
