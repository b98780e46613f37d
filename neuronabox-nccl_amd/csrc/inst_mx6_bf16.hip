#include "nbx_registry.h"
#include "nbx_mx6.h"
namespace nbx {
// MXFP6 block-scaled sums (nbxReduceMultiWideMx): plain bf16 sources (kind 10).
void fillMx6BF16(MxTable& t) { t[10] = makeMx6Set<Mx4Src16<TyBF16>>(); }
}  // namespace nbx
