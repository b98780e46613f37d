#include "nbx_registry.h"
#include "nbx_mx6.h"
namespace nbx {
// MXFP6 block-scaled sums (nbxReduceMultiWideMx): plain f16 sources (kind 9).
void fillMx6F16(MxTable& t) { t[9] = makeMx6Set<Mx4Src16<TyF16>>(); }
}  // namespace nbx
