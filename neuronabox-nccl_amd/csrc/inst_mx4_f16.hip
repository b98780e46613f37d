#include "nbx_registry.h"
#include "nbx_mx4.h"
namespace nbx {
// MXFP4 block-scaled sums (nbxReduceMultiWideMx): plain f16 sources (kind 0).
void fillMx4F16(Mx4Table& t) { t[0] = makeMx4Set<Mx4Src16<TyF16>>(); }
}  // namespace nbx
