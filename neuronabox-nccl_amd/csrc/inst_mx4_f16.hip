#include "nbx_registry.h"
#include "nbx_mx4.h"
namespace nbx {
// MXFP4 block-scaled sums (nbxReduceMultiWideMx): plain f16 sources (kind 6).
void fillMx4F16(MxTable& t) { t[6] = makeMx4Set<Mx4Src16<TyF16>>(); }
}  // namespace nbx
