#include "nbx_registry.h"
#include "nbx_mx4.h"
namespace nbx {
// MXFP4 block-scaled sums (nbxReduceMultiWideMx): MXFP4 sources (kind 2), which also store fp32.
void fillMx4Fp4(Mx4Table& t) { t[2] = makeMx4Set<Mx4SrcFp4>(); }
}  // namespace nbx
