#include "nbx_registry.h"
#include "nbx_mx4.h"
namespace nbx {
// MXFP4 block-scaled sums (nbxReduceMultiWideMx): MXFP4 sources (kind 8), which also store fp32.
void fillMx4Fp4(MxTable& t) { t[8] = makeMx4Set<Mx4SrcFp4>(); }
}  // namespace nbx
