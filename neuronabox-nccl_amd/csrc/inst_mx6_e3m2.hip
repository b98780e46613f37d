#include "nbx_registry.h"
#include "nbx_mx6.h"
namespace nbx {
// MXFP6 block-scaled sums (nbxReduceMultiWideMx): E3M2 sources (kind 12), which also store fp32.
void fillMx6E3M2(MxTable& t) { t[12] = makeMx6Set<Mx6SrcFp6<Mx6E3M2>>(); }
}  // namespace nbx
