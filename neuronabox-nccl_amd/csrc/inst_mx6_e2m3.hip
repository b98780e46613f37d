#include "nbx_registry.h"
#include "nbx_mx6.h"
namespace nbx {
// MXFP6 block-scaled sums (nbxReduceMultiWideMx): E2M3 sources (kind 11), which also store fp32.
void fillMx6E2M3(MxTable& t) { t[11] = makeMx6Set<Mx6SrcFp6<Mx6E2M3>>(); }
}  // namespace nbx
