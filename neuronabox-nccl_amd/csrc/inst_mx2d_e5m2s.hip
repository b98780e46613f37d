#include "nbx_registry.h"
#include "nbx_mx2d.h"
namespace nbx {
// 2-D MXFP8 block-scaled sums (nbxReduceMultiWideMx2d): e5m2 sources with block scales (kind 5).
void fillMx2dE5M2Scaled(Mx2dTable& t) { t[5] = makeMx2dSet<TyE5M2, true>(); }
}  // namespace nbx
