#include "nbx_registry.h"
#include "nbx_mx2d.h"
namespace nbx {
// 2-D MXFP8 block-scaled sums (nbxReduceMultiWideMx2d): e4m3 sources with block scales (kind 4).
void fillMx2dE4M3Scaled(Mx2dTable& t) { t[4] = makeMx2dSet<TyE4M3, true>(); }
}  // namespace nbx
