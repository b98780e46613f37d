#include "nbx_registry.h"
#include "nbx_mx2d.h"
namespace nbx {
// 2-D MXFP8 block-scaled sums (nbxReduceMultiWideMx2d): plain e4m3 sources (kind 2).
void fillMx2dE4M3(Mx2dTable& t) { t[2] = makeMx2dSet<TyE4M3, false>(); }
}  // namespace nbx
