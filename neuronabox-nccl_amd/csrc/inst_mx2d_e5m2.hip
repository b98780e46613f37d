#include "nbx_registry.h"
#include "nbx_mx2d.h"
namespace nbx {
// 2-D MXFP8 block-scaled sums (nbxReduceMultiWideMx2d): plain e5m2 sources (kind 3).
void fillMx2dE5M2(Mx2dTable& t) { t[3] = makeMx2dSet<TyE5M2, false>(); }
}  // namespace nbx
