#include "nbx_registry.h"
#include "nbx_mx2d.h"
namespace nbx {
// 2-D MXFP8 block-scaled sums (nbxReduceMultiWideMx2d): f16 sources (kind 0).
void fillMx2dF16(Mx2dTable& t) { t[0] = makeMx2dSet<TyF16, false>(); }
}  // namespace nbx
