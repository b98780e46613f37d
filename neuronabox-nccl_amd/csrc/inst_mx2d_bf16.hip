#include "nbx_registry.h"
#include "nbx_mx2d.h"
namespace nbx {
// 2-D MXFP8 block-scaled sums (nbxReduceMultiWideMx2d): bf16 sources (kind 1).
void fillMx2dBF16(Mx2dTable& t) { t[1] = makeMx2dSet<TyBF16, false>(); }
}  // namespace nbx
