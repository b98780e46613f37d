#include "nbx_registry.h"
#include "nbx_mx_batch.h"
namespace nbx {
// Batched MXFP8 block-scaled sums (nbxReduceMultiWideMxBatch): plain e5m2 sources (kind 3).
void fillMxBatchE5M2(MxBatchTable& t) { t[3] = makeMxBatchSet<TyE5M2, false>(); }
}  // namespace nbx
