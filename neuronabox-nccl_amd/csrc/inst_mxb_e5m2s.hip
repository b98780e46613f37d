#include "nbx_registry.h"
#include "nbx_mx_batch.h"
namespace nbx {
// Batched MXFP8 block-scaled sums (nbxReduceMultiWideMxBatch): e5m2 sources with block scales, which also store fp32 (kind 5).
void fillMxBatchE5M2Scaled(MxBatchTable& t) { t[5] = makeMxBatchSet<TyE5M2, true>(); }
}  // namespace nbx
