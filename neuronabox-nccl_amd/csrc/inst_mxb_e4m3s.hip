#include "nbx_registry.h"
#include "nbx_mx_batch.h"
namespace nbx {
// Batched MXFP8 block-scaled sums (nbxReduceMultiWideMxBatch): e4m3 sources with block scales, which also store fp32 (kind 4).
void fillMxBatchE4M3Scaled(MxBatchTable& t) { t[4] = makeMxBatchSet<TyE4M3, true>(); }
}  // namespace nbx
