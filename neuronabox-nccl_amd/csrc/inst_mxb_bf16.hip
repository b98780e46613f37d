#include "nbx_registry.h"
#include "nbx_mx_batch.h"
namespace nbx {
// Batched MXFP8 block-scaled sums (nbxReduceMultiWideMxBatch): plain bf16 sources (kind 1).
void fillMxBatchBF16(MxBatchTable& t) { t[1] = makeMxBatchSet<TyBF16, false>(); }
}  // namespace nbx
