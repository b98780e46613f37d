#include "nbx_registry.h"
#include "nbx_mx_batch.h"
namespace nbx {
// Batched MXFP8 block-scaled sums (nbxReduceMultiWideMxBatch): plain f16 sources (kind 0).
void fillMxBatchF16(MxBatchTable& t) { t[0] = makeMxBatchSet<TyF16, false>(); }
}  // namespace nbx
