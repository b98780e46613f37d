#include "nbx_registry.h"
#include "nbx_mx_batch.h"
namespace nbx {
// Batched MXFP8 block-scaled sums (nbxReduceMultiWideMxBatch): plain e4m3 sources (kind 2).
void fillMxBatchE4M3(MxBatchTable& t) { t[2] = makeMxBatchSet<TyE4M3, false>(); }
}  // namespace nbx
