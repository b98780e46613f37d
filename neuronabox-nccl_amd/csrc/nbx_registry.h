// nbx_registry.h — kernel table shared by the per-type instantiation units
// (inst_*.hip, compiled in parallel) and the host launchers (nbx_launch.h).
// Replaces the generated ncclDevFuncTable / ncclDevFuncId of the reference
// (/root/reference/src/device/generate.py:125-149, src/include/device.h:412-459):
// one KernelSet per (datatype, device op); signed integers share the
// unsigned kernels for Sum/Prod/MinMax/PreMulSum exactly as generate.py's
// equivalent_primary() maps them.
#pragma once
#include "nbx_kargs.h"

namespace nbx {
constexpr int kNumTypes = 12;   // ncclNumTypes (incl. fp8)
constexpr int kNumDevOps = 5;   // nbxNumDevRedOps
typedef KernelSet KernelTable[kNumTypes][kNumDevOps];

void fillInt8(KernelTable& t);
void fillInt32(KernelTable& t);
void fillInt64(KernelTable& t);
void fillF16(KernelTable& t);
void fillBF16(KernelTable& t);
void fillF32(KernelTable& t);
void fillF64(KernelTable& t);
void fillFp8(KernelTable& t);

// fp32-accumulating sums: one WideSet per source type (f16, bf16, fp8)
typedef WideSet WideTable[kNumTypes];
void fillWide(WideTable& t);
// their realigning kernels, per element width (called by fillWide)
void fillWideShift16(WideTable& t);
void fillWideShift8(WideTable& t);

// their STATS forms (nbxReduceMultiWideStats): a table of its own with the
// same indices, a unit per element width and kernel family
// (inst_wide_stats*.hip), and the two kernels that sum the slots
typedef WideSet WideStatsTable[kNumTypes];
void fillWideStats(WideStatsTable& t);   // inst_wide_stats_sum.hip; calls the four below
void fillWideStats16(WideStatsTable& t);
void fillWideStats8(WideStatsTable& t);
void fillWideStatsShift16(WideStatsTable& t);
void fillWideStatsShift8(WideStatsTable& t);
struct WideStatsKernels {
  const void* reduce;   // kWideStatsReduce
  const void* batch;    // kWideStatsBatch
};
WideStatsKernels wideStatsKernels();

// the collectives' fp32-accumulating kernels: one WideCollSet per element
// type, a unit per element width (inst_wide_coll*.hip)
typedef WideCollSet WideCollTable[kNumTypes];
void fillWideColl16(WideCollTable& t);
void fillWideColl8(WideCollTable& t);

// the block-scaled sums (nbxReduceMultiWideMx): one MxSet per source kind, a
// unit per kind. [index] kind, its outputs (MxSet::blocks' first index):
//   MXFP8 (nbx_mx.h, inst_mx_*.hip), outputs 0 e4m3, 1 e5m2, 2 fp32 (scaled kinds only)
//     [0] f16  [1] bf16  [2] e4m3  [3] e5m2 plain   [4] e4m3  [5] e5m2 with scales
//   MXFP4 (NBX_FLOAT4_E2M1, nbx_mx4.h, inst_mx4_*.hip), outputs 0 MXFP4, 1 fp32 (MXFP4 sources only)
//     [6] f16  [7] bf16 plain   [8] MXFP4
//   MXFP6 (NBX_FLOAT6_E2M3 / NBX_FLOAT6_E3M2, nbx_mx6.h, inst_mx6_*.hip), outputs of the
//   plain kinds 0 E2M3, 1 E3M2, of the MXFP6 kinds 0 their own type, 1 fp32
//     [9] f16  [10] bf16 plain   [11] E2M3  [12] E3M2
// The host's view of the same rows is nbx_reduce_mx.cc's format table.
typedef MxSet MxTable[kMxKinds];
void fillMxF16(MxTable& t);
void fillMxBF16(MxTable& t);
void fillMxE4M3(MxTable& t);
void fillMxE5M2(MxTable& t);
void fillMxE4M3Scaled(MxTable& t);
void fillMxE5M2Scaled(MxTable& t);
void fillMx4F16(MxTable& t);
void fillMx4BF16(MxTable& t);
void fillMx4Fp4(MxTable& t);
void fillMx6F16(MxTable& t);
void fillMx6BF16(MxTable& t);
void fillMx6E2M3(MxTable& t);
void fillMx6E3M2(MxTable& t);

// the MXFP8 kinds' work-list batch (nbxReduceMultiWideMxBatch, nbx_mx_batch.h):
// one MxBatchSet per kind, MxTable's first six indices, a unit per kind (inst_mxb_*.hip)
typedef MxBatchSet MxBatchTable[kMxFp8Kinds];
void fillMxBatchF16(MxBatchTable& t);
void fillMxBatchBF16(MxBatchTable& t);
void fillMxBatchE4M3(MxBatchTable& t);
void fillMxBatchE5M2(MxBatchTable& t);
void fillMxBatchE4M3Scaled(MxBatchTable& t);
void fillMxBatchE5M2Scaled(MxBatchTable& t);

// the MXFP8 kinds' 2-D form (nbxReduceMultiWideMx2d, nbx_mx2d.h): one Mx2dSet
// per kind, the same six indices, a unit per kind (inst_mx2d_*.hip)
typedef Mx2dSet Mx2dTable[kMxFp8Kinds];
void fillMx2dF16(Mx2dTable& t);
void fillMx2dBF16(Mx2dTable& t);
void fillMx2dE4M3(Mx2dTable& t);
void fillMx2dE5M2(Mx2dTable& t);
void fillMx2dE4M3Scaled(Mx2dTable& t);
void fillMx2dE5M2Scaled(Mx2dTable& t);
}  // namespace nbx
