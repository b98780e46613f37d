// nbx_kargs.h — kernel argument block and launch-table entry, shared by the
// device instantiation units and the host launcher (no device code here, so
// host .cc files compile as plain C++).
#pragma once
#include <stdint.h>

namespace nbx {

constexpr int kBlock = 256;      // workgroup = 4 wave64
constexpr int kMaxKSrcs = 8;     // sources per kernel pass
// realigning kernel (kReduceShiftedLds): waves per workgroup, packs per lane
// per tile (2 from 3 sources, else 1) and workgroups per CU (1 from 3 sources,
// else 2) — profiles/r2/sweep_shift_256MiB_r2f.txt
constexpr int kShiftLdsWaves = 4;
constexpr int kShiftLdsStages = 2;
constexpr int shiftLdsUnroll(int nSrcs) { return nSrcs >= 3 ? 2 : 1; }
constexpr int shiftLdsBlocksPerCU(int nSrcs) { return nSrcs >= 3 ? 1 : 2; }
// its dynamic schedule: wave tiles in kShiftDynClasses classes (t mod C), one
// counter per class kShiftDynStride words apart (KArgs.dynCtr -> the first)
constexpr int kShiftDynClasses = 32;
constexpr int kShiftDynStride = 64;
constexpr int kMaxKDsts = 8;     // destinations: NCCL_MAX_DIRECT_ARITY + 1 (device.h:147, all_reduce.h:343-360)

struct KArgs {
  const void* src[kMaxKSrcs];
  void* dst[kMaxKDsts];
  uint64_t nElts;     // total elements
  uint64_t nPacks;    // 16-B packs in the aligned body (starts at headElts)
  uint64_t arg;       // ncclDevRedOpFull.scalarArg (by value)
  const void* argPtr; // device scalar (ncclScalarDevice) or nullptr
  uint32_t preMask;   // bit s set: apply the PreMulSum pre-op to source s
  int32_t nSrcs;
  int32_t nDsts;
  int32_t postOp;
  int32_t headElts;   // elements before the 16-B aligned body
  int32_t variant;    // 0 = small tile (U = 1), 1 = big tile
  int32_t acquireSystem;  // 1: system-scope acquire at kernel start (sources include peer GPU memory)
  // dynamic tiles (dynCtr != nullptr): tiles past the first gridDim.x come
  // from a per-stream counter that every launch on that stream advances by
  // exactly its tile count; this launch's tiles are counter - dynBase
  uint32_t* dynCtr;
  uint32_t dynBase;
  int32_t pad;
};

// Batched reduce (nbxReduceMultiBatch): several independent buckets with the
// same functor and source count in one launch — the analogue of NCCL packing
// grouped collectives into one ncclWork (enqueue.cc:67-91 appendWorkElemColl,
// up to NCCL_MAX_WORK_ELEMENTS = 9 elements, device.h:230). Every bucket's
// pointers share one alignment modulo 16. The bucket table travels in the
// kernel-argument segment (4 KiB, read with scalar loads), packed with
// variable-length records so a launch holds 46 (8 sources) to 101 (2 sources)
// single-destination buckets:
//   w[o]          tileEnd: running total of tiles through this bucket
//   w[o+1]        nElts | headElts << 56 | nDsts << 60
//   w[o+2 ..]     NSRC source pointers, then nDsts destination pointers
constexpr int kBatchTilePacks = 256;   // one 16-B pack per lane per tile (kBlock lanes)
constexpr int kBatchHeaderBytes = 40;
constexpr int kBatchWords = (4096 - kBatchHeaderBytes) / 8;
constexpr uint64_t kBatchCountMask = (1ull << 56) - 1;
// up to this many buckets of one source count (fitting one table) use the
// kernel-argument form even when work lists are on (profiles/r2/batch_list_*)
constexpr int kBatchKernargMaxBuckets = 16;

struct BatchArgs {
  uint64_t arg;
  const void* argPtr;
  uint64_t totalTiles;
  uint32_t preMask;
  int32_t postOp;
  int32_t nTasks;
  int32_t acquireSystem;
  uint64_t w[kBatchWords];
};

// Work-list form of the batch (kReduceBatchList): the bucket records live in a
// table outside the kernel arguments (NCCL's work FIFO, enqueue.cc:759
// uploadWork / common.h:146-176), so one launch takes up to kListMaxRecs
// buckets (and a call any number, in as many launches). The host writes the
// table straight into uncached device memory through the large BAR (pinned
// host memory where the BAR is small). Records of recWords = 3 + nSrcs +
// (the launch's largest nDsts) words: tileBegin, tileEnd, count | head << 56 |
// nDsts << 60, the sources, the destinations — at most kBatchRecWords; sized
// to the launch because every record crosses PCIe (a 2-source bucket's is 48 B
// instead of 160 B). The records' running tile totals also
// travel in the kernel arguments (scalar-cache hits, fresh every launch):
// workgroups take chunks of `chunk` consecutive tiles round-robin (chunk 1 =
// grid stride, the whole GPU on one window of memory, as for one bucket), and
// a wave finds the record of a tile by comparing 64 tile totals at once
// (ballot), so skipping many small buckets costs one step, not one per record.
constexpr int kBatchRecWords = 20;
constexpr int kListMaxRecs = 384;
constexpr int kBatchListSlotBytes = kListMaxRecs * kBatchRecWords * 8;   // one table per slot

struct BatchListArgs {
  const uint64_t* recs;      // recWords words per bucket
  uint64_t totalTiles;
  uint64_t arg;
  const void* argPtr;
  uint32_t preMask;
  int32_t postOp;
  int32_t acquireSystem;
  int32_t nRecs;
  uint32_t chunk;            // consecutive tiles per workgroup turn
  uint32_t recWords;         // words per record: 3 + nSrcs + max nDsts of the launch
  uint32_t tileEnd[kListMaxRecs];   // running tile totals (recs[k][1]); totals < 2^32
};

// Launch table for one functor (kernel entry points as host handles).

struct KernelSet {
  const void* packs[2][kMaxKSrcs];  // [0 = small tile, 1 = big tile][nSrcs-1]
  const void* elts;
  const void* shifted;              // sources realigned against 16-B aligned destinations (kReduceShifted, run-time source count; fallback)
  const void* shiftedN[kMaxKSrcs];   // the same per source count, [nSrcs-1] (kReduceShiftedLds: LDS-DMA staging)
  const void* ll;                   // LL-protocol collectives (nbx_ll.h)
  const void* ll128;                // LL128-protocol collectives (nbx_ll.h)
  const void* ll128x2;              // LL128 two-shot AllReduce (nbx_ll.h)
  const void* llChk;                // the same three with plan words (NBX_CHECK_PLANS)
  const void* ll128Chk;
  const void* ll128x2Chk;
  const void* simple;               // Simple protocol, direct schedule over init-mapped staging (nbx_simple.h)
  const void* simpleRing;           // Simple protocol, ring schedule over init-mapped staging (nbx_simple.h)
  const void* simpleChk;            // the same two with slice checksums (NBX_CHECK_SLICES)
  const void* simpleRingChk;
  const void* batch[kMaxKSrcs];     // batched buckets (kReduceBatch), [nSrcs-1]
  const void* batchList[kMaxKSrcs]; // batched buckets from a work-list table (kReduceBatchList), [nSrcs-1]
  int unroll[kMaxKSrcs];            // big-tile packs per lane per source
  int bigBlocksPerCU;               // Fn::kBigBlocksPerCU (at least this many big-tile workgroups per CU)
  int eltBytes;
  int valid;
};

// Launch table for one source type of the fp32-accumulating sums (nbx_wide.h,
// nbxReduceMultiWide). One tile shape per source count: 4 packs per lane per
// source from 4 sources (the per-step kernels' big tile for 5-8), one below
// (their small tile, which wins for 1-3 sources).
constexpr int wideUnroll(int nSrcs) { return nSrcs >= 4 ? 4 : 1; }

struct WideSet {
  const void* packs[2][2][kMaxKSrcs];  // [0 = source-type output, 1 = fp32 output][source 0 is an fp32 partial][nSrcs-1]
  const void* elts[2][2];              // element kernels, same first two indices
  const void* shiftedLds[2][2][kMaxKSrcs];  // realigning kernels (kWideShiftedLds: LDS-DMA staging), indexed as packs
  const void* batchList[2][kMaxKSrcs]; // batched buckets from a work-list table (kWideBatchList), [fp32 output][nSrcs-1]
  int blocksPerCU;                     // at least this many unrolled-tile workgroups per CU
  int eltBytes;
  int valid;
};

// MXFP8 block-scaled form of the fp32-accumulating sums (nbx_mx.h,
// nbxReduceMultiWideMx): 32-element blocks, one E8M0 scale byte each. A lane of
// the block kernel holds one 16-element group (half a block: one dwordx4 of
// fp8 codes), so a tile is mxUnroll x kBlock groups. The packs per lane and
// source follow wideUnroll: an fp8 group is one pack, a 16-bit group two, so
// the 16-bit tile holds half the groups (and never less than one).
constexpr int kMxBlockElts = 32;
constexpr int kMxGroupElts = 16;
constexpr int mxUnroll(int nSrcs, int eltBytes) {
  return eltBytes == 1 ? wideUnroll(nSrcs) : (wideUnroll(nSrcs) >= 2 ? wideUnroll(nSrcs) / 2 : 1);
}

// The scale arrays travel as a second kernel argument, so KArgs is what it was.
struct MxArgs {
  const uint8_t* srcScale[kMaxKSrcs];   // scaled sources only; slot 0 unused behind a partial
  uint8_t* dstScale[kMaxKDsts];         // fp8 outputs only
};

// Launch table of one source kind of nbxReduceMultiWideMx, the same struct for
// every element format (the kinds and their outputs: nbx_registry.h MxTable).
// [output][source 0 is an fp32 partial][nSrcs-1]; the generic kernel takes
// nSrcs at run time. An output a kind does not have stays NULL.
constexpr int kMxKinds = 13, kMxOuts = 3;
constexpr int kMxFp8Kinds = 6;   // the MXFP8 kinds come first; the batch has these alone
struct MxSet {
  const void* blocks[kMxOuts][2][kMaxKSrcs];
  const void* generic[kMxOuts][2];
  int scaled;   // the sources carry block scales
  int valid;
};
// One output of a set: the block kernels of 1 .. 8 sources, those behind a
// partial (later[0] is NULL: a partial alone is no pass), the generic pair.
inline void setMxOut(MxSet& ms, int out, const void* const* first, const void* const* later, const void* generic,
                     const void* genericPart) {
  for (int i = 0; i < kMaxKSrcs; i++) {
    ms.blocks[out][0][i] = first[i];
    ms.blocks[out][1][i] = later[i];
  }
  ms.generic[out][0] = generic;
  ms.generic[out][1] = genericPart;
}

// Its 2-D form (nbx_mx2d.h, nbxReduceMultiWideMx2d): a row-major rows x cols
// bucket stored with blocks down the columns and, when asked, along the rows
// too. The tile kernel's workgroup owns kMx2dTileRows x kMx2dTileCols elements,
// a lane one 16-element group of one row; a wave of the any-layout kernel owns
// kMx2dTileRows x kMx2dWaveCols, a lane one column. KArgs.dst holds the
// column-wise destinations; everything else 2-D travels in Mx2dArgs.
constexpr int kMx2dTileRows = kMxBlockElts;
constexpr int kMx2dTileCols = (kBlock / kMx2dTileRows) * kMxGroupElts;   // 8 groups: 128
constexpr int kMx2dWaveCols = 64;
struct Mx2dArgs {
  const uint8_t* srcScale[kMaxKSrcs];   // scaled sources only (flat 1-D blocks); slot 0 unused behind a partial
  uint8_t* colScale[kMaxKDsts];         // ceil(rows / 32) x cols
  void* rowDst[kMaxKDsts];              // rowOut only
  uint8_t* rowScale[kMaxKDsts];         // rowOut only: rows x ceil(cols / 32)
  uint64_t rows, cols;
  int32_t rowOut;                       // uniform: the row-wise copy is stored too
  int32_t pad;
};
// Launch table of one MXFP8 source kind: [output 0 e4m3, 1 e5m2][source 0 is
// an fp32 partial][nSrcs-1]; the any-layout kernel takes nSrcs at run time.
struct Mx2dSet {
  const void* tiles[2][2][kMaxKSrcs];
  const void* generic[2][2];
  int valid;
};

// Its work-list batch (nbx_mx_batch.h, nbxReduceMultiWideMxBatch):
// kMxBatchList takes BatchListArgs as it is and one tile shape for every
// source type and count — one group per lane, kBlock groups, 128 blocks. A
// record in the arena slot, words of 8 bytes:
//   tileBegin, tileEnd, count | nDsts << 60   (no head: blocks count from element 0)
//   nSrcs sources, then nSrcs source-scale pointers (scaled kinds)
//   maxD destinations, then maxD destination-scale pointers (MX output),
//   maxD the launch's largest nDsts; unused entries 0
// so recWords = 3 + nSrcs (1 + scaled) + maxD (1 + MX output) <= kMxBatchRecWords,
// and a launch holds min(kListMaxRecs, slot words / recWords) records.
constexpr int kMxBatchTileGroups = kBlock;
constexpr int kMxBatchTileElts = kMxBatchTileGroups * kMxGroupElts;
constexpr int kMxBatchRecWords = 3 + 2 * kMaxKSrcs + 2 * kMaxKDsts;
constexpr int mxBatchRecWords(int nSrcs, bool scaled, int maxD, bool mxOut) {
  return 3 + nSrcs * (scaled ? 2 : 1) + maxD * (mxOut ? 2 : 1);
}

// Its launch table, one per MXFP8 source kind: [output as MxSet::blocks][nSrcs-1].
struct MxBatchSet {
  const void* list[kMxOuts][kMaxKSrcs];
  int valid;
};

// MXFP4 elements in the same call (nbx_mx4.h): two codes per byte, so a lane of
// the block kernel holds one 8-element group (a quarter of a block: one dword
// of codes, one dwordx4 of a 16-bit source) and a tile is mx4Unroll x kBlock
// groups. An FP4 source brings 4 bytes per lane and step, so its tiles are deep;
// a 16-bit source brings the wide kernels' 16.
constexpr int kMx4GroupElts = 8;
constexpr int kTypeFp4 = 32;   // NBX_FLOAT4_E2M1 (include/nbx_reduce.h): a tag outside ncclDataType_t's own values
constexpr int mx4Unroll(int nSrcs, bool fp4) { return fp4 ? (nSrcs <= 4 ? 8 : 4) : (nSrcs >= 4 ? 4 : 2); }

// MXFP6 elements in the same call (nbx_mx6.h): 6-bit codes in a dense bit stream,
// 24 bytes per block. gfx950's FP6 converters take a whole block in one lane, so
// the block kernel's unit is the block: a lane ends up owning mx6Unroll blocks
// per tile (a tile is mx6Unroll x kBlock blocks). A 16-bit source brings 64 bytes
// per lane and block, an MXFP6 source 24.
constexpr int kTypeFp6E2M3 = 33, kTypeFp6E3M2 = 34;   // NBX_FLOAT6_E2M3 / NBX_FLOAT6_E3M2 (include/nbx_reduce.h)
constexpr int mx6Unroll(int nSrcs, bool fp6) { return fp6 ? (nSrcs <= 4 ? 4 : 2) : (nSrcs <= 3 ? 2 : 1); }

// Bucket statistics of the fp32-accumulating sums (nbxReduceMultiWideStats,
// nbx_wide.h "Bucket statistics"). The STATS kernels take the slot array as a
// second kernel argument, so KArgs and BatchListArgs are what they were.
struct WideSlot {      // one tile's (and wave's) partial: 16 bytes, one dwordx4 store
  double sumSq;
  float amax;          // IEEE max: a NaN element shows in sumSq only
  uint32_t pad;
};
constexpr int kWideEltsStatTile = 8;      // elements per lane per tile of kWideEltsStats
constexpr int kWideStatsFan = 4096;       // slots one workgroup of kWideStatsReduce sums

// kWideStatsBatch: workgroup r sums record r's slot range
// [begin * 4 + r, tileEnd[r] * 4 + r] (begin = tileEnd[r - 1], 0 for r = 0)
// into stats[statIdx[r]].
struct WideStatsBatchArgs {
  const WideSlot* slots;
  void* stats;                        // nbxWideStats*
  uint32_t tileEnd[kListMaxRecs];
  uint32_t statIdx[kListMaxRecs];
};

// Launch table for one element type of the collectives' fp32-accumulating
// folds (nbx_wide_coll.h: the direct-schedule kernels of nbx_ll.h and
// nbx_simple.h over FnWide). A table of its own, as WideSet: KernelSet and
// nbxKernelCount stay as they are. There is no ring entry: the ring moves
// partials of the element type.
struct WideCollSet {
  const void* ll;
  const void* ll128;
  const void* ll128x2;
  const void* llChk;        // the same three with plan words (NBX_CHECK_PLANS)
  const void* ll128Chk;
  const void* ll128x2Chk;
  const void* simple;       // Simple protocol, direct schedule
  const void* simpleChk;    // with slice checksums (NBX_CHECK_SLICES)
  int valid;
};

}  // namespace nbx
