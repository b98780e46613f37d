// nbx_reduce_mx_batch.cc — nbxReduceMultiWideMxBatch: the checks of every
// bucket, which buckets enter a work-list table, the MX record writer and the
// launches of kMxBatchList (nbx_mx_batch.h). The arena and the life cycle of
// its slots are nbx_reduce_batch.cc's.
#include <cstdio>
#include <mutex>
#include <vector>

#include "nbx_launch.h"

namespace nbx {
namespace {
MxBatchTable g_mxBatch;
std::once_flag g_mxBatchOnce;

// A batched bucket's tiles: kMxBatchTileGroups 16-element groups of its full
// blocks each; a bucket below one block still owns a tile (its elements).
uint64_t mxBucketTiles(const nbxReduceMxTask& t) {
  const uint64_t groups = (uint64_t)(t.count / kMxBlockElts) * (kMxBlockElts / kMxGroupElts);
  const uint64_t tiles = (groups + kMxBatchTileGroups - 1) / kMxBatchTileGroups;
  return tiles ? tiles : 1;
}

// Launches the buckets of one source count as kMxBatchList launches (as many
// as slots they need): launchBatchList's loop (nbx_reduce_batch.cc) over the
// MX record (nbx_kargs.h). *done: the buckets launched from the front of `ts`
// (fewer than ts.size() when no slot was free).
ncclResult_t launchMxBatchList(const void* kernel, bool scaled, bool mxOut, int nSrcs,
                               const std::vector<const nbxReduceMxTask*>& ts, const nbxDevRedOpFull& op, uint32_t mask,
                               hipStream_t st, size_t* done) {
  *done = 0;
  const int dev = launchDevice(st);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  hipGraph_t graph = nullptr;
  if (hipStreamGetCaptureInfo_v2(st, &cs, nullptr, &graph, nullptr, nullptr) != hipSuccess) {
    cs = hipStreamCaptureStatusNone;
    graph = nullptr;
  }
  const bool capturing = cs != hipStreamCaptureStatusNone;
  if (capturing && (cs != hipStreamCaptureStatusActive || graph == nullptr)) return ncclSuccess;
  const uint64_t maxG = (uint64_t)cuCount(dev) * (uint64_t)maxBlocksPerCU(false, nSrcs, false);
  static const uint64_t chunkEnv = (uint64_t)envInt("NBX_BATCH_CHUNK", 4);   // as launchBatchList; not measured here
  const uint64_t chunk = chunkEnv < 1 ? 1 : chunkEnv;
  constexpr size_t kSlotWords = (size_t)kBatchListSlotBytes / 8;
  static_assert(kSlotWords / kMxBatchRecWords >= 1, "a slot holds the widest record");
  const int flagBits = (mxOut ? 0 : kLaunchOut32) | (scaled ? kLaunchMxScaled : 0);
  BatchListArgs a;
  size_t i = 0;
  while (i < ts.size()) {
    // this launch's buckets: records of the launch's widest shape that fit the
    // slot, up to kListMaxRecs, running tile totals < 2^32
    size_t nRec = 0;
    uint64_t tiles = 0;
    int maxD = 1;
    while (nRec < (size_t)kListMaxRecs && i + nRec < ts.size()) {
      const nbxReduceMxTask& t = *ts[i + nRec];
      const int d = t.nDsts > maxD ? t.nDsts : maxD;
      if ((nRec + 1) * (size_t)mxBatchRecWords(nSrcs, scaled, d, mxOut) > kSlotWords) break;
      const uint64_t next = tiles + mxBucketTiles(t);
      if (next > 0xffffffffull) break;
      maxD = d;
      tiles = next;
      a.tileEnd[nRec++] = (uint32_t)tiles;
    }
    if (nRec == 0) return ncclSuccess;   // a bucket of >= 2^32 tiles: the caller's single launch
    char* mem = nullptr;
    const int slot = acquireListSlot(dev, capturing, &mem);
    if (slot < 0) return ncclSuccess;
    uint64_t* recs = (uint64_t*)mem;   // write-only: the slot may be device memory behind the BAR
    const int recWords = mxBatchRecWords(nSrcs, scaled, maxD, mxOut);
    for (size_t r = 0; r < nRec; r++) {
      const nbxReduceMxTask& t = *ts[i + r];
      uint64_t* w = recs + r * (size_t)recWords;
      *w++ = r ? a.tileEnd[r - 1] : 0;
      *w++ = a.tileEnd[r];
      *w++ = (uint64_t)t.count | (uint64_t)t.nDsts << 60;
      for (int s = 0; s < nSrcs; s++) *w++ = (uint64_t)(uintptr_t)t.srcs[s];
      for (int s = 0; scaled && s < nSrcs; s++) *w++ = (uint64_t)(uintptr_t)t.srcScales[s];
      for (int d = 0; d < maxD; d++) *w++ = d < t.nDsts ? (uint64_t)(uintptr_t)t.dsts[d] : 0;
      for (int d = 0; mxOut && d < maxD; d++) *w++ = d < t.nDsts ? (uint64_t)(uintptr_t)t.dstScales[d] : 0;
    }
    a.recs = recs;
    a.nRecs = (int)nRec;
    a.chunk = (uint32_t)chunk;
    a.recWords = (uint32_t)recWords;
    a.totalTiles = tiles;
    setScalarArg(a, op);
    a.preMask = mask;
    a.postOp = 0;
    a.acquireSystem = 0;
    publishListSlot(dev, (const volatile uint32_t*)(recs + nRec * (size_t)recWords - 1));
    const size_t G = cappedGrid((tiles + chunk - 1) / chunk, maxG);
    void* args[] = {&a};
    const hipError_t err = hipLaunchKernel(kernel, dim3((unsigned)G), dim3(kBlock), args, 0, st);
    releaseListSlot(dev, slot, st, capturing ? graph : nullptr, err == hipSuccess);
    if (err != hipSuccess) {
      std::fprintf(stderr, "nbx: MX batch-list kernel launch failed: %s\n", hipGetErrorString(err));
      return ncclUnhandledCudaError;
    }
    logLaunch(kFamMxBatchList, nSrcs, 1, flagBits | ((int)nRec << kLaunchSegsShift));
    i += nRec;
    *done = i;
  }
  return ncclSuccess;
}
}  // namespace

const MxBatchTable& mxBatchTable() {
  std::call_once(g_mxBatchOnce, [] {
    std::memset(&g_mxBatch, 0, sizeof(g_mxBatch));
    fillMxBatchF16(g_mxBatch);
    fillMxBatchBF16(g_mxBatch);
    fillMxBatchE4M3(g_mxBatch);
    fillMxBatchE5M2(g_mxBatch);
    fillMxBatchE4M3Scaled(g_mxBatch);
    fillMxBatchE5M2Scaled(g_mxBatch);
  });
  return g_mxBatch;
}

}  // namespace nbx

using namespace nbx;

// The buckets kMxBlocks would take go into work-list launches of kMxBatchList
// per source count; every other bucket, and every bucket no table slot was
// left for, is one nbxReduceMultiWideMx launch (wideBatch's policy,
// nbx_reduce_batch.cc).
NBX_EXPORT ncclResult_t nbxReduceMultiWideMxBatch(const nbxReduceMxTask* tasks, int nTasks, ncclDataType_t srcType,
                                                  ncclDataType_t dstType, nbxDevRedOpFull op, int nPreOpSrcs,
                                                  ncclStream_t stream) {
  // ---- checks: all of them before any device call ----
  const int st = (int)srcType, dt = (int)dstType;
  const bool out32 = dt == (int)ncclFloat32;
  // scaled or plain is a property of the call; without a bucket to say which,
  // the types are checked as those of the form that takes this output
  const bool scaled = nTasks > 0 && tasks != nullptr ? tasks[0].srcScales != nullptr : out32;
  int kind, out;
  ncclResult_t r = checkMxTypes(srcType, dstType, op, scaled, !out32, &kind, &out);
  if (r != ncclSuccess) return r;
  if (kind >= kMxFp8Kinds) return ncclInvalidArgument;   // the MXFP8 kinds (and so their outputs) alone are batched
  if (nTasks < 0 || (nTasks > 0 && tasks == nullptr)) return ncclInvalidArgument;
  bool any = false;
  for (int i = 0; i < nTasks; i++) {
    const nbxReduceMxTask& t = tasks[i];
    if ((t.srcScales != nullptr) != scaled || (t.dstScales != nullptr) == out32) return ncclInvalidArgument;
    if (!argArraysOk(t.dsts, t.nDsts, t.srcs, t.nSrcs)) return ncclInvalidArgument;
    if (t.count == 0) continue;   // the entries of its arrays unexamined, as in the single call
    r = checkMxBucket(st, dt, t.dsts, t.dstScales, t.nDsts, t.srcs, t.srcScales, t.nSrcs, t.count);
    if (r != ncclSuccess) return r;
    any = true;
  }
  if (!any) return ncclSuccess;

  if (nPreOpSrcs < 0) nPreOpSrcs = 0;
  const bool pre = op.op == nbxDevPreMulSum;
  hipStream_t hs = (hipStream_t)stream;
  auto alone = [&](const nbxReduceMxTask& t) {
    return nbxReduceMultiWideMx(t.dsts, t.dstScales, t.nDsts, t.srcs, t.srcScales, t.nSrcs, t.count, srcType, dstType,
                                op, nPreOpSrcs, stream);
  };
  // single buckets first, in bucket order: layouts the block kernel does not
  // take, > 8 sources (passes through the fp32 partial), everything under
  // launch variant 2, and buckets of 4+ sources whose groups give every CU one
  // of the single call's unrolled tiles alone (bigTileRule; variant 1 batches
  // those too)
  const int eb = typeSize(st);
  const int force = launchVariant();
  const uint64_t cus = (uint64_t)cuCount(launchDevice(hs));
  std::vector<const nbxReduceMxTask*> lists[kMaxKSrcs];
  for (int i = 0; i < nTasks; i++) {
    const nbxReduceMxTask& t = tasks[i];
    if (t.count == 0) continue;
    const bool single =
        t.nSrcs > kMaxKSrcs || t.count > kBatchCountMask ||
        !mxBlockLayout(t.dsts, out32 ? nullptr : t.dstScales, t.nDsts, t.srcs, t.nSrcs) ||
        bigTileRule(force, t.nSrcs, false, (uint64_t)(t.count / kMxBlockElts) * (kMxBlockElts / kMxGroupElts),
                    (uint64_t)mxUnroll(t.nSrcs, eb) * kBlock, cus, /*partialTileCounts=*/false);
    if (single) {
      r = alone(t);
      if (r != ncclSuccess) return r;
      continue;
    }
    lists[t.nSrcs - 1].push_back(&t);
  }
  const nbxDevRedOpFull lop = wideScalarOp(op);
  const MxBatchSet& bs = mxBatchTable()[kind];
  const bool useList = batchListEnabled();
  for (int q = 0; q < kMaxKSrcs; q++) {
    if (lists[q].empty()) continue;
    const int ns = q + 1;
    size_t done = 0;
    if (useList) {
      r = launchMxBatchList(bs.list[out][q], scaled, !out32, ns, lists[q], lop, preMask(pre, nPreOpSrcs, 0, ns, 0), hs,
                            &done);
      if (r != ncclSuccess) return r;
    }
    // the rest one launch each (work lists off, or no table slot free)
    for (size_t j = done; j < lists[q].size(); j++) {
      r = alone(*lists[q][j]);
      if (r != ncclSuccess) return r;
    }
  }
  return ncclSuccess;
}

// Elements of kMxBatchList's tile, the same for every source type and count
// (test hook, include/nbx_debug.h).
NBX_EXPORT int nbxDebugMxBatchTileElts(void) { return kMxBatchTileElts; }
