// nbx_reduce_batch.cc — the batched entry points (nbxReduceMultiBatch,
// nbxReduceMultiWideBatch): which buckets leave the batch, the
// kernel-argument packer, and the work-list arena with its slot life cycle.
#include <cstdio>
#include <mutex>
#include <vector>

#include "nbx_launch.h"

namespace nbx {
namespace {
// A batched bucket's tiles (kBatchTilePacks packs each) and *head, the
// elements of eb bytes that bring its sources to a 16-byte boundary (at most
// count). A bucket below one pack still owns a tile (its elements).
uint64_t bucketTiles(const nbxReduceTask& t, int eb, uint64_t* head) {
  const unsigned mis = (unsigned)((uintptr_t)t.srcs[0] & 15u);
  uint64_t h = mis ? (uint64_t)((16u - mis) / (unsigned)eb) : 0;
  if (h > t.count) h = t.count;
  *head = h;
  const uint64_t nPacks = (t.count - h) / (uint64_t)(16 / eb);
  const uint64_t tiles = (nPacks + kBatchTilePacks - 1) / kBatchTilePacks;
  return tiles ? tiles : 1;
}

// Packs bucket records (nbx_kargs.h BatchArgs) for kReduceBatch launches of
// one source count; a launch goes out when the table is full, or on flush().
struct BatchPacker {
  const KernelSet& ks;
  int nSrcs;
  const nbxDevRedOpFull& op;
  uint32_t mask;
  int postOp, acquireSystem;
  hipStream_t stream;
  BatchArgs a;
  int used = 0;

  BatchPacker(const KernelSet& k, int ns, const nbxDevRedOpFull& o, uint32_t pm, int post, int acq, hipStream_t st)
      : ks(k), nSrcs(ns), op(o), mask(pm), postOp(post), acquireSystem(acq), stream(st) {
    static_assert(sizeof(BatchArgs) <= 4096, "batch table must fit the kernel-argument segment");
    reset();
  }
  void reset() {
    std::memset(&a, 0, offsetof(BatchArgs, w));
    used = 0;
  }
  // appends one bucket (count > 0, one shared misalignment)
  ncclResult_t add(const nbxReduceTask& t) {
    const int len = 2 + nSrcs + t.nDsts;
    if (used + len > kBatchWords) {
      ncclResult_t r = flush();
      if (r != ncclSuccess) return r;
    }
    uint64_t head = 0;
    a.totalTiles += bucketTiles(t, ks.eltBytes, &head);
    uint64_t* w = a.w + used;
    w[0] = a.totalTiles;
    w[1] = (uint64_t)t.count | head << 56 | (uint64_t)t.nDsts << 60;
    for (int s = 0; s < nSrcs; s++) w[2 + s] = (uint64_t)(uintptr_t)t.srcs[s];
    for (int d = 0; d < t.nDsts; d++) w[2 + nSrcs + d] = (uint64_t)(uintptr_t)t.dsts[d];
    used += len;
    a.nTasks++;
    return ncclSuccess;
  }
  ncclResult_t flush() {
    if (a.nTasks == 0) return ncclSuccess;
    setScalarArg(a, op);
    a.preMask = mask;
    a.postOp = postOp;
    a.acquireSystem = acquireSystem;
    const size_t maxBlocks =
        (size_t)cuCount(launchDevice(stream)) * (size_t)maxBlocksPerCU(false, nSrcs, acquireSystem != 0);
    const size_t grid = cappedGrid(a.totalTiles, maxBlocks);
    void* args[] = {&a};
    hipError_t err = hipLaunchKernel(ks.batch[nSrcs - 1], dim3((unsigned)grid), dim3(kBlock), args, 0, stream);
    const int nBuckets = a.nTasks;
    reset();
    if (err != hipSuccess) {
      std::fprintf(stderr, "nbx: batch kernel launch failed: %s\n", hipGetErrorString(err));
      return ncclUnhandledCudaError;
    }
    logLaunch(kFamBatch, nSrcs, 1, nBuckets << kLaunchSegsShift);
    return ncclSuccess;
  }
};

// Work-list tables (kReduceBatchList): one arena of kListSlots fixed-size
// slots per device, allocated on first use outside stream capture. Where the
// device's memory is CPU-visible (large BAR) the arena is uncached device
// memory the host writes directly — a workgroup's dependent record read then
// costs ~110 ns instead of ~1.2 us from pinned host memory
// (scripts/probe_table_mem.hip, profiles/r2/probe_table_mem_r2.txt); uncached,
// so no GPU cache can keep an earlier table of a reused slot. Otherwise the
// arena is pinned, coherent host memory the kernel reads in place.
// A slot written for an eager launch is reusable once the event recorded after
// that launch has completed; every eager call sweeps a few slots' events so
// completed slots return to the free pool (a capture cannot query events). A
// slot written while the stream is being captured belongs to the graph (every
// replay reads it); a user object retained by the graph hands it back when
// the graph is destroyed. Nothing ever waits for a slot: with none free the
// caller falls back to kernel-argument batches.
constexpr int kListSlots = 128;
constexpr int kListSweep = 8;   // eager calls query at most this many in-flight slots

struct ListArena {
  std::mutex mu;
  char* base = nullptr;
  bool onDevice = false;
  hipEvent_t ev[kListSlots] = {};
  std::atomic<int> state[kListSlots];   // 0 free, 1 eager (event pending), 2 owned by a graph
  std::atomic<long> fallbacks{0};       // launches that found no free slot
  int cursor = 0, sweep = 0;
  ListArena() {
    for (auto& s : state) s.store(0);
  }
};
ListArena g_lists[kMaxDevices];

void releaseGraphSlot(void* p) { static_cast<std::atomic<int>*>(p)->store(0); }

bool allocArena(ListArena& A, int dev) {
  CurDev cur(dev);
  const size_t bytes = (size_t)kListSlots * kBatchListSlotBytes;
  int largeBar = 0;
  static const int want = envInt("NBX_BATCH_TABLE_DEVICE", 1);
  void* p = nullptr;
  if (want && hipDeviceGetAttribute(&largeBar, hipDeviceAttributeIsLargeBar, dev) == hipSuccess && largeBar &&
      hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached) == hipSuccess) {
    A.onDevice = true;
  } else {
    p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocCoherent) != hipSuccess) return false;
    A.onDevice = false;
  }
  for (int i = 0; i < kListSlots; i++) {
    if (hipEventCreateWithFlags(&A.ev[i], hipEventDisableTiming) != hipSuccess) {
      for (int j = 0; j < i; j++) (void)hipEventDestroy(A.ev[j]);
      if (A.onDevice) (void)hipFree(p);
      else (void)hipHostFree(p);
      return false;
    }
  }
  A.base = (char*)p;
  return true;
}

// A free slot of this device's arena (index, *ptr = its memory), or -1.
int acquireListSlot(int dev, bool capturing, char** ptr) {
  if (dev < 0 || dev >= kMaxDevices) return -1;
  ListArena& A = g_lists[dev];
  std::lock_guard<std::mutex> lk(A.mu);
  if (A.base == nullptr) {
    if (capturing) return -1;   // no allocation inside a capture
    if (!allocArena(A, dev)) return -1;
  }
  if (!capturing) {   // return a few completed slots to the free pool
    for (int j = 0; j < kListSweep; j++) {
      const int i = A.sweep;
      A.sweep = (A.sweep + 1) % kListSlots;
      if (A.state[i].load() == 1 && hipEventQuery(A.ev[i]) == hipSuccess) A.state[i].store(0);
    }
  }
  int pick = -1;
  for (int j = 0; j < kListSlots && pick < 0; j++) {
    const int i = (A.cursor + j) % kListSlots;
    if (A.state[i].load() == 0) pick = i;
  }
  if (pick < 0 && !capturing) {   // the oldest in-flight slot, if it has completed
    for (int j = 0; j < kListSlots && pick < 0; j++) {
      const int i = (A.cursor + j) % kListSlots;
      if (A.state[i].load() == 1) {
        if (hipEventQuery(A.ev[i]) == hipSuccess) pick = i;
        break;
      }
    }
  }
  if (pick < 0) {
    A.fallbacks++;
    return -1;
  }
  A.state[pick].store(2);   // reserved until released by the launch
  A.cursor = (pick + 1) % kListSlots;
  *ptr = A.base + (size_t)pick * kBatchListSlotBytes;
  return pick;
}

// Make the host's writes into a device-memory slot land before the launch
// (posted PCIe writes, write-combined mapping): fence, then read one back.
void publishListSlot(int dev, const volatile uint32_t* last) {
  if (!g_lists[dev].onDevice) return;
  std::atomic_thread_fence(std::memory_order_seq_cst);
  (void)*last;
}

// After the launch that reads slot i: eager -> its event; captured -> the
// graph owns it until destroyed; launch failed -> free again.
void releaseListSlot(int dev, int i, hipStream_t st, hipGraph_t graph, bool launched) {
  ListArena& A = g_lists[dev];
  if (!launched) {
    A.state[i].store(0);
    return;
  }
  if (graph != nullptr) {
    hipUserObject_t obj = nullptr;
    if (hipUserObjectCreate(&obj, &A.state[i], releaseGraphSlot, 1, hipUserObjectNoDestructorSync) == hipSuccess &&
        hipGraphRetainUserObject(graph, obj, 1, hipGraphUserObjectMove) == hipSuccess)
      return;   // state stays 2 until the graph lets go of it
    return;     // could not attach: the slot stays the graph's for good (never reused)
  }
  if (hipEventRecord(A.ev[i], st) != hipSuccess) {
    (void)hipStreamSynchronize(st);
    A.state[i].store(0);
    return;
  }
  A.state[i].store(1);
}

// NBX_BATCH_LIST: 1 (default) = work-list launches (sets of <= 16 buckets
// that fit one kernel-argument table excepted), 2 = work lists for every set,
// 0 = kernel-argument batches only (also settable through nbxDebugSetBatchMode).
int parseBatchMode() {
  const int e = envInt("NBX_BATCH_LIST", 1);
  return e == 0 ? 0 : (e == 2 ? 2 : 1);
}
LazySetting<int> g_batchMode{-1, parseBatchMode};
bool batchListEnabled() { return g_batchMode.get() != 0; }

// Launches the buckets of one source count as work-list kernels (as many
// launches as slots they need). Returns the number of buckets launched from
// the front of `ts` (fewer than ts.size() when no slot was free). One record
// writer for both batched entry points: `kernel` is kReduceBatchList's or
// kWideBatchList's instantiation for nSrcs, eb the sources' element size (the
// head is counted in source elements), family / flagBits its launch record.
ncclResult_t launchBatchList(const void* kernel, int eb, int family, int flagBits, int nSrcs,
                             const std::vector<const nbxReduceTask*>& ts, const nbxDevRedOpFull& op, uint32_t mask,
                             int postOp, int acq, hipStream_t st, size_t* done) {
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
  const uint64_t maxG = (uint64_t)cuCount(dev) * (uint64_t)maxBlocksPerCU(false, nSrcs, acq != 0);
  // 4 consecutive tiles per workgroup turn: the best of 1 / 4 / 16 on every
  // config-C bucket set (profiles/r2/batch_list_chunk_r2p.jsonl)
  static const uint64_t chunkEnv = (uint64_t)envInt("NBX_BATCH_CHUNK", 4);
  const uint64_t chunk = chunkEnv < 1 ? 1 : chunkEnv;
  static_assert(sizeof(BatchListArgs) <= 4096, "work-list arguments must fit the kernel-argument segment");
  BatchListArgs a;
  size_t i = 0;
  while (i < ts.size()) {
    // this launch's buckets: up to kListMaxRecs, running tile totals < 2^32
    size_t nRec = 0;
    uint64_t tiles = 0, head = 0;
    int maxD = 1;
    while (nRec < (size_t)kListMaxRecs && i + nRec < ts.size()) {
      const nbxReduceTask& t = *ts[i + nRec];
      if (t.nDsts > maxD) maxD = t.nDsts;
      const uint64_t next = tiles + bucketTiles(t, eb, &head);
      if (next > 0xffffffffull) break;
      tiles = next;
      a.tileEnd[nRec++] = (uint32_t)tiles;
    }
    if (nRec == 0) return ncclSuccess;   // a bucket of >= 2^32 tiles: the caller's fallback
    char* mem = nullptr;
    const int slot = acquireListSlot(dev, capturing, &mem);
    if (slot < 0) return ncclSuccess;
    uint64_t* recs = (uint64_t*)mem;   // write-only: the slot may be device memory behind the BAR
    const int recWords = 3 + nSrcs + maxD;   // <= kBatchRecWords
    for (size_t r = 0; r < nRec; r++) {
      const nbxReduceTask& t = *ts[i + r];
      (void)bucketTiles(t, eb, &head);
      uint64_t* w = recs + r * (size_t)recWords;
      w[0] = r ? a.tileEnd[r - 1] : 0;
      w[1] = a.tileEnd[r];
      w[2] = (uint64_t)t.count | head << 56 | (uint64_t)t.nDsts << 60;
      for (int s = 0; s < nSrcs; s++) w[3 + s] = (uint64_t)(uintptr_t)t.srcs[s];
      for (int d = 0; d < maxD; d++) w[3 + nSrcs + d] = d < t.nDsts ? (uint64_t)(uintptr_t)t.dsts[d] : 0;
    }
    const size_t G = cappedGrid((tiles + chunk - 1) / chunk, maxG);
    a.recs = recs;
    a.nRecs = (int)nRec;
    a.chunk = (uint32_t)chunk;
    a.recWords = (uint32_t)recWords;
    a.totalTiles = tiles;
    setScalarArg(a, op);
    a.preMask = mask;
    a.postOp = postOp;
    a.acquireSystem = acq;
    publishListSlot(dev, (const volatile uint32_t*)(recs + nRec * (size_t)recWords - 1));
    void* args[] = {&a};
    const hipError_t err = hipLaunchKernel(kernel, dim3((unsigned)G), dim3(kBlock), args, 0, st);
    releaseListSlot(dev, slot, st, capturing ? graph : nullptr, err == hipSuccess);
    if (err != hipSuccess) {
      std::fprintf(stderr, "nbx: batch-list kernel launch failed: %s\n", hipGetErrorString(err));
      return ncclUnhandledCudaError;
    }
    logLaunch(family, nSrcs, 1, flagBits | ((int)nRec << kLaunchSegsShift));
    i += nRec;
    *done = i;
  }
  return ncclSuccess;
}
}  // namespace

ncclResult_t reduceMultiBatchEx(const nbxReduceTask* tasks, int nTasks, ncclDataType_t datatype, nbxDevRedOpFull op,
                                int nPreOpSrcs, int postOp, ncclStream_t stream, int flags) {
  if (nTasks < 0 || (nTasks > 0 && tasks == nullptr)) return ncclInvalidArgument;
  const KernelSet* ksp = nullptr;
  ncclResult_t r = checkOp(datatype, op, &ksp);
  if (r != ncclSuccess) return r;
  const KernelSet& ks = *ksp;
  const size_t eb = (size_t)ks.eltBytes;
  // every bucket is checked before anything is enqueued
  for (int i = 0; i < nTasks; i++) {
    r = checkBucket(eb, eb, false, tasks[i].dsts, tasks[i].nDsts, tasks[i].srcs, tasks[i].nSrcs, tasks[i].count);
    if (r != ncclSuccess) return r;
  }
  if (nPreOpSrcs < 0) nPreOpSrcs = 0;
  const bool pre = op.op == nbxDevPreMulSum;
  const int post = (op.op == nbxDevSumPostDiv && postOp) ? 1 : 0;
  const int acq = (flags & kReduceAcquireSystem) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  // buckets with <= 8 sources and one shared alignment go into batches per
  // source count, in order; the rest (mixed alignment, > 8 sources) take the
  // single-bucket path, and so do buckets of 4+ sources big enough to give
  // every CU a big tile on their own (bigTileRule: they fill the GPU alone, at
  // the big tile's higher rate; 1-3 sources use the batch kernel's tile shape
  // anyway). Launch variant 1 (force small tiles) batches those too; variant 2
  // (force big tiles) batches nothing.
  const int force = launchVariant();
  const uint64_t cus = (uint64_t)cuCount(launchDevice(st));
  const uint64_t epp = 16 / eb;
  std::vector<const nbxReduceTask*> lists[kMaxKSrcs];
  const bool useList = batchListEnabled();
  for (int i = 0; i < nTasks; i++) {
    const nbxReduceTask& t = tasks[i];
    if (t.count == 0) continue;
    const bool single = t.nSrcs > kMaxKSrcs || t.count > kBatchCountMask ||
                        sharedMisalignment(t.dsts, t.nDsts, t.srcs, t.nSrcs) < 0 ||
                        bigTileRule(force, t.nSrcs, acq != 0, t.count / epp, (uint64_t)ks.unroll[t.nSrcs - 1] * kBlock,
                                    cus, /*partialTileCounts=*/false);
    if (single) {
      r = reduceMultiEx(t.dsts, t.nDsts, t.srcs, t.nSrcs, t.count, datatype, op, nPreOpSrcs, postOp, stream, flags);
      if (r != ncclSuccess) return r;
      continue;
    }
    lists[t.nSrcs - 1].push_back(&t);
  }
  for (int q = 0; q < kMaxKSrcs; q++) {
    if (lists[q].empty()) continue;
    const int ns = q + 1;
    const uint32_t mask = preMask(pre, nPreOpSrcs, 0, ns, 0);
    size_t done = 0;
    // a handful of buckets that fit one kernel-argument table run faster from
    // it (records in the scalar cache, a short cursor walk); longer lists,
    // whose cursor walk dominates, take the work list
    bool fitsKernarg = g_batchMode.get() != 2 && lists[q].size() <= (size_t)kBatchKernargMaxBuckets;
    if (fitsKernarg) {
      size_t words = 0;
      for (const nbxReduceTask* t : lists[q]) words += (size_t)(2 + ns + t->nDsts);
      fitsKernarg = words <= (size_t)kBatchWords;
    }
    if (useList && !fitsKernarg) {
      r = launchBatchList(ks.batchList[q], ks.eltBytes, kFamBatchList, 0, ns, lists[q], op, mask, post, acq, st,
                          &done);
      if (r != ncclSuccess) return r;
    }
    if (done == lists[q].size()) continue;
    // the rest as kernel-argument batches (work lists off, or no table slot free)
    BatchPacker packer(ks, ns, op, mask, post, acq, st);
    for (size_t j = done; j < lists[q].size(); j++) {
      r = packer.add(*lists[q][j]);
      if (r != ncclSuccess) return r;
    }
    r = packer.flush();
    if (r != ncclSuccess) return r;
  }
  return ncclSuccess;
}

}  // namespace nbx

using namespace nbx;

NBX_EXPORT ncclResult_t nbxReduceMultiBatch(const nbxReduceTask* tasks, int nTasks, ncclDataType_t datatype,
                                            nbxDevRedOpFull op, int nPreOpSrcs, int postOp, ncclStream_t stream) {
  return reduceMultiBatchEx(tasks, nTasks, datatype, op, nPreOpSrcs, postOp, stream, 0);
}

// nbxReduceMultiWideBatch: the buckets nbxReduceMultiWide's pack kernel would
// take go into work-list launches of kWideBatchList per source count; every
// other bucket, and every bucket no table slot was left for, is one
// nbxReduceMultiWide launch. There is no kernel-argument form, so batch modes
// 1 and 2 both mean work lists.
NBX_EXPORT ncclResult_t nbxReduceMultiWideBatch(const nbxReduceTask* tasks, int nTasks, ncclDataType_t srcType,
                                                ncclDataType_t dstType, nbxDevRedOpFull op, int nPreOpSrcs,
                                                ncclStream_t stream) {
  ncclResult_t r = checkWideOp(srcType, dstType, op);
  if (r != ncclSuccess) return r;
  if (nTasks < 0 || (nTasks > 0 && tasks == nullptr)) return ncclInvalidArgument;
  const int stype = (int)srcType;
  const WideSet& ws = wideTable()[stype];
  const bool out32 = (int)dstType != stype;
  const size_t eb = (size_t)ws.eltBytes, deb = out32 ? sizeof(float) : eb;
  // every bucket is checked before anything is enqueued
  bool any = false;
  for (int i = 0; i < nTasks; i++) {
    r = checkBucket(eb, deb, out32, tasks[i].dsts, tasks[i].nDsts, tasks[i].srcs, tasks[i].nSrcs, tasks[i].count);
    if (r != ncclSuccess) return r;
    any |= tasks[i].count != 0;
  }
  if (!any) return ncclSuccess;
  if (nPreOpSrcs < 0) nPreOpSrcs = 0;
  const bool pre = op.op == nbxDevPreMulSum;
  hipStream_t st = (hipStream_t)stream;
  // single buckets first, in bucket order: layouts the pack kernel does not
  // take, > 8 sources (passes through the fp32 partial), everything under
  // launch variant 2, and buckets of 4+ sources whose body gives every CU an
  // unrolled tile alone (bigTileRule; variant 1 batches those too)
  const int force = launchVariant();
  const uint64_t cus = (uint64_t)cuCount(launchDevice(st));
  std::vector<const nbxReduceTask*> lists[kMaxKSrcs];
  for (int i = 0; i < nTasks; i++) {
    const nbxReduceTask& t = tasks[i];
    if (t.count == 0) continue;
    size_t head = 0;
    const bool single = t.nSrcs > kMaxKSrcs || t.count > kBatchCountMask ||
                        wideLayout(eb, deb, t.dsts, t.nDsts, t.srcs, t.nSrcs, t.count, &head) != kWideLayoutPacks ||
                        bigTileRule(force, t.nSrcs, false, (t.count - head) / (16 / eb),
                                    (uint64_t)wideUnroll(t.nSrcs) * kBlock, cus, /*partialTileCounts=*/false);
    if (single) {
      r = nbxReduceMultiWide(t.dsts, t.nDsts, t.srcs, t.nSrcs, t.count, srcType, dstType, op, nPreOpSrcs, stream);
      if (r != ncclSuccess) return r;
      continue;
    }
    lists[t.nSrcs - 1].push_back(&t);
  }
  const nbxDevRedOpFull lop = wideScalarOp(op);
  const bool useList = batchListEnabled();
  for (int q = 0; q < kMaxKSrcs; q++) {
    if (lists[q].empty()) continue;
    const int ns = q + 1;
    size_t done = 0;
    if (useList) {
      r = launchBatchList(ws.batchList[out32 ? 1 : 0][q], (int)eb, kFamWideBatchList, out32 ? kLaunchOut32 : 0, ns,
                          lists[q], lop, preMask(pre, nPreOpSrcs, 0, ns, 0), 0, 0, st, &done);
      if (r != ncclSuccess) return r;
    }
    // the rest one launch each (work lists off, or no table slot free)
    for (size_t j = done; j < lists[q].size(); j++) {
      const nbxReduceTask& t = *lists[q][j];
      r = nbxReduceMultiWide(t.dsts, t.nDsts, t.srcs, t.nSrcs, t.count, srcType, dstType, op, nPreOpSrcs, stream);
      if (r != ncclSuccess) return r;
    }
  }
  return ncclSuccess;
}

NBX_EXPORT int nbxDebugSetBatchMode(int mode) { return g_batchMode.set(mode, mode >= 0 && mode <= 2); }

// Slots of the device's work-list arena by state (free / eager / graph-owned; 3: fallbacks).
NBX_EXPORT int nbxDebugBatchListSlots(int dev, int state) {
  if (dev < 0 || dev >= kMaxDevices) return -1;
  ListArena& A = g_lists[dev];
  std::lock_guard<std::mutex> lk(A.mu);
  if (state == 3) return (int)A.fallbacks.load();
  if (A.base == nullptr) return state == 0 ? kListSlots : 0;
  int n = 0;
  for (auto& s : A.state) n += s.load() == state;
  return n;
}
