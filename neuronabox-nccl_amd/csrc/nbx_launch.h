// nbx_launch.h — what the host units of the reduction core share: the kernel
// tables, the launch policy, the launch record, and the one copy of every rule
// that more than one launcher follows (the communicator layer: nbx_internal.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/nbx_reduce.h"
#include "nbx_registry.h"
#include "nbx_internal.h"

#ifndef NBX_EXPORT
#define NBX_EXPORT extern "C" __attribute__((visibility("default")))
#endif

namespace nbx {

const KernelTable& table();       // nbx_reduce.cc
const WideTable& wideTable();     // nbx_reduce_wide.cc
int typeSize(int dt);             // bytes of an ncclDataType_t, -1 unknown (nbx_reduce.cc)

// ---- launch policy, device and stream helpers (nbx_policy.cc) ----
constexpr int kMaxDevices = 64;
int envInt(const char* name, int dflt);
int cuCount(int dev);
int launchDevice(hipStream_t st);
int launchVariant();   // nbxSetLaunchConfig: 0 = auto, 1 = force small tile, 2 = force big tile
int maxBlocksPerCU(bool big, int loadsPerLane, bool classic = false);
int shiftedBlocksPerCU(bool perCount, int nSrcs);
// NBX_BLOCKS_PER_CU or nbxSetLaunchConfig fixes the workgroups per CU: the
// per-functor and mid-size adjustments of the big tile stand back.
bool launchPolicyOverridden();
int dynMinTilesPerWG();
uint32_t* shiftDynCounters(int dev, hipStream_t st);

// Makes `dev` current for an allocation, restoring the caller's device.
struct CurDev {
  int prev = -1;
  explicit CurDev(int dev) {
    if (hipGetDevice(&prev) != hipSuccess || prev == dev || hipSetDevice(dev) != hipSuccess) prev = -1;
  }
  ~CurDev() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// A setting read from the environment on first use (`parse`), overridable by
// a debug hook. `unset` is a value no parse and no hook ever stores.
template <class T>
class LazySetting {
 public:
  constexpr LazySetting(T unset, T (*parse)()) : v_(unset), unset_(unset), parse_(parse) {}
  T get() {
    T v = v_.load(std::memory_order_relaxed);
    if (v == unset_) {
      T expect = unset_;
      v_.compare_exchange_strong(expect, parse_());
      v = v_.load();
    }
    return v;
  }
  // the hooks' contract: returns the previous value; input out of range only queries
  T set(T v, bool inRange) {
    const T prev = get();
    if (inRange) v_.store(v);
    return prev;
  }

 private:
  std::atomic<T> v_;
  const T unset_;
  T (*const parse_)();
};

// Launch record (include/nbx_debug.h nbxDebugLaunchLog): the newest passes
// launched from this thread, as {family, nSrcs, unroll, flags}. The
// collective launches (comm_mp_launch.cc, families 8-12 in nbx_internal.h)
// append to the same log through nbx::logCollLaunch.
enum LaunchFamily {
  kFamSmallPacks = 1, kFamBigPacks = 2, kFamElts = 3, kFamShiftedLds = 4, kFamShifted = 5, kFamWidePacks = 6,
  kFamWideElts = 7,
  kFamBatch = 13, kFamBatchList = 14,   // batched buckets: flags bits kLaunchSegsShift.. = buckets of the launch
  kFamWideBatchList = 15,               // the same for nbxReduceMultiWideBatch (bit 1: fp32 output)
  kFamWideShiftedLds = 16               // wide realigning LDS-DMA (kWideShiftedLds)
};
enum LaunchFlag { kLaunchDynamic = 1, kLaunchOut32 = 2, kLaunchPartFirst = 4 };
void logLaunch(int family, int nSrcs, int unroll, int flags);

// Argument checks the batched entry points share with the single ones.
ncclResult_t checkOp(ncclDataType_t datatype, const nbxDevRedOpFull& op, const KernelSet** ks);
ncclResult_t checkWideOp(ncclDataType_t srcType, ncclDataType_t dstType, const nbxDevRedOpFull& op);
ncclResult_t checkBucket(size_t eb, size_t deb, bool apart, void* const* dsts, int nDsts, const void* const* srcs,
                         int nSrcs, size_t count);
// Layouts of an fp32-accumulating call (wideLayout; nbxDebugWideLayout returns
// these values).
enum WideLayout { kWideLayoutElts = 0, kWideLayoutPacks = 1, kWideLayoutShifted = 2 };
int wideLayout(size_t eb, size_t deb, void* const* dsts, int nDsts, const void* const* srcs, int nSrcs, size_t count,
               size_t* head);
// The op as the wide kernels take it: their scalar is an fp32 value, and only
// PreMulSum has one — zero without it, the low 32 bits when passed by value.
nbxDevRedOpFull wideScalarOp(nbxDevRedOpFull op);

// ---- rules shared by the launchers ----
inline bool overlaps(const void* a, size_t aBytes, const void* b, size_t bBytes) {
  uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bBytes && y < x + aBytes;
}

// Source and destination counts in range, neither array NULL.
inline bool argArraysOk(void* const* dsts, int nDsts, const void* const* srcs, int nSrcs) {
  return nSrcs >= 1 && nSrcs <= NBX_MAX_SRCS && nDsts >= 1 && nDsts <= NBX_MAX_DSTS && srcs && dsts;
}
// Every pointer non-null and aligned to its element size (eb sources, deb destinations).
inline bool pointersOk(size_t eb, size_t deb, void* const* dsts, int nDsts, const void* const* srcs, int nSrcs) {
  for (int s = 0; s < nSrcs; s++)
    if (srcs[s] == nullptr || ((uintptr_t)srcs[s] % eb) != 0) return false;
  for (int d = 0; d < nDsts; d++)
    if (dsts[d] == nullptr || ((uintptr_t)dsts[d] % deb) != 0) return false;
  return true;
}
// The address modulo 16 that p[0 .. n) share (-1: they differ).
inline int sharedMis16(const void* const* p, int n) {
  const unsigned mis = (unsigned)((uintptr_t)p[0] & 15u);
  for (int i = 1; i < n; i++)
    if (((uintptr_t)p[i] & 15u) != mis) return -1;
  return (int)mis;
}
// The same over every pointer of a bucket.
inline int sharedMisalignment(void* const* dsts, int nDsts, const void* const* srcs, int nSrcs) {
  const int mis = sharedMis16(srcs, nSrcs);
  return mis >= 0 && sharedMis16(dsts, nDsts) == mis ? mis : -1;
}

// The scalar of the op: by value, or a device pointer the kernel dereferences.
// A: KArgs, BatchArgs, BatchListArgs, LLArgs, SimpleArgs.
template <class A>
inline void setScalarArg(A& a, const nbxDevRedOpFull& op) {
  a.arg = op.scalarArgIsPtr ? 0 : op.scalarArg;
  a.argPtr = op.scalarArgIsPtr ? (const void*)(uintptr_t)op.scalarArg : nullptr;
}

// PreMulSum's pre-op mask of one pass: the caller's sources [firstSrc,
// firstSrc + n) sit in kernel slots slot0 ...; those below nPreOpSrcs get it.
inline uint32_t preMask(bool pre, int nPreOpSrcs, int firstSrc, int n, int slot0) {
  uint32_t m = 0;
  if (pre)
    for (int k = 0; k < n; k++)
      if (firstSrc + k < nPreOpSrcs) m |= 1u << (slot0 + k);
  return m;
}

// The fields every single-bucket pass sets the same way.
inline void fillKArgs(KArgs& a, void* const* dsts, int nDsts, const void* const* srcs, int nSrcs, size_t count,
                      const nbxDevRedOpFull& op, uint32_t mask) {
  std::memset(&a, 0, sizeof(a));
  for (int s = 0; s < nSrcs; s++) a.src[s] = srcs[s];
  for (int d = 0; d < kMaxKDsts; d++) a.dst[d] = dsts[d < nDsts ? d : 0];
  a.nElts = count;
  setScalarArg(a, op);
  a.preMask = mask;
  a.nSrcs = nSrcs;
  a.nDsts = nDsts;
}

// Workgroups of a tiled launch: one per tile up to the cap, at least one.
inline size_t cappedGrid(size_t tiles, size_t maxBlocks) {
  const size_t grid = tiles < maxBlocks ? tiles : maxBlocks;
  return grid == 0 ? 1 : grid;
}

// Body of a pack launch: the elements behind the head (at most count) as
// 16-byte packs, cut() into tiles of `tile` packs for at most maxBlocks
// (CUs x workgroups per CU) workgroups.
struct Body {
  size_t head, nPacks, tiles = 0, grid = 0;
  Body(size_t count, size_t headElts, int epp)
      : head(headElts < count ? headElts : count), nPacks((count - head) / (size_t)epp) {}
  size_t tilesOf(size_t tile) const { return (nPacks + tile - 1) / tile; }
  void cut(size_t tile, size_t maxBlocks) {
    tiles = tilesOf(tile);
    grid = cappedGrid(tiles, maxBlocks);
  }
  void into(KArgs& a) const {
    a.headElts = (int)head;
    a.nPacks = nPacks;
  }
};

// "This call runs big tiles" (launchPass) and "this bucket fills the GPU
// alone, so it leaves the batch" (both batched entry points): the launch
// variant when forced; else 4+ sources (or peer-memory sources) whose `packs`
// give every CU a big tile. The callers count differently, and every size at
// which they disagree is a decision taken today, so the difference stays:
//   launchPass      packs behind its 128-byte peel; a partial tile counts
//   per-step batch  count / epp, head included; whole tiles only
//   wide batch      (count - head) / epp behind its 16-byte head; whole tiles
// (a bucket within a tile of the threshold stays batched where launchPass
// alone would give it big tiles).
inline bool bigTileRule(int force, int nSrcs, bool acquireSystem, uint64_t packs, uint64_t bigTile, uint64_t cus,
                        bool partialTileCounts) {
  if (force != 0) return force == 2;
  const uint64_t tiles = partialTileCounts ? (packs + bigTile - 1) / bigTile : packs / bigTile;
  return (nSrcs > 3 || acquireSystem) && tiles >= cus;
}

// > kMaxKSrcs sources: an ordered left fold in passes of 8 + 7 + 7 ...
//   pass 0: part = fold(srcs[0..8)); pass k: part = fold(part, next <= 7 srcs);
//   the last pass writes every destination.
// The caller places the partial (`part`; `scratch` != nullptr is freed in
// stream order after the last pass, even a failing one — the first error is
// the one reported) and launches one pass:
//   pass(dsts, nDsts, srcs, n, first, partFirst, last)
// with `first` the index of the first caller source among srcs (srcs[0] is the
// partial when partFirst). The fold stops at the first failing pass.
template <class Pass>
inline ncclResult_t foldPasses(void* const* dsts, int nDsts, const void* const* srcs, int nSrcs, void* part,
                               void* scratch, hipStream_t stream, Pass&& pass) {
  void* partDst[1] = {part};
  ncclResult_t r = pass(partDst, 1, srcs, kMaxKSrcs, 0, false, false);
  int next = kMaxKSrcs;
  while (r == ncclSuccess && next < nSrcs) {
    const void* ps[kMaxKSrcs];
    ps[0] = part;
    const int first = next;
    int n = 1;
    while (n < kMaxKSrcs && next < nSrcs) ps[n++] = srcs[next++];
    const bool last = next >= nSrcs;
    r = pass(last ? dsts : partDst, last ? nDsts : 1, ps, n, first, true, last);
  }
  if (scratch != nullptr && hipFreeAsync(scratch, stream) != hipSuccess && r == ncclSuccess) r = ncclUnhandledCudaError;
  return r;
}

}  // namespace nbx
