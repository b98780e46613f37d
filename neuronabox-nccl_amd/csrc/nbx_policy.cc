// nbx_policy.cc — what every launcher of the reduction core asks before a
// launch: the launch-configuration knobs, the device of a stream, the
// per-(device, stream) tile counters of the dynamic schedules, and the launch
// record (nbx_launch.h).
#include <cstdlib>
#include <mutex>
#include <unordered_map>
#include <utility>

#include "nbx_launch.h"

namespace nbx {
namespace {
// Launch configuration (NCCL_NTHREADS / NCCL_MAX_NCHANNELS analogues).
std::atomic<int> g_maxBlocksPerCU{0};   // 0 = default per variant
std::atomic<int> g_variant{0};          // 0 = auto, 1 = force small tile, 2 = force big tile

// Workgroups per CU fixed by nbxSetLaunchConfig, else by NBX_BLOCKS_PER_CU; 0: neither.
int fixedBlocksPerCU() {
  static const int env = envInt("NBX_BLOCKS_PER_CU", 0);
  const int v = g_maxBlocksPerCU.load(std::memory_order_relaxed);
  return v > 0 ? v : env > 0 ? env : 0;
}

std::atomic<int> g_cuCount[kMaxDevices];
}  // namespace

int envInt(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return (v && *v) ? std::atoi(v) : dflt;
}

int cuCount(int dev) {
  if (dev < 0 || dev >= kMaxDevices) return 256;
  int c = g_cuCount[dev].load(std::memory_order_relaxed);
  if (c > 0) return c;
  if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
  g_cuCount[dev].store(c, std::memory_order_relaxed);
  return c;
}

int launchVariant() { return g_variant.load(std::memory_order_relaxed); }

bool launchPolicyOverridden() { return fixedBlocksPerCU() > 0; }

// Workgroups per CU: big tiles keep ~32 dwordx4 loads in flight per lane
// slot — one 256-thread workgroup per CU (4 waves, ~128 KiB in flight per CU)
// when nSrcs x U >= 32, proportionally more when the unroll is capped. Small
// tiles (one pack per lane per source): 5 / 4 / 3 workgroups per CU for 1 / 2
// / 3 sources, 4 above — measured on MI355X (profiles/r1/tiles_sweep_r1n.jsonl:
// 2 sources at 256 MiB 6.80 TB/s with 4 per CU vs 6.12 with 8 and 5.91 with
// one big-tile workgroup; 3 sources 6.58 vs 6.38 big-tile). classic = true
// keeps 8 small workgroups per CU: the element kernel, and passes that read
// peer GPUs' memory (the collectives' direct and ring schedules) — xGMI
// latency wants more bytes in flight, and the local-HBM measurement does not
// carry over (no multi-GPU box to measure it on).
int maxBlocksPerCU(bool big, int loadsPerLane, bool classic) {
  if (const int v = fixedBlocksPerCU()) return v;
  if (!big) {
    if (classic) return 8;
    return loadsPerLane <= 1 ? 5 : loadsPerLane == 2 ? 4 : loadsPerLane == 3 ? 3 : 4;
  }
  int b = (32 + loadsPerLane - 1) / loadsPerLane;
  return b < 1 ? 1 : (b > 8 ? 8 : b);
}

// Realigning kernels: 8 workgroups per CU for the run-time-count kernel
// (profiles/r1/sweep_shift.txt); per source count, the LDS-DMA kernel's
// shiftLdsBlocksPerCU (profiles/r2/sweep_shift_256MiB_r2f.txt).
int shiftedBlocksPerCU(bool perCount, int nSrcs) {
  if (const int v = fixedBlocksPerCU()) return v;
  if (!perCount) return 8;
  return shiftLdsBlocksPerCU(nSrcs);
}

// The device a launch on `st` runs on (the per-device arenas and tile
// counters must live there): the stream's own device, the current one for
// the null / per-thread stream.
int launchDevice(hipStream_t st) {
  if (st != nullptr && st != hipStreamPerThread) {
    hipDevice_t d = 0;
    if (hipStreamGetDevice(st, &d) == hipSuccess) return (int)d;
  }
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev;
}

namespace {
// A stream may take a dynamic schedule: not while it is being captured (a
// replay would reuse a stale base, and may run on any stream), not
// hipStreamPerThread (one handle, many streams), not with NBX_DYNAMIC_TILES=0.
bool dynEligible(int dev, hipStream_t st) {
  static const int on = envInt("NBX_DYNAMIC_TILES", 1);
  if (!on || dev < 0 || dev >= kMaxDevices || st == hipStreamPerThread) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone;
}

// kWords counters per (device, stream) for up to kSlots streams of a device,
// in device memory allocated on first use; a stream's counters are zeroed in
// that stream's own order, ahead of its first launch (a memset on the null
// stream would not order a non-blocking stream's kernel after it).
// Keyed by the stream handle. HIP hands a destroyed stream's handle to the
// next stream created (63 of 64 create / destroy cycles), but hipStreamDestroy
// returns only once the stream's work has completed (20 ms of pending kernels:
// destroy took 21.4 ms on the ROCm 7.2 runtime, 39 ms on torch's 7.0 runtime,
// nothing left running after it; scripts/probe_stream_id.hip,
// scripts/probe_stream_destroy.py, profiles/r3/probe_stream_*_r3f.log). So a
// new stream that inherits a handle inherits an idle counter whose value is
// the base the host tracks, and streams created per iteration keep reusing
// the same few counters (tests/test_reduce_gpu.py::
// test_dynamic_counters_with_stream_churn).
template <size_t kWords, int kSlots>
struct CounterPool {
  typedef std::pair<uint32_t*, uint32_t> Slot;   // (counters, base tracked by the host; 0 where the kernel resets)
  std::mutex mu;
  uint32_t* pool = nullptr;
  int used = 0;
  bool failed = false;
  std::unordered_map<hipStream_t, Slot> slots;

  // The stream's slot; nullptr when the pool cannot be allocated, is used up,
  // or the zeroing fails. Call with mu held.
  Slot* slotFor(int dev, hipStream_t st) {
    if (pool == nullptr) {
      if (failed) return nullptr;
      CurDev cur(dev);
      void* p = nullptr;
      if (hipMalloc(&p, (size_t)kSlots * kWords * sizeof(uint32_t)) != hipSuccess) {
        failed = true;
        return nullptr;
      }
      pool = (uint32_t*)p;
    }
    auto it = slots.find(st);
    if (it != slots.end()) return &it->second;
    if (used >= kSlots) return nullptr;
    uint32_t* c = pool + (size_t)used * kWords;
    if (hipMemsetAsync(c, 0, kWords * sizeof(uint32_t), st) != hipSuccess) return nullptr;
    used++;
    return &slots.emplace(st, Slot(c, 0u)).first->second;
  }
  int usedSlots() {
    std::lock_guard<std::mutex> lk(mu);
    return used;
  }
};

// Dynamic tiles (kernels' forEachTile): one 32-bit counter per (device,
// stream) in device memory. Every launch on a stream advances its counter by
// exactly its tile count, so the host knows each launch's base without the
// kernel resetting anything; launches on one stream run in order, so no two
// launches ever share a counter concurrently. The lock is held from reading
// the base to the launch, so calls racing on one stream from several threads
// still enqueue in base order.
CounterPool<1, 4096> g_dyn[kMaxDevices];

// Class counters of the realigning kernel's dynamic schedule: kShiftDynClasses
// counters kShiftDynStride words apart per (device, stream). The kernel resets
// each class counter on its last fetch, so a launch always starts from zero
// and the host tracks no base; launches on one stream run in order, so no two
// share a block at once. Static schedule once the 64 blocks are used up.
CounterPool<(size_t)kShiftDynClasses * kShiftDynStride, 64> g_shiftDyn[kMaxDevices];

int parseDynMinTiles() {
  const int e = envInt("NBX_DYN_MIN_TILES_PER_WG", 16);
  return e < 1 ? 1 : e;
}
// Tiles per workgroup from which a big-tile launch is dynamic (launchPass);
// env NBX_DYN_MIN_TILES_PER_WG, nbxDebugSetDynMinTiles.
LazySetting<int> g_dynMinTiles{0, parseDynMinTiles};

constexpr int kLaunchLogCap = 64;
struct LaunchLog {
  int32_t rec[kLaunchLogCap][4];
  uint64_t n;
};
thread_local LaunchLog t_launchLog;   // host stores only; nothing reads it but the test hook
}  // namespace

int dynMinTilesPerWG() { return g_dynMinTiles.get(); }

uint32_t* shiftDynCounters(int dev, hipStream_t st) {
  if (!dynEligible(dev, st)) return nullptr;
  auto& D = g_shiftDyn[dev];
  std::lock_guard<std::mutex> lk(D.mu);
  auto* slot = D.slotFor(dev, st);
  return slot ? slot->first : nullptr;
}

bool DynLaunch::begin(int dev, hipStream_t st, uint64_t nTiles, KArgs& a) {
  if (nTiles == 0 || nTiles > 0xffffffffull || !dynEligible(dev, st)) return false;
  auto& D = g_dyn[dev];
  lk_ = std::unique_lock<std::mutex>(D.mu);
  slot_ = D.slotFor(dev, st);
  if (slot_ == nullptr) {
    lk_.unlock();
    return false;
  }
  tiles_ = nTiles;
  a.dynCtr = slot_->first;
  a.dynBase = slot_->second;
  return true;
}

void DynLaunch::done(bool launched) {
  if (slot_ && launched) slot_->second += (uint32_t)tiles_;   // mod 2^32, as the kernel's arithmetic
  slot_ = nullptr;
  if (lk_.owns_lock()) lk_.unlock();
}

void logLaunch(int family, int nSrcs, int unroll, int flags) {
  int32_t* r = t_launchLog.rec[t_launchLog.n++ % kLaunchLogCap];
  r[0] = family;
  r[1] = nSrcs;
  r[2] = unroll;
  r[3] = flags;
}
void logCollLaunch(int family, int nRanks, int unroll, int flags) { logLaunch(family, nRanks, unroll, flags); }
}  // namespace nbx

using namespace nbx;

NBX_EXPORT ncclResult_t nbxSetLaunchConfig(int blocksPerCU, int variant) {
  if (blocksPerCU < 0 || blocksPerCU > 64 || variant < 0 || variant > 2) return ncclInvalidArgument;
  g_maxBlocksPerCU.store(blocksPerCU);
  g_variant.store(variant);
  return ncclSuccess;
}

NBX_EXPORT ncclResult_t nbxGetLaunchConfig(int* blocksPerCU, int* variant) {
  if (blocksPerCU) *blocksPerCU = g_maxBlocksPerCU.load();
  if (variant) *variant = g_variant.load();
  return ncclSuccess;
}

NBX_EXPORT int nbxDebugDynStreamSlots(int device, int which) {
  if (device < 0 || device >= kMaxDevices) return -1;
  return which == 0 ? g_dyn[device].usedSlots() : g_shiftDyn[device].usedSlots();
}

NBX_EXPORT int nbxDebugLaunchLog(int32_t* out, int maxRecords) {
  const LaunchLog& L = t_launchLog;
  const uint64_t total = L.n;
  uint64_t k = total < (uint64_t)kLaunchLogCap ? total : (uint64_t)kLaunchLogCap;
  if (out == nullptr || maxRecords <= 0) k = 0;
  else if ((uint64_t)maxRecords < k) k = (uint64_t)maxRecords;
  for (uint64_t i = 0; i < k; i++)
    std::memcpy(out + 4 * i, L.rec[(total - k + i) % kLaunchLogCap], sizeof(L.rec[0]));
  return total > 0x7fffffffull ? 0x7fffffff : (int)total;
}

NBX_EXPORT void nbxDebugLaunchLogReset(void) { t_launchLog.n = 0; }

NBX_EXPORT int nbxDebugSetDynMinTiles(int tilesPerWG) { return g_dynMinTiles.set(tilesPerWG, tilesPerWG >= 1); }
