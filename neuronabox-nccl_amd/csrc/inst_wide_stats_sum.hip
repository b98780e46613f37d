#include "../../include/nbx_reduce.h"
#include "nbx_registry.h"
#include "nbx_wide.h"
namespace nbx {
namespace {
// A workgroup's sum of slots [lo, hi) in a tree fixed by the slot index alone:
// lane t adds slots lo + t, lo + t + kBlock, ... in that order, the wave folds
// over the xor butterfly of wideStatsFlush, and the four wave results are
// added in wave order. Every thread returns the same {sumSq, amax}.
__device__ __forceinline__ WideSlot sumSlots(const WideSlot* slots, uint64_t lo, uint64_t hi) {
  __shared__ WideSlot waveSum[kBlock / 64];
  double s = 0.0;
  float m = 0.0f;
  for (uint64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
    const WideSlot v = slots[i];
    s = s + v.sumSq;
    m = __builtin_fmaxf(m, v.amax);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s = s + __shfl_xor(s, o, 64);
    m = __builtin_fmaxf(m, __shfl_xor(m, o, 64));
  }
  if ((threadIdx.x & 63u) == 0) waveSum[threadIdx.x >> 6] = WideSlot{s, m, 0u};
  __syncthreads();
  WideSlot r = waveSum[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; w++) {
    r.sumSq = r.sumSq + waveSum[w].sumSq;
    r.amax = __builtin_fmaxf(r.amax, waveSum[w].amax);
  }
  return r;
}

// The caller's record. The slots' max dropped every NaN and the square-sum
// kept it, so amax is a NaN exactly when sumSq is.
__device__ __forceinline__ void storeStats(nbxWideStats* out, const WideSlot& r) {
  nbxWideStats o;
  o.sumSq = r.sumSq;
  o.amax = r.sumSq != r.sumSq ? __uint_as_float(0x7fc00000u) : r.amax;
  o.reserved = 0u;
  *out = o;
}

// One level of the single call's tree: workgroup j sums slots
// [j * kWideStatsFan, ...) of `in` into next[j], or — the last level, one
// workgroup — into the caller's record. n = 0 writes zeros.
__global__ __launch_bounds__(kBlock) void kWideStatsReduce(const WideSlot* in, uint64_t n, WideSlot* next,
                                                           nbxWideStats* out) {
  const uint64_t lo = (uint64_t)blockIdx.x * kWideStatsFan;
  const uint64_t hi = lo + kWideStatsFan < n ? lo + kWideStatsFan : n;
  const WideSlot r = sumSlots(in, lo, hi);
  if (threadIdx.x == 0) {
    if (out != nullptr) storeStats(out, r);
    else next[blockIdx.x] = r;
  }
}

// The batch: workgroup r sums record r's slots (nbx_kargs.h WideStatsBatchArgs).
__global__ __launch_bounds__(kBlock) void kWideStatsBatch(WideStatsBatchArgs a) {
  const uint32_t r = blockIdx.x;
  const uint64_t begin = r ? a.tileEnd[r - 1] : 0;
  const WideSlot v = sumSlots(a.slots, begin * (kBlock / 64) + r, (uint64_t)a.tileEnd[r] * (kBlock / 64) + r + 1);
  if (threadIdx.x == 0) storeStats((nbxWideStats*)a.stats + a.statIdx[r], v);
}
}  // namespace

WideStatsKernels wideStatsKernels() {
  return WideStatsKernels{(const void*)&kWideStatsReduce, (const void*)&kWideStatsBatch};
}

void fillWideStats(WideStatsTable& t) {
  fillWideStats16(t);
  fillWideStats8(t);
  fillWideStatsShift16(t);
  fillWideStatsShift8(t);
}
}  // namespace nbx
