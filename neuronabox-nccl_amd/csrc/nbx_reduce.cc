// nbx_reduce.cc — host side of the reduction core: the C ABI of
// include/nbx_reduce.h, argument checks, pointer alignment analysis, one
// kernel pass and the multi-pass fold for > 8 sources. The policy it asks and
// the rules it shares with the other launchers: nbx_launch.h.
//
// Reference behaviour mirrored:
//   * alignment fallback — reduceCopy checks every pointer for 16-B alignment
//     and otherwise runs sizeof(T) packs (common_kernel.h:209-238). Here the
//     fast kernel also accepts pointers that share ONE misalignment modulo 16
//     (peeling < 16 B of head elements), so only genuinely mixed alignments
//     take the element kernel.
//   * opArg: by value, or a device pointer dereferenced by the kernel
//     (ncclScalarDevice; common.h:100-119, onerank.cu:32-42).
//   * PreOp on sources s < nPreOpSrcs, postOp after the fold
//     (common_kernel.h:79-137).
#include <cstdio>
#include <mutex>

#include "nbx_launch.h"

namespace nbx {
namespace {

KernelTable g_table;
std::once_flag g_tableOnce;

bool isFloatType(int dt) {
  return dt == ncclFloat16 || dt == ncclFloat32 || dt == ncclFloat64 || dt == ncclBfloat16 ||
         dt == ncclFloat8e4m3 || dt == ncclFloat8e5m2;
}

// Elements folded one by one before the 16-B pack body, so that the body of
// dsts[0] starts on a 128-B cache-line boundary (NBX_PEEL_BYTES: 16 keeps
// the smallest peel). Streams that start mid-line cost every wave
// instruction a partial line at each end: all pointers one element off ran
// 9 % slower at 256 MiB per input than aligned ones with a 16-B peel, and a
// destination body on a line boundary gains 2-5 % for the realigning kernels
// (profiles/r2/realign_probe_r2d.jsonl, sweep_shift_256MiB_r2d.txt).
size_t peelElts(uintptr_t dst, int eb) {
  static const unsigned line = [] {
    const int v = envInt("NBX_PEEL_BYTES", 128);
    return (unsigned)(v == 16 || v == 32 || v == 64 || v == 128 || v == 256 ? v : 128);
  }();
  const unsigned mis = (unsigned)(dst & (line - 1));
  return mis ? (size_t)((line - mis) / (unsigned)eb) : 0;
}

// One kernel pass over <= kMaxKSrcs sources.
ncclResult_t launchPass(const KernelSet& ks, void* const* dsts, int nDsts, const void* const* srcs,
                        int nSrcs, size_t count, const nbxDevRedOpFull& op, uint32_t mask,
                        int postOp, int acquireSystem, hipStream_t stream) {
  KArgs a;
  fillKArgs(a, dsts, nDsts, srcs, nSrcs, count, op, mask);
  a.acquireSystem = acquireSystem;
  a.postOp = postOp;

  const int eb = ks.eltBytes;
  const int epp = 16 / eb;
  const int dev = launchDevice(stream);
  const int cus = cuCount(dev);
  void* args[] = {&a};
  hipError_t err;
  if (sharedMisalignment(dsts, nDsts, srcs, nSrcs) >= 0) {
    Body b(count, peelElts((uintptr_t)dsts[0], eb), epp);
    b.into(a);
    // big tiles once every CU gets at least one, for 4+ sources; small tiles
    // below that, and always for 1-3 sources (more workgroups per CU beat
    // deeper unrolling when a quarter or more of the traffic is stores:
    // profiles/r1/tiles_sweep_r1n.jsonl)
    const size_t bigTile = (size_t)ks.unroll[nSrcs - 1] * kBlock;
    const bool big = bigTileRule(launchVariant(), nSrcs, acquireSystem != 0, b.nPacks, bigTile, (uint64_t)cus,
                                 /*partialTileCounts=*/true);
    const size_t tile = big ? bigTile : (size_t)kBlock;
    int perCU = maxBlocksPerCU(big, nSrcs * (big ? ks.unroll[nSrcs - 1] : 1), acquireSystem != 0);
    // Few big tiles per CU (config C's mid-size buckets): one tile per
    // workgroup, up to NBX_MID_BLOCKS_PER_CU workgroups per CU, so every tile's
    // loads are in flight at once instead of a workgroup's second tile waiting
    // for its first tile's fold (scripts/steps/r4-o.txt, r4-p.txt)
    static const int midPerCU = envInt("NBX_MID_BLOCKS_PER_CU", 4);
    if (big && !launchPolicyOverridden()) {
      if (perCU < ks.bigBlocksPerCU) perCU = ks.bigBlocksPerCU;   // VALU-heavy functors: a second wave per SIMD
      const size_t need = (b.tilesOf(tile) + (size_t)cus - 1) / (size_t)cus;
      if (midPerCU > 1 && need > (size_t)perCU && need <= (size_t)midPerCU) perCU = (int)need;
    }
    b.cut(tile, (size_t)cus * (size_t)perCU);
    a.variant = big ? 1 : 0;
    // dynamic tiles for big tiles only: small tiles (1-3 sources, 3-5
    // workgroups per CU, 16x the atomics) collapse to 0.7-1.4 TB/s on the
    // counter's contention (profiles/r2/probe_dyn_r2x.jsonl), and fetching
    // chunks of 4-16 consecutive small tiles per atomic still lost 15-60 % to
    // the static grid stride (profiles/r2/probe_dyn_small_chunk_r3k.jsonl).
    // And only for launches of >= 16 tiles per workgroup: every workgroup's
    // fetch goes to one address, and device-scope atomics on one address
    // serialize (~11 ns each), so the launch's first and last round of
    // fetches — one per workgroup, all at once — add ~3 us, which only long
    // launches win back (8 x fp32 sources: 4 MiB per input 7.50 vs 4.71 us
    // static, 16 MiB 27.4 vs 24.4 us, 64 MiB 97.4 vs 98.1, 256 MiB 376 vs 395;
    // scripts/sweep_dyn_xcd.hip, profiles/r2/sweep_dyn_xcd_r4e.txt,
    // profiles/r2/probe_mid_sizes_r4d.jsonl)
    DynLaunch dyn;
    if (big && b.tiles >= (size_t)dynMinTilesPerWG() * b.grid) dyn.begin(dev, stream, b.tiles, a);
    err = hipLaunchKernel((const void*)ks.packs[big ? 1 : 0][nSrcs - 1], dim3((unsigned)b.grid), dim3(kBlock), args,
                          0, stream);
    logLaunch(big ? kFamBigPacks : kFamSmallPacks, nSrcs, big ? ks.unroll[nSrcs - 1] : 1,
              a.dynCtr != nullptr ? kLaunchDynamic : 0);
    dyn.done(err == hipSuccess);
  } else if (sharedMis16(dsts, nDsts) >= 0 && ks.shifted != nullptr) {
    // destinations share one alignment: 16-B packs on their side, the
    // sources realigned in registers (kReduceShifted)
    Body b(count, peelElts((uintptr_t)dsts[0], eb), epp);
    b.into(a);
    // one kernel per source count staging the sources through LDS by
    // LDS-DMA (profiles/r2/sweep_shift_256MiB_r2f.txt);
    // NBX_SHIFT_N=0 or launch variant 1 (small tiles) selects the
    // run-time-count register kernel (1 pack per lane, 8 workgroups/CU)
    static const int useN = envInt("NBX_SHIFT_N", 1);
    const bool small = launchVariant() == 1;
    const void* fn = (useN && !small) ? ks.shiftedN[nSrcs - 1] : nullptr;
    const size_t tile = fn ? (size_t)shiftLdsUnroll(nSrcs) * 64 * kShiftLdsWaves : (size_t)kBlock;
    b.cut(tile, (size_t)cus * (size_t)shiftedBlocksPerCU(fn != nullptr, nSrcs));
    const size_t blocks = b.tiles ? b.tiles : 1;   // a body below one pack counts as one tile here
    const unsigned threads = fn ? (unsigned)(kShiftLdsWaves * 64) : (unsigned)kBlock;
    // dynamic schedule for long eager launches from 3 sources, over
    // kShiftDynClasses class counters (kReduceShiftedLds): one counter for
    // all workgroup tiles ran 1.1-4.9 TB/s here — 4-8x the big kernel's
    // atomics on one address (profiles/r2/realign_dyn_r3a.jsonl). At 256 MiB
    // per input the classes give 8 sources +4.7 %, 4 sources +1.1 % over
    // the static stride; 2 sources (1-pack wave tiles, 2 workgroups per CU:
    // 8x the fetches per byte) lost 28 % to the counters' contention, so
    // they stay static (profiles/r2/realign_probe_r4q.jsonl)
    if (fn && nSrcs >= 3 && blocks >= (size_t)dynMinTilesPerWG() * b.grid) a.dynCtr = shiftDynCounters(dev, stream);
    const bool perCount = fn != nullptr;
    if (!fn) fn = ks.shifted;
    err = hipLaunchKernel(fn, dim3((unsigned)b.grid), dim3(threads), args, 0, stream);
    logLaunch(perCount ? kFamShiftedLds : kFamShifted, nSrcs, perCount ? shiftLdsUnroll(nSrcs) : 1,
              a.dynCtr != nullptr ? kLaunchDynamic : 0);
  } else {
    const size_t blocks = (count + kBlock - 1) / kBlock;
    const size_t grid = cappedGrid(blocks, (size_t)cus * (size_t)maxBlocksPerCU(false, nSrcs, /*classic=*/true));
    err = hipLaunchKernel((const void*)ks.elts, dim3((unsigned)grid), dim3(kBlock), args, 0, stream);
    logLaunch(kFamElts, nSrcs, 1, 0);
  }
  if (err != hipSuccess) {
    std::fprintf(stderr, "nbx: kernel launch failed: %s\n", hipGetErrorString(err));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}

}  // namespace

const KernelTable& table() {
  std::call_once(g_tableOnce, [] {
    std::memset(&g_table, 0, sizeof(g_table));
    for (auto fill : {fillInt8, fillInt32, fillInt64, fillF16, fillBF16, fillF32, fillF64, fillFp8}) fill(g_table);
  });
  return g_table;
}

int typeSize(int dt) {
  switch (dt) {
    case ncclInt8: case ncclUint8: case ncclFloat8e4m3: case ncclFloat8e5m2: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return -1;
  }
}

// Datatype / op checks shared by the single and batched entry points; on
// success *ks is the functor's kernel set.
ncclResult_t checkOp(ncclDataType_t datatype, const nbxDevRedOpFull& op, const KernelSet** ks) {
  const int dt = (int)datatype;
  if (dt < 0 || dt >= kNumTypes) return ncclInvalidArgument;
  if (op.op < 0 || op.op >= kNumDevOps) return ncclInvalidArgument;
  const KernelSet& k = table()[dt][op.op];
  if (!k.valid) return ncclInvalidArgument;   // e.g. SumPostDiv on floats
  if (op.op == nbxDevSumPostDiv && !op.scalarArgIsPtr && (int)op.scalarArg == 0) return ncclInvalidArgument;
  if (op.scalarArgIsPtr && op.scalarArg == 0) return ncclInvalidArgument;
  *ks = &k;
  return ncclSuccess;
}

// Per-bucket checks: counts of sources and destinations, non-null pointers
// aligned to their element size (eb sources, deb destinations); count == 0
// accepts anything but NULL arrays. apart (the fp32 output of narrower
// sources): no destination may touch any source — a source-type destination
// may be a source (in place), an fp32 one's elements are wider than the ones
// still to be read.
ncclResult_t checkBucket(size_t eb, size_t deb, bool apart, void* const* dsts, int nDsts, const void* const* srcs,
                         int nSrcs, size_t count) {
  if (!argArraysOk(dsts, nDsts, srcs, nSrcs)) return ncclInvalidArgument;
  if (count == 0) return ncclSuccess;
  if (!pointersOk(eb, deb, dsts, nDsts, srcs, nSrcs)) return ncclInvalidArgument;
  if (apart)
    for (int d = 0; d < nDsts; d++)
      for (int s = 0; s < nSrcs; s++)
        if (overlaps(dsts[d], count * deb, srcs[s], count * eb)) return ncclInvalidArgument;
  return ncclSuccess;
}

ncclResult_t reduceMultiEx(void* const* dsts, int nDsts, const void* const* srcs, int nSrcs, size_t count,
                           ncclDataType_t datatype, nbxDevRedOpFull op, int nPreOpSrcs, int postOp,
                           ncclStream_t stream, int flags) {
  const int acq = (flags & kReduceAcquireSystem) ? 1 : 0;
  const KernelSet* ksp = nullptr;
  if (!argArraysOk(dsts, nDsts, srcs, nSrcs)) return ncclInvalidArgument;
  ncclResult_t cr = checkOp(datatype, op, &ksp);
  if (cr != ncclSuccess) return cr;
  const KernelSet& ks = *ksp;
  if (count == 0) return ncclSuccess;
  const size_t eb = (size_t)ks.eltBytes;
  cr = checkBucket(eb, eb, false, dsts, nDsts, srcs, nSrcs, count);
  if (cr != ncclSuccess) return cr;
  if (nPreOpSrcs < 0) nPreOpSrcs = 0;
  hipStream_t st = (hipStream_t)stream;
  const bool pre = op.op == nbxDevPreMulSum;
  const int post = (op.op == nbxDevSumPostDiv && postOp) ? 1 : 0;

  if (nSrcs <= kMaxKSrcs)
    return launchPass(ks, dsts, nDsts, srcs, nSrcs, count, op, preMask(pre, nPreOpSrcs, 0, nSrcs, 0), post, acq, st);

  // > 8 sources (foldPasses): the partial lives in dsts[0] unless dsts[0]
  // overlaps a source read by a later pass — in-place collectives past 8
  // ranks put the rank's own send block (= its output) last in fold order —
  // then in stream-ordered scratch memory, so the fold order (and the result)
  // is unchanged.
  const size_t bytes = count * eb;
  bool alias = false;
  for (int s = kMaxKSrcs; s < nSrcs; s++) alias |= overlaps(dsts[0], bytes, srcs[s], bytes);
  void* part = dsts[0];
  if (alias) {
    // graph-capturable (a stream-ordered allocation node); freed after the last pass
    if (hipMallocAsync(&part, bytes, st) != hipSuccess) return ncclUnhandledCudaError;
  }
  return foldPasses(dsts, nDsts, srcs, nSrcs, part, alias ? part : nullptr, st,
                    [&](void* const* d, int nd, const void* const* s, int n, int first, bool partFirst, bool last) {
                      const int slot0 = partFirst ? 1 : 0;
                      return launchPass(ks, d, nd, s, n, count, op, preMask(pre, nPreOpSrcs, first, n - slot0, slot0),
                                        last ? post : 0, acq, st);
                    });
}
}  // namespace nbx

using namespace nbx;

NBX_EXPORT ncclResult_t nbxHostToDevRedOp(nbxDevRedOpFull* out, ncclRedOp_t op, ncclDataType_t datatype, int nRanks) {
  // enqueue.cc:1436-1512 for the built-in ops.
  if (out == nullptr) return ncclInvalidArgument;
  const int sz = typeSize((int)datatype);
  if (sz < 0) return ncclInvalidArgument;
  const int nbits = 8 * sz;
  const uint64_t allBits = ~0ull >> (64 - nbits);
  const uint64_t signBit = allBits ^ (allBits >> 1);
  out->scalarArgIsPtr = 0;
  out->scalarArg = 0;
  switch ((int)op) {
    case ncclSum: out->op = nbxDevSum; return ncclSuccess;
    case ncclProd: out->op = nbxDevProd; return ncclSuccess;
    case ncclMin:
    case ncclMax:
      out->op = nbxDevMinMax;
      if (datatype == ncclInt8 || datatype == ncclInt32 || datatype == ncclInt64) out->scalarArg ^= signBit;
      out->scalarArg ^= ((int)op == ncclMax) ? allBits : 0;
      return ncclSuccess;
    case ncclAvg: {
      if (nRanks < 1) return ncclInvalidArgument;
      if (!isFloatType((int)datatype)) {
        out->op = nbxDevSumPostDiv;
        out->scalarArg = (uint64_t)nRanks;
        return ncclSuccess;
      }
      out->op = nbxDevPreMulSum;
      const float f = (float)(1.0 / nRanks);
      uint32_t fb;
      std::memcpy(&fb, &f, 4);
      switch ((int)datatype) {
        case ncclFloat16: {  // __float2half(float(1.0/n)) — enqueue.cc:1483
          _Float16 h = (_Float16)f;
          uint16_t hb;
          std::memcpy(&hb, &h, 2);
          out->scalarArg = hb;
          break;
        }
        case ncclBfloat16: {  // __float2bfloat16(float(1.0/n)) — enqueue.cc:1488, RNE
          uint32_t u = fb + 0x7fffu + ((fb >> 16) & 1u);
          out->scalarArg = (uint16_t)(u >> 16);
          break;
        }
        case ncclFloat32: out->scalarArg = fb; break;
        case ncclFloat64: {
          double d = 1.0 / nRanks;
          std::memcpy(&out->scalarArg, &d, 8);
          break;
        }
        case ncclFloat8e4m3:
        case ncclFloat8e5m2: {
          // this build's extension: the element type's RNE encoding of float(1/n)
          // (e4m3fn: E=4,M=3,bias=7; e5m2: E=5,M=2,bias=15). 1/n <= 1, never overflows.
          const bool e4 = datatype == ncclFloat8e4m3;
          const int E = e4 ? 4 : 5, M = e4 ? 3 : 2;
          const int bias = (1 << (E - 1)) - 1, emin = 1 - bias;
          const int e = (int)((fb >> 23) & 0xff) - 127;
          const int et = e < emin ? emin : e;
          int shift = (23 - M) + (et - e);
          if (shift > 31) shift = 31;
          const uint32_t mant = (fb & 0x7fffffu) | 0x800000u;
          uint32_t q = mant >> shift;
          const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
          if (rem > half || (rem == half && (q & 1u))) q++;
          out->scalarArg = (uint64_t)((uint32_t)((et + bias - 1) << M) + q);
          break;
        }
      }
      return ncclSuccess;
    }
    default: return ncclInvalidArgument;
  }
}

NBX_EXPORT ncclResult_t nbxReduceMulti(void* const* dsts, int nDsts, const void* const* srcs, int nSrcs, size_t count,
                                       ncclDataType_t datatype, nbxDevRedOpFull op, int nPreOpSrcs, int postOp,
                                       ncclStream_t stream) {
  return reduceMultiEx(dsts, nDsts, srcs, nSrcs, count, datatype, op, nPreOpSrcs, postOp, stream, 0);
}

NBX_EXPORT int nbxKernelCount(void) {
  int n = 0;
  const KernelTable& t = table();
  for (int ty = 0; ty < kNumTypes; ty++)
    for (int o = 0; o < kNumDevOps; o++)
      if (t[ty][o].valid) n++;
  return n;
}

NBX_EXPORT int nbxAbiVersion(void) { return 1; }
