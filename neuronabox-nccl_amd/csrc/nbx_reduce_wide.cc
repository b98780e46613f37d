// nbx_reduce_wide.cc — host side of the fp32-accumulating sums (nbx_wide.h,
// nbxReduceMultiWide): their checks, the layout decision, one kernel pass and
// the fold of > 8 sources through an fp32 partial.
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "nbx_launch.h"

namespace nbx {
namespace {
// their own table, so nbxKernelCount and KernelSet stay as they are
WideTable g_wide;
std::once_flag g_wideOnce;

// Elements from which a call outside the pack layout takes the realigning
// kernel (kWideShiftedLds) instead of the element kernel; env
// NBX_WIDE_SHIFT_MIN_ELTS, nbxDebugSetWideShiftMinElts. The default is the
// measured crossover (scripts/ab_wide_shift.py, profiles/r9/
// ab_wide_shift_mi355x.txt): the smallest swept count from which
// the realigning kernel beats the element kernel for every type, output and
// 2 / 4 / 8 sources. Below about 512 Ki elements every kernel is launch-bound
// (3.5-4.3 us) and the 8-source realigning kernel, with its 129 KiB of LDS, has
// the higher floor (5.2-6.2 us); 2 sources already win from 512 Ki.
constexpr long long kWideShiftMinEltsDefault = 2097152;
long long parseWideShiftMinElts() {
  if (const char* s = std::getenv("NBX_WIDE_SHIFT_MIN_ELTS")) {
    char* end = nullptr;
    const long long x = std::strtoll(s, &end, 10);
    if (end != s && x >= 1) return x;
  }
  return kWideShiftMinEltsDefault;
}
LazySetting<long long> g_wideShiftMinElts{0, parseWideShiftMinElts};

// One pass of the fp32-accumulating kernels (nbx_wide.h) over <= kMaxKSrcs
// sources. partFirst: srcs[0] is the fp32 partial of the earlier passes.
// layout / head are decided once per call from the caller's pointers (every
// pass of a call folds sources of the same alignment into the same partial).
// op: as wideScalarOp() returns it.
ncclResult_t launchWidePass(const WideSet& ws, bool out32, bool partFirst, int layout, size_t head, void* const* dsts,
                            int nDsts, const void* const* srcs, int nSrcs, size_t count, const nbxDevRedOpFull& op,
                            uint32_t mask, int acquireSystem, hipStream_t stream) {
  KArgs a;
  fillKArgs(a, dsts, nDsts, srcs, nSrcs, count, op, mask);
  a.acquireSystem = acquireSystem;
  const int dev = launchDevice(stream);
  const size_t cus = (size_t)cuCount(dev);
  void* args[] = {&a};
  hipError_t err;
  const int wideFlags = (out32 ? kLaunchOut32 : 0) | (partFirst ? kLaunchPartFirst : 0);
  const int o = out32 ? 1 : 0, p = partFirst ? 1 : 0;
  Body b(count, head, 16 / ws.eltBytes);
  if (layout == kWideLayoutPacks) {
    const int unroll = wideUnroll(nSrcs);
    const bool big = unroll > 1;
    int perCU = maxBlocksPerCU(big, nSrcs * unroll);
    if (big && !launchPolicyOverridden() && perCU < ws.blocksPerCU) perCU = ws.blocksPerCU;
    b.cut((size_t)unroll * kBlock, cus * (size_t)perCU);
    b.into(a);
    a.variant = big ? 1 : 0;
    // dynamic tiles under launchPass's rule: unrolled tiles, long launches
    DynLaunch dyn;
    if (big && b.tiles >= (size_t)dynMinTilesPerWG() * b.grid) dyn.begin(dev, stream, b.tiles, a);
    err = hipLaunchKernel(ws.packs[o][p][nSrcs - 1], dim3((unsigned)b.grid), dim3(kBlock), args, 0, stream);
    logLaunch(kFamWidePacks, nSrcs, unroll, wideFlags | (a.dynCtr != nullptr ? kLaunchDynamic : 0));
    dyn.done(err == hipSuccess);
  } else if (layout == kWideLayoutShifted) {
    // 16-byte packs on the destinations' side, the typed sources realigned
    // through LDS (kWideShiftedLds): the per-step realigning kernel's tile,
    // workgroups per CU and static schedule
    const int unroll = shiftLdsUnroll(nSrcs);
    b.cut((size_t)unroll * 64 * kShiftLdsWaves, cus * (size_t)shiftedBlocksPerCU(true, nSrcs));
    b.into(a);
    err = hipLaunchKernel(ws.shiftedLds[o][p][nSrcs - 1], dim3((unsigned)b.grid),
                          dim3((unsigned)(kShiftLdsWaves * 64)), args, 0, stream);
    logLaunch(kFamWideShiftedLds, nSrcs, unroll, wideFlags);
  } else {
    const size_t blocks = (count + kBlock - 1) / kBlock;
    const size_t grid = cappedGrid(blocks, cus * (size_t)maxBlocksPerCU(false, nSrcs, /*classic=*/true));
    err = hipLaunchKernel(ws.elts[o][p], dim3((unsigned)grid), dim3(kBlock), args, 0, stream);
    logLaunch(kFamWideElts, nSrcs, 1, wideFlags);
  }
  if (err != hipSuccess) {
    std::fprintf(stderr, "nbx: wide kernel launch failed: %s\n", hipGetErrorString(err));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}

// Pack-kernel layout: the sources share one misalignment modulo 16, and behind
// the head elements that align them every destination is 16-byte aligned.
// *head: those elements, at most count.
bool widePackLayout(size_t eb, size_t deb, void* const* dsts, int nDsts, const void* const* srcs, int nSrcs,
                    size_t count, size_t* head) {
  const int mis = sharedMis16(srcs, nSrcs);
  const size_t h = mis > 0 ? (size_t)(16 - mis) / eb : 0;
  bool fast = mis >= 0;
  for (int d = 0; d < nDsts; d++) fast &= ((((uintptr_t)dsts[d] + h * deb) & 15u) == 0);
  *head = h > count ? count : h;
  return fast;
}
}  // namespace

const WideTable& wideTable() {
  std::call_once(g_wideOnce, [] {
    std::memset(&g_wide, 0, sizeof(g_wide));
    fillWide(g_wide);
  });
  return g_wide;
}

nbxDevRedOpFull wideScalarOp(nbxDevRedOpFull op) {
  if (op.op != nbxDevPreMulSum) op.scalarArg = 0, op.scalarArgIsPtr = 0;
  else if (!op.scalarArgIsPtr) op.scalarArg &= 0xffffffffull;
  return op;
}

// Type, op and scalar checks of the fp32-accumulating sums, shared by the
// single and batched entry points.
ncclResult_t checkWideOp(ncclDataType_t srcType, ncclDataType_t dstType, const nbxDevRedOpFull& op) {
  const int st = (int)srcType, dt = (int)dstType;
  if (st < 0 || st >= kNumTypes || !wideTable()[st].valid) return ncclInvalidArgument;   // f16, bf16, fp8 only
  if (dt != st && dt != (int)ncclFloat32) return ncclInvalidArgument;
  if (op.op != nbxDevSum && op.op != nbxDevPreMulSum) return ncclInvalidArgument;
  if (op.op == nbxDevPreMulSum && op.scalarArgIsPtr && (op.scalarArg == 0 || (op.scalarArg & 3u) != 0))
    return ncclInvalidArgument;
  return ncclSuccess;
}

// The layout of a call, decided once from its pointers. Packs: above.
// Realigning: any other layout whose destinations share one address modulo 16,
// from NBX_WIDE_SHIFT_MIN_ELTS elements; *head is then the elements that bring
// the destinations to a 16-byte boundary (< 16 / deb), at most count.
// Everything else — destinations on different alignments, short calls — runs
// the element kernel (*head = 0). The launch variant has no say.
int wideLayout(size_t eb, size_t deb, void* const* dsts, int nDsts, const void* const* srcs, int nSrcs, size_t count,
               size_t* head) {
  if (widePackLayout(eb, deb, dsts, nDsts, srcs, nSrcs, count, head)) return kWideLayoutPacks;
  *head = 0;
  const int dmis = sharedMis16(dsts, nDsts);
  if (dmis < 0 || count < (unsigned long long)g_wideShiftMinElts.get()) return kWideLayoutElts;
  const size_t h = (size_t)((16 - dmis) & 15) / deb;
  *head = h > count ? count : h;
  return kWideLayoutShifted;
}

// nbxReduceMultiWide with the internal flags of reduceMultiEx: with
// kReduceAcquireSystem every pass's workgroups issue a system-scope acquire
// before their first load (the clique's fold reads its peers' buffers).
ncclResult_t reduceMultiWideEx(void* const* dsts, int nDsts, const void* const* srcs, int nSrcs, size_t count,
                               ncclDataType_t srcType, ncclDataType_t dstType, nbxDevRedOpFull op, int nPreOpSrcs,
                               ncclStream_t stream, int flags) {
  const int acq = (flags & kReduceAcquireSystem) ? 1 : 0;
  if (!argArraysOk(dsts, nDsts, srcs, nSrcs)) return ncclInvalidArgument;
  ncclResult_t cr = checkWideOp(srcType, dstType, op);
  if (cr != ncclSuccess) return cr;
  if (count == 0) return ncclSuccess;
  const int st = (int)srcType;
  const bool pre = op.op == nbxDevPreMulSum;
  const WideSet& ws = wideTable()[st];
  const bool out32 = (int)dstType != st;
  const size_t eb = (size_t)ws.eltBytes, deb = out32 ? sizeof(float) : eb;
  cr = checkBucket(eb, deb, out32, dsts, nDsts, srcs, nSrcs, count);
  if (cr != ncclSuccess) return cr;
  if (nPreOpSrcs < 0) nPreOpSrcs = 0;
  hipStream_t strm = (hipStream_t)stream;
  const nbxDevRedOpFull lop = wideScalarOp(op);

  size_t head = 0;
  const int layout = wideLayout(eb, deb, dsts, nDsts, srcs, nSrcs, count, &head);

  if (nSrcs <= kMaxKSrcs)
    return launchWidePass(ws, out32, false, layout, head, dsts, nDsts, srcs, nSrcs, count, lop,
                          preMask(pre, nPreOpSrcs, 0, nSrcs, 0), acq, strm);

  // > 8 sources (foldPasses) through an fp32 partial that is never narrowed,
  // so the result is the single fp32 left fold. The partial lives in dsts[0]
  // when the output is fp32 (no source overlaps it), else in stream-ordered
  // scratch (graph-capturable), placed so that its body behind the head
  // elements is 16-byte aligned like the sources' (pack layout) or the
  // destinations' (realigning layout, which reads it by packs).
  void* scratch = nullptr;
  void* part = dsts[0];
  if (!out32) {
    if (hipMallocAsync(&scratch, count * sizeof(float) + 16, strm) != hipSuccess) return ncclUnhandledCudaError;
    part = (char*)scratch + ((16u - (unsigned)((head * sizeof(float)) & 15u)) & 15u);
  }
  // the partial is fp32 whatever the output: its passes use the fp32-output kernels
  return foldPasses(dsts, nDsts, srcs, nSrcs, part, scratch, strm,
                    [&](void* const* d, int nd, const void* const* s, int n, int first, bool partFirst, bool last) {
                      const int slot0 = partFirst ? 1 : 0;
                      return launchWidePass(ws, last ? out32 : true, partFirst, layout, head, d, nd, s, n, count, lop,
                                            preMask(pre, nPreOpSrcs, first, n - slot0, slot0), acq, strm);
                    });
}

}  // namespace nbx

using namespace nbx;

NBX_EXPORT ncclResult_t nbxReduceMultiWide(void* const* dsts, int nDsts, const void* const* srcs, int nSrcs,
                                           size_t count, ncclDataType_t srcType, ncclDataType_t dstType,
                                           nbxDevRedOpFull op, int nPreOpSrcs, ncclStream_t stream) {
  return reduceMultiWideEx(dsts, nDsts, srcs, nSrcs, count, srcType, dstType, op, nPreOpSrcs, stream, 0);
}

NBX_EXPORT long long nbxDebugSetWideShiftMinElts(long long elts) { return g_wideShiftMinElts.set(elts, elts >= 1); }

NBX_EXPORT int nbxDebugWideLayout(void* const* dsts, int nDsts, const void* const* srcs, int nSrcs, size_t count,
                                  ncclDataType_t srcType, ncclDataType_t dstType, size_t* head) {
  const int st = (int)srcType, dt = (int)dstType;
  if (st != ncclFloat16 && st != ncclBfloat16 && st != ncclFloat8e4m3 && st != ncclFloat8e5m2) return -1;
  if (dt != st && dt != (int)ncclFloat32) return -1;
  if (!argArraysOk(dsts, nDsts, srcs, nSrcs)) return -1;
  const size_t eb = (size_t)typeSize(st), deb = dt != st ? sizeof(float) : eb;
  if (!pointersOk(eb, deb, dsts, nDsts, srcs, nSrcs)) return -1;
  size_t h = 0;
  const int layout = wideLayout(eb, deb, dsts, nDsts, srcs, nSrcs, count, &h);
  if (head != nullptr) *head = h;
  return layout;
}
