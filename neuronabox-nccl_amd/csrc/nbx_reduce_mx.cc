// nbx_reduce_mx.cc — host side of the MXFP8 block-scaled sums (nbx_mx.h,
// nbxReduceMultiWideMx): their checks, the layout decision, one kernel pass
// and the fold of > 8 sources through an fp32 partial.
#include <cstdio>
#include <mutex>

#include "nbx_launch.h"

namespace nbx {
namespace {
// a table of its own, so nbxKernelCount and KernelSet stay as they are
MxTable g_mx;
std::once_flag g_mxOnce;

bool isFp8(int t) { return t == (int)ncclFloat8e4m3 || t == (int)ncclFloat8e5m2; }

// Output index (MxSet::blocks) of a checked type.
int mxOut(int dt) { return dt == (int)ncclFloat8e4m3 ? 0 : dt == (int)ncclFloat8e5m2 ? 1 : 2; }

struct MxCall {
  const MxSet* ms;
  int out;            // MxSet::blocks index of the call's output
  bool blocks;        // the block kernel's layout, decided once per call
  size_t count;
  void* const* dstScales;
  const void* const* srcScales;
  nbxDevRedOpFull op;
  hipStream_t stream;
};

// One pass over <= kMaxKSrcs sources. partFirst: srcs[0] is the fp32 partial;
// the caller's sources, and their scales, then start at `first`. out: this
// pass's output (2 = the fp32 partial of a later pass).
ncclResult_t launchMxPass(const MxCall& c, int out, bool partFirst, void* const* dsts, int nDsts,
                          const void* const* srcs, int nSrcs, int first, uint32_t mask) {
  KArgs a;
  fillKArgs(a, dsts, nDsts, srcs, nSrcs, c.count, c.op, mask);
  MxArgs x;
  std::memset(&x, 0, sizeof(x));
  const int slot0 = partFirst ? 1 : 0;
  if (c.ms->scaled)
    for (int s = slot0; s < nSrcs; s++) x.srcScale[s] = (const uint8_t*)c.srcScales[first + s - slot0];
  if (out != 2)
    for (int d = 0; d < kMaxKDsts; d++) x.dstScale[d] = (uint8_t*)c.dstScales[d < nDsts ? d : 0];
  const size_t cus = (size_t)cuCount(launchDevice(c.stream));
  const int flags =
      (out == 2 ? kLaunchOut32 : 0) | (partFirst ? kLaunchPartFirst : 0) | (c.ms->scaled ? kLaunchMxScaled : 0);
  void* args[] = {&a, &x};
  hipError_t err;
  if (c.blocks) {
    // the wide pack launch's grid rule over tiles of `unroll` groups per lane
    const int unroll = mxUnroll(nSrcs, c.ms->eltBytes);
    const bool big = wideUnroll(nSrcs) > 1;
    int perCU = maxBlocksPerCU(big, nSrcs * wideUnroll(nSrcs));
    if (big && !launchPolicyOverridden() && perCU < 2) perCU = 2;
    a.nPacks = (uint64_t)(c.count / kMxBlockElts) * (kMxBlockElts / kMxGroupElts);
    const size_t tile = (size_t)unroll * kBlock;
    const size_t grid = cappedGrid((size_t)((a.nPacks + tile - 1) / tile), cus * (size_t)perCU);
    err = hipLaunchKernel(c.ms->blocks[out][slot0][nSrcs - 1], dim3((unsigned)grid), dim3(kBlock), args, 0, c.stream);
    logLaunch(kFamMxBlocks, nSrcs, unroll, flags);
  } else {
    const size_t perWG = (size_t)kBlock / kMxBlockElts;
    const size_t wgs = ((c.count + kMxBlockElts - 1) / kMxBlockElts + perWG - 1) / perWG;
    const size_t grid = cappedGrid(wgs, cus * (size_t)maxBlocksPerCU(false, nSrcs, /*classic=*/true));
    err = hipLaunchKernel(c.ms->generic[out][slot0], dim3((unsigned)grid), dim3(kBlock), args, 0, c.stream);
    logLaunch(kFamMxGeneric, nSrcs, 1, flags);
  }
  if (err != hipSuccess) {
    std::fprintf(stderr, "nbx: MX kernel launch failed: %s\n", hipGetErrorString(err));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}

bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1u)) == 0; }
}  // namespace

// Source kind (MxTable index) of checked types.
int mxKind(int st, bool scaled) {
  const int plain = st == (int)ncclFloat16 ? 0 : st == (int)ncclBfloat16 ? 1 : st == (int)ncclFloat8e4m3 ? 2 : 3;
  return scaled ? plain + 2 : plain;
}

// The four source types, Sum / PreMulSum, the scalar; scales only beside fp8
// sources; an fp8 output with scale arrays, or fp32 without and from scaled
// sources only.
ncclResult_t checkMxTypes(ncclDataType_t srcType, ncclDataType_t dstType, const nbxDevRedOpFull& op, bool scaled,
                          bool dstScaled) {
  ncclResult_t cr = checkWideOp(srcType, srcType, op);
  if (cr != ncclSuccess) return cr;
  const int st = (int)srcType, dt = (int)dstType;
  if (scaled && !isFp8(st)) return ncclInvalidArgument;
  if (dt == (int)ncclFloat32 ? (dstScaled || !scaled) : (!isFp8(dt) || !dstScaled)) return ncclInvalidArgument;
  return ncclSuccess;
}

ncclResult_t checkMxBucket(int st, int dt, void* const* dsts, void* const* dstScales, int nDsts,
                           const void* const* srcs, const void* const* srcScales, int nSrcs, size_t count) {
  const bool scaled = srcScales != nullptr, out32 = dt == (int)ncclFloat32;
  const size_t eb = (size_t)typeSize(st), deb = out32 ? sizeof(float) : 1;
  if (!pointersOk(eb, deb, dsts, nDsts, srcs, nSrcs)) return ncclInvalidArgument;
  for (int s = 0; scaled && s < nSrcs; s++)
    if (srcScales[s] == nullptr) return ncclInvalidArgument;
  for (int d = 0; !out32 && d < nDsts; d++)
    if (dstScales[d] == nullptr) return ncclInvalidArgument;
  // A destination may be one of the sources when the types agree (a lane
  // reads the bytes it writes before it writes them), and its scales then are
  // that source's; everything else a destination owns is apart from
  // everything a source owns, and its two arrays from each other.
  const size_t nScales = (count + kMxBlockElts - 1) / kMxBlockElts;
  for (int d = 0; d < nDsts; d++) {
    if (!out32 && overlaps(dsts[d], count * deb, dstScales[d], nScales)) return ncclInvalidArgument;
    for (int s = 0; s < nSrcs; s++) {
      const bool same = st == dt && dsts[d] == srcs[s];
      if (!same && overlaps(dsts[d], count * deb, srcs[s], count * eb)) return ncclInvalidArgument;
      if (same && scaled && dstScales[d] != srcScales[s]) return ncclInvalidArgument;
      if (scaled && overlaps(dsts[d], count * deb, srcScales[s], nScales)) return ncclInvalidArgument;
      if (out32) continue;
      if (overlaps(dstScales[d], nScales, srcs[s], count * eb)) return ncclInvalidArgument;
      if (scaled && !same && overlaps(dstScales[d], nScales, srcScales[s], nScales)) return ncclInvalidArgument;
    }
  }
  return ncclSuccess;
}

bool mxBlockLayout(void* const* dsts, void* const* dstScales, int nDsts, const void* const* srcs, int nSrcs) {
  bool ok = true;
  for (int s = 0; s < nSrcs; s++) ok &= aligned(srcs[s], 16);
  for (int d = 0; d < nDsts; d++) ok &= aligned(dsts[d], 16) && (dstScales == nullptr || aligned(dstScales[d], 4));
  return ok;
}

const MxTable& mxTable() {
  std::call_once(g_mxOnce, [] {
    std::memset(&g_mx, 0, sizeof(g_mx));
    fillMxF16(g_mx);
    fillMxBF16(g_mx);
    fillMxE4M3(g_mx);
    fillMxE5M2(g_mx);
    fillMxE4M3Scaled(g_mx);
    fillMxE5M2Scaled(g_mx);
  });
  return g_mx;
}

}  // namespace nbx

using namespace nbx;

NBX_EXPORT ncclResult_t nbxReduceMultiWideMx(void* const* dsts, void* const* dstScales, int nDsts,
                                             const void* const* srcs, const void* const* srcScales, int nSrcs,
                                             size_t count, ncclDataType_t srcType, ncclDataType_t dstType,
                                             nbxDevRedOpFull op, int nPreOpSrcs, ncclStream_t stream) {
  const auto fp6 = [](ncclDataType_t t) { return (int)t == kTypeFp6E2M3 || (int)t == kTypeFp6E3M2; };
  if (fp6(srcType) || fp6(dstType))   // MXFP6: nbx_reduce_mx6.cc; a pair with NBX_FLOAT4_E2M1 is refused there
    return reduceMultiWideMx6(dsts, dstScales, nDsts, srcs, srcScales, nSrcs, count, srcType, dstType, op, nPreOpSrcs,
                              stream);
  if ((int)srcType == kTypeFp4 || (int)dstType == kTypeFp4)   // MXFP4: nbx_reduce_mx4.cc
    return reduceMultiWideMx4(dsts, dstScales, nDsts, srcs, srcScales, nSrcs, count, srcType, dstType, op, nPreOpSrcs,
                              stream);
  // ---- checks: all of them before any device call ----
  if (!argArraysOk(dsts, nDsts, srcs, nSrcs)) return ncclInvalidArgument;
  const bool scaled = srcScales != nullptr;
  ncclResult_t cr = checkMxTypes(srcType, dstType, op, scaled, dstScales != nullptr);
  if (cr != ncclSuccess) return cr;
  if (count == 0) return ncclSuccess;
  const int st = (int)srcType, dt = (int)dstType;
  const bool out32 = dt == (int)ncclFloat32;
  cr = checkMxBucket(st, dt, dsts, dstScales, nDsts, srcs, srcScales, nSrcs, count);
  if (cr != ncclSuccess) return cr;

  // ---- layout: the block kernel needs 16-byte element pointers and 4-byte
  // destination scale pointers (the partial, scratch or dsts[0], follows) ----
  MxCall c;
  c.ms = &mxTable()[mxKind(st, scaled)];
  c.out = mxOut(dt);
  c.count = count;
  c.dstScales = dstScales;
  c.srcScales = srcScales;
  c.op = wideScalarOp(op);
  c.stream = (hipStream_t)stream;
  c.blocks = mxBlockLayout(dsts, out32 ? nullptr : dstScales, nDsts, srcs, nSrcs);
  if (nPreOpSrcs < 0) nPreOpSrcs = 0;
  const bool pre = op.op == nbxDevPreMulSum;

  if (nSrcs <= kMaxKSrcs)
    return launchMxPass(c, c.out, false, dsts, nDsts, srcs, nSrcs, 0, preMask(pre, nPreOpSrcs, 0, nSrcs, 0));

  // > 8 sources: earlier passes leave the fp32 left fold of the sources before
  // the last pass in a partial that is never narrowed — dsts[0] for an fp32
  // output (no source overlaps it), else stream-ordered scratch — and the last
  // pass is the PART kernel.
  void* scratch = nullptr;
  void* part = dsts[0];
  if (!out32) {
    if (hipMallocAsync(&scratch, count * sizeof(float), c.stream) != hipSuccess) return ncclUnhandledCudaError;
    part = scratch;
  }
  if (scaled)
    return foldPasses(dsts, nDsts, srcs, nSrcs, part, scratch, c.stream,
                      [&](void* const* d, int nd, const void* const* s, int n, int first, bool partFirst, bool last) {
                        const int slot0 = partFirst ? 1 : 0;
                        return launchMxPass(c, last ? c.out : 2, partFirst, d, nd, s, n, first,
                                            preMask(pre, nPreOpSrcs, first, n - slot0, slot0));
                      });
  // plain sources: all but the last 7 are nbxReduceMultiWide's fp32-output
  // fold (itself in passes beyond 8), the same ordered fp32 operations
  const int first = nSrcs - (kMaxKSrcs - 1);
  void* partDst[1] = {part};
  cr = reduceMultiWideEx(partDst, 1, srcs, first, count, srcType, ncclFloat32, op, nPreOpSrcs, stream, 0);
  if (cr == ncclSuccess) {
    const void* ps[kMaxKSrcs];
    ps[0] = part;
    for (int k = 1; k < kMaxKSrcs; k++) ps[k] = srcs[first + k - 1];
    cr = launchMxPass(c, c.out, true, dsts, nDsts, ps, kMaxKSrcs, first,
                      preMask(pre, nPreOpSrcs, first, kMaxKSrcs - 1, 1));
  }
  if (hipFreeAsync(scratch, c.stream) != hipSuccess && cr == ncclSuccess) cr = ncclUnhandledCudaError;
  return cr;
}

// Elements of the block kernel's tile for `nSrcs` sources of srcType (test
// hook, include/nbx_debug.h); 0 for a type or count the call does not take.
NBX_EXPORT int nbxDebugMxTileElts(ncclDataType_t srcType, int nSrcs) {
  const int st = (int)srcType;
  if (st != (int)ncclFloat16 && st != (int)ncclBfloat16 && !isFp8(st)) return 0;
  if (nSrcs < 1 || nSrcs > kMaxKSrcs) return 0;
  return mxUnroll(nSrcs, isFp8(st) ? 1 : 2) * kBlock * kMxGroupElts;
}
