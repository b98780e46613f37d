// nbx_reduce_mx6.cc — host side of the MXFP6 forms of nbxReduceMultiWideMx
// (nbx_mx6.h; the entry point in nbx_reduce_mx.cc hands every call that names
// NBX_FLOAT6_E2M3 or NBX_FLOAT6_E3M2 to reduceMultiWideMx6): their checks, the
// layout decision, one kernel pass and the fold of > 8 sources through an fp32
// partial.
#include <cstdio>
#include <mutex>

#include "nbx_launch.h"

namespace nbx {
namespace {
// a table of its own, so nbxKernelCount and KernelSet stay as they are
Mx6Table g_mx6;
std::once_flag g_mx6Once;

const Mx6Table& mx6Table() {
  std::call_once(g_mx6Once, [] {
    std::memset(&g_mx6, 0, sizeof(g_mx6));
    fillMx6F16(g_mx6);
    fillMx6BF16(g_mx6);
    fillMx6E2M3(g_mx6);
    fillMx6E3M2(g_mx6);
  });
  return g_mx6;
}

bool isFp6(int t) { return t == kTypeFp6E2M3 || t == kTypeFp6E3M2; }
bool is16(int t) { return t == (int)ncclFloat16 || t == (int)ncclBfloat16; }
// bytes of `count` elements: an FP6 array is a dense stream of 6-bit codes
size_t arrayBytes(int t, size_t count) {
  return isFp6(t) ? (3 * count + 3) / 4 : count * (t == (int)ncclFloat32 ? sizeof(float) : sizeof(uint16_t));
}

struct Mx6Call {
  const Mx6Set* ms;
  int out;            // the call's output in the set's table (nbx_kargs.h Mx6Set)
  bool out32;         // ... is fp32
  bool blocks;        // the block kernel's layout, decided once per call
  size_t count;
  void* const* dstScales;
  const void* const* srcScales;
  nbxDevRedOpFull op;
  hipStream_t stream;
};

// One pass over <= kMaxKSrcs sources. partFirst: srcs[0] is the fp32 partial;
// the caller's sources, and their scales, then start at `first`. out32: this
// pass's output (the call's, or the fp32 partial of a later pass).
ncclResult_t launchMx6Pass(const Mx6Call& c, bool out32, bool partFirst, void* const* dsts, int nDsts,
                           const void* const* srcs, int nSrcs, int first, uint32_t mask) {
  KArgs a;
  fillKArgs(a, dsts, nDsts, srcs, nSrcs, c.count, c.op, mask);
  MxArgs x;
  std::memset(&x, 0, sizeof(x));
  const int slot0 = partFirst ? 1 : 0;
  if (c.ms->fp6)
    for (int s = slot0; s < nSrcs; s++) x.srcScale[s] = (const uint8_t*)c.srcScales[first + s - slot0];
  if (!out32)
    for (int d = 0; d < kMaxKDsts; d++) x.dstScale[d] = (uint8_t*)c.dstScales[d < nDsts ? d : 0];
  const int out = out32 ? 1 : c.out;   // an fp32 pass exists for MXFP6 sources only, whose output 1 it is
  const size_t cus = (size_t)cuCount(launchDevice(c.stream));
  const int flags =
      (out32 ? kLaunchOut32 : 0) | (partFirst ? kLaunchPartFirst : 0) | (c.ms->fp6 ? kLaunchMxScaled : 0);
  void* args[] = {&a, &x};
  hipError_t err;
  if (c.blocks) {
    // the wide pack launch's grid rule over tiles of `unroll` blocks per lane, a
    // lane's loads counted in 16-byte units (a 16-bit block is four, an FP6 block 1.5)
    const int unroll = mx6Unroll(nSrcs, c.ms->fp6 != 0);
    const int loads = c.ms->fp6 ? (nSrcs * unroll * 3 + 1) / 2 : nSrcs * unroll * 4;
    int perCU = maxBlocksPerCU(true, loads);
    if (!launchPolicyOverridden() && perCU < 2) perCU = 2;
    a.nPacks = (uint64_t)(c.count / kMxBlockElts);
    const size_t tile = (size_t)unroll * kBlock;
    const size_t grid = cappedGrid((size_t)((a.nPacks + tile - 1) / tile), cus * (size_t)perCU);
    err = hipLaunchKernel(c.ms->blocks[out][slot0][nSrcs - 1], dim3((unsigned)grid), dim3(kBlock), args, 0, c.stream);
    logLaunch(kFamMx6Blocks, nSrcs, unroll, flags);
  } else {
    const size_t perWG = (size_t)kBlock / 8;
    const size_t wgs = ((c.count + kMxBlockElts - 1) / kMxBlockElts + perWG - 1) / perWG;
    const size_t grid = cappedGrid(wgs, cus * (size_t)maxBlocksPerCU(false, nSrcs, /*classic=*/true));
    err = hipLaunchKernel(c.ms->generic[out][slot0], dim3((unsigned)grid), dim3(kBlock), args, 0, c.stream);
    logLaunch(kFamMx6Generic, nSrcs, 1, flags);
  }
  if (err != hipSuccess) {
    std::fprintf(stderr, "nbx: MXFP6 kernel launch failed: %s\n", hipGetErrorString(err));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}

bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1u)) == 0; }
}  // namespace

ncclResult_t reduceMultiWideMx6(void* const* dsts, void* const* dstScales, int nDsts, const void* const* srcs,
                                const void* const* srcScales, int nSrcs, size_t count, ncclDataType_t srcType,
                                ncclDataType_t dstType, nbxDevRedOpFull op, int nPreOpSrcs, ncclStream_t stream) {
  // ---- checks: all of them before any device call ----
  if (!argArraysOk(dsts, nDsts, srcs, nSrcs)) return ncclInvalidArgument;
  const int st = (int)srcType, dt = (int)dstType;
  const bool fp6In = isFp6(st), out32 = dt == (int)ncclFloat32;
  // provided: f16 / bf16 -> MXFP6, MXFP6 -> the same type, MXFP6 -> fp32
  if (!(fp6In ? (dt == st || out32) : (is16(st) && isFp6(dt)))) return ncclInvalidArgument;
  if (fp6In != (srcScales != nullptr) || out32 != (dstScales == nullptr)) return ncclInvalidArgument;
  // Sum / PreMulSum and the scalar: the wide sum's rule, which knows no FP6 tag
  const ncclDataType_t opType = fp6In ? ncclFloat16 : srcType;
  ncclResult_t cr = checkWideOp(opType, opType, op);
  if (cr != ncclSuccess) return cr;
  if (count == 0) return ncclSuccess;
  if (!pointersOk(fp6In ? 1 : sizeof(uint16_t), out32 ? sizeof(float) : 1, dsts, nDsts, srcs, nSrcs))
    return ncclInvalidArgument;
  for (int s = 0; fp6In && s < nSrcs; s++)
    if (srcScales[s] == nullptr) return ncclInvalidArgument;
  for (int d = 0; !out32 && d < nDsts; d++)
    if (dstScales[d] == nullptr) return ncclInvalidArgument;
  // nbxReduceMultiWideMx's overlap rule with an FP6 array's ceil(3 count / 4)
  // bytes: in place only MXFP6 into the same type on the source's own scale array.
  const size_t nScales = (count + kMxBlockElts - 1) / kMxBlockElts;
  const size_t sBytes = arrayBytes(st, count), dBytes = arrayBytes(dt, count);
  for (int d = 0; d < nDsts; d++) {
    if (!out32 && overlaps(dsts[d], dBytes, dstScales[d], nScales)) return ncclInvalidArgument;
    for (int s = 0; s < nSrcs; s++) {
      const bool same = st == dt && dsts[d] == srcs[s];
      if (!same && overlaps(dsts[d], dBytes, srcs[s], sBytes)) return ncclInvalidArgument;
      if (same && dstScales[d] != srcScales[s]) return ncclInvalidArgument;
      if (fp6In && overlaps(dsts[d], dBytes, srcScales[s], nScales)) return ncclInvalidArgument;
      if (out32) continue;
      if (overlaps(dstScales[d], nScales, srcs[s], sBytes)) return ncclInvalidArgument;
      if (fp6In && !same && overlaps(dstScales[d], nScales, srcScales[s], nScales)) return ncclInvalidArgument;
    }
  }

  // ---- layout: the block kernel needs 16-byte element pointers and 4-byte
  // destination scale pointers (the partial, scratch or dsts[0], follows) ----
  Mx6Call c;
  c.ms = &mx6Table()[st == (int)ncclFloat16 ? 0 : st == (int)ncclBfloat16 ? 1 : st == kTypeFp6E2M3 ? 2 : 3];
  c.out = fp6In ? (out32 ? 1 : 0) : (dt == kTypeFp6E2M3 ? 0 : 1);
  c.out32 = out32;
  c.count = count;
  c.dstScales = dstScales;
  c.srcScales = srcScales;
  c.op = wideScalarOp(op);
  c.stream = (hipStream_t)stream;
  c.blocks = true;
  for (int s = 0; s < nSrcs; s++) c.blocks &= aligned(srcs[s], 16);
  for (int d = 0; d < nDsts; d++) c.blocks &= aligned(dsts[d], 16) && (out32 || aligned(dstScales[d], 4));
  if (nPreOpSrcs < 0) nPreOpSrcs = 0;
  const bool pre = op.op == nbxDevPreMulSum;

  if (nSrcs <= kMaxKSrcs)
    return launchMx6Pass(c, out32, false, dsts, nDsts, srcs, nSrcs, 0, preMask(pre, nPreOpSrcs, 0, nSrcs, 0));

  // > 8 sources, as the other MX forms: the fp32 left fold of the sources
  // before the last pass sits in a partial that is never narrowed — dsts[0] for
  // an fp32 output, else stream-ordered scratch — and the last pass is the PART
  // kernel.
  void* scratch = nullptr;
  void* part = dsts[0];
  if (!out32) {
    if (hipMallocAsync(&scratch, count * sizeof(float), c.stream) != hipSuccess) return ncclUnhandledCudaError;
    part = scratch;
  }
  if (fp6In)
    return foldPasses(dsts, nDsts, srcs, nSrcs, part, scratch, c.stream,
                      [&](void* const* d, int nd, const void* const* s, int n, int first, bool partFirst, bool last) {
                        const int slot0 = partFirst ? 1 : 0;
                        return launchMx6Pass(c, last ? out32 : true, partFirst, d, nd, s, n, first,
                                             preMask(pre, nPreOpSrcs, first, n - slot0, slot0));
                      });
  // plain sources: all but the last 7 are nbxReduceMultiWide's fp32-output fold
  const int first = nSrcs - (kMaxKSrcs - 1);
  void* partDst[1] = {part};
  cr = reduceMultiWideEx(partDst, 1, srcs, first, count, srcType, ncclFloat32, op, nPreOpSrcs, stream, 0);
  if (cr == ncclSuccess) {
    const void* ps[kMaxKSrcs];
    ps[0] = part;
    for (int k = 1; k < kMaxKSrcs; k++) ps[k] = srcs[first + k - 1];
    cr = launchMx6Pass(c, false, true, dsts, nDsts, ps, kMaxKSrcs, first,
                       preMask(pre, nPreOpSrcs, first, kMaxKSrcs - 1, 1));
  }
  if (hipFreeAsync(scratch, c.stream) != hipSuccess && cr == ncclSuccess) cr = ncclUnhandledCudaError;
  return cr;
}

}  // namespace nbx

using namespace nbx;

// Elements of the MXFP6 block kernel's tile for `nSrcs` sources of srcType
// (test hook, include/nbx_debug.h); 0 for a type or count the call does not take.
NBX_EXPORT int nbxDebugMx6TileElts(ncclDataType_t srcType, int nSrcs) {
  const int st = (int)srcType;
  if ((!is16(st) && !isFp6(st)) || nSrcs < 1 || nSrcs > kMaxKSrcs) return 0;
  return mx6Unroll(nSrcs, isFp6(st)) * kBlock * kMxBlockElts;
}
