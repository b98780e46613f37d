// nbx_reduce_mx.cc — host side of the block-scaled sums (nbxReduceMultiWideMx:
// MXFP8 nbx_mx.h, MXFP4 nbx_mx4.h, MXFP6 nbx_mx6.h): the format table, the
// checks, the layout decision, one kernel pass and the fold of > 8 sources
// through an fp32 partial. The formats differ in the table's rows and in
// nothing else here.
#include <cstdio>
#include <mutex>

#include "nbx_launch.h"

namespace nbx {
namespace {
MxTable g_mx;
std::once_flag g_mxOnce;

// ---- the format table ----
// What an element format's kernels share: the lanes a 32-element block takes
// in the block kernel (2: 16-element groups, 4: 8-element groups, 1: the
// block) and in the any-alignment kernel, the launch families, and the word
// the launch-failure message says.
enum MxFamilyId { kMx8, kMx4, kMx6 };
struct MxFamily {
  int famBlocks, famGeneric;
  const char* word;
  int groupsPerBlock;
  int eltLanesPerBlock;
};
constexpr MxFamily kMxFamilies[] = {{kFamMxBlocks, kFamMxGeneric, "MX", 2, 32},
                                    {kFamMx4Blocks, kFamMx4Generic, "MXFP4", 4, 16},
                                    {kFamMx6Blocks, kFamMx6Generic, "MXFP6", 1, 8}};

// One row per source kind, in MxTable's order (nbx_registry.h). A call is
// taken exactly when a row has its source type, its source scales (there or
// not) and its output type; destination scales go with every output but fp32.
constexpr int kF16 = ncclFloat16, kBF16 = ncclBfloat16, kE4M3 = ncclFloat8e4m3, kE5M2 = ncclFloat8e5m2,
              kF32 = ncclFloat32, kNoOut = -1;
struct MxForm {
  int fam;
  int st;             // source type tag
  bool scaled;        // ... with block scales
  int opType;         // the type checkWideOp is asked about: it knows no FP4 / FP6 tag
  int outs[kMxOuts];  // output type by MxSet::blocks index
  int partOut;        // index of the fp32 partial that passes before the last write; kNoOut: plain
                      // kinds, whose early passes are reduceMultiWideEx
};
constexpr MxForm kMxForms[kMxKinds] = {
    {kMx8, kF16, false, kF16, {kE4M3, kE5M2, kNoOut}, kNoOut},
    {kMx8, kBF16, false, kBF16, {kE4M3, kE5M2, kNoOut}, kNoOut},
    {kMx8, kE4M3, false, kE4M3, {kE4M3, kE5M2, kNoOut}, kNoOut},
    {kMx8, kE5M2, false, kE5M2, {kE4M3, kE5M2, kNoOut}, kNoOut},
    {kMx8, kE4M3, true, kE4M3, {kE4M3, kE5M2, kF32}, 2},
    {kMx8, kE5M2, true, kE5M2, {kE4M3, kE5M2, kF32}, 2},
    {kMx4, kF16, false, kF16, {kTypeFp4, kNoOut, kNoOut}, kNoOut},
    {kMx4, kBF16, false, kBF16, {kTypeFp4, kNoOut, kNoOut}, kNoOut},
    {kMx4, kTypeFp4, true, kF16, {kTypeFp4, kF32, kNoOut}, 1},
    {kMx6, kF16, false, kF16, {kTypeFp6E2M3, kTypeFp6E3M2, kNoOut}, kNoOut},
    {kMx6, kBF16, false, kBF16, {kTypeFp6E2M3, kTypeFp6E3M2, kNoOut}, kNoOut},
    {kMx6, kTypeFp6E2M3, true, kF16, {kTypeFp6E2M3, kF32, kNoOut}, 1},
    {kMx6, kTypeFp6E3M2, true, kF16, {kTypeFp6E3M2, kF32, kNoOut}, 1},
};

// Bits of an element of a type tag (0: a tag no form names). An array of
// `count` elements is a dense bit stream: 4 count bytes of fp32, ceil(count / 2)
// of FP4, ceil(3 count / 4) of FP6. pointersOk asks the element's bytes of a
// 16-bit source and an fp32 destination, 1 of everything narrower.
int eltBits(int t) {
  switch (t) {
    case kF32: return 32;
    case kF16: case kBF16: return 16;
    case kE4M3: case kE5M2: return 8;
    case kTypeFp6E2M3: case kTypeFp6E3M2: return 6;
    case kTypeFp4: return 4;
  }
  return 0;
}
size_t arrayBytes(int t, size_t count) {
  const size_t bits = (size_t)eltBits(t);
  return count / 8 * bits + (count % 8 * bits + 7) / 8;
}
size_t eltAlign(int t) { return eltBits(t) >= 16 ? (size_t)eltBits(t) / 8 : 1; }

// Groups (MXFP6: blocks) per lane of the block kernel's tile.
int formUnroll(const MxForm& f, int nSrcs) {
  switch (f.fam) {
    case kMx8: return mxUnroll(nSrcs, eltBits(f.st) / 8);
    case kMx4: return mx4Unroll(nSrcs, f.scaled);
    default: return mx6Unroll(nSrcs, f.scaled);
  }
}

// Workgroups per CU of the block kernel: the wide pack launch's rule. MXFP8
// follows wideUnroll as that launch does; the others always run its big-tile
// policy, a lane's loads counted in 16-byte units (an FP4 group is a quarter
// of one, an FP6 block 1.5, a 16-bit block four).
int formBlocksPerCU(const MxForm& f, int nSrcs, int unroll) {
  bool big = true;
  int loads;
  switch (f.fam) {
    case kMx8:
      big = wideUnroll(nSrcs) > 1;
      loads = nSrcs * wideUnroll(nSrcs);
      break;
    case kMx4: loads = f.scaled ? (nSrcs * unroll + 3) / 4 : nSrcs * unroll; break;
    default: loads = f.scaled ? (nSrcs * unroll * 3 + 1) / 2 : nSrcs * unroll * 4; break;
  }
  int perCU = maxBlocksPerCU(big, loads);
  if (big && !launchPolicyOverridden() && perCU < 2) perCU = 2;
  return perCU;
}

struct MxCall {
  const MxForm* f;
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
// pass's output (the call's, or the form's partOut for the partial of a later pass).
ncclResult_t launchMxPass(const MxCall& c, int out, bool partFirst, void* const* dsts, int nDsts,
                          const void* const* srcs, int nSrcs, int first, uint32_t mask) {
  const MxForm& f = *c.f;
  const MxFamily& fam = kMxFamilies[f.fam];
  const bool out32 = out == f.partOut;
  KArgs a;
  fillKArgs(a, dsts, nDsts, srcs, nSrcs, c.count, c.op, mask);
  MxArgs x;
  std::memset(&x, 0, sizeof(x));
  const int slot0 = partFirst ? 1 : 0;
  if (f.scaled)
    for (int s = slot0; s < nSrcs; s++) x.srcScale[s] = (const uint8_t*)c.srcScales[first + s - slot0];
  if (!out32)
    for (int d = 0; d < kMaxKDsts; d++) x.dstScale[d] = (uint8_t*)c.dstScales[d < nDsts ? d : 0];
  const size_t cus = (size_t)cuCount(launchDevice(c.stream));
  const int flags = (out32 ? kLaunchOut32 : 0) | (partFirst ? kLaunchPartFirst : 0) | (f.scaled ? kLaunchMxScaled : 0);
  void* args[] = {&a, &x};
  hipError_t err;
  if (c.blocks) {
    // the wide pack launch's grid rule over tiles of `unroll` groups per lane
    const int unroll = formUnroll(f, nSrcs);
    const int perCU = formBlocksPerCU(f, nSrcs, unroll);
    a.nPacks = (uint64_t)(c.count / kMxBlockElts) * fam.groupsPerBlock;
    const size_t tile = (size_t)unroll * kBlock;
    const size_t grid = cappedGrid((size_t)((a.nPacks + tile - 1) / tile), cus * (size_t)perCU);
    err = hipLaunchKernel(c.ms->blocks[out][slot0][nSrcs - 1], dim3((unsigned)grid), dim3(kBlock), args, 0, c.stream);
    logLaunch(fam.famBlocks, nSrcs, unroll, flags);
  } else {
    const size_t perWG = (size_t)kBlock / fam.eltLanesPerBlock;
    const size_t wgs = ((c.count + kMxBlockElts - 1) / kMxBlockElts + perWG - 1) / perWG;
    const size_t grid = cappedGrid(wgs, cus * (size_t)maxBlocksPerCU(false, nSrcs, /*classic=*/true));
    err = hipLaunchKernel(c.ms->generic[out][slot0], dim3((unsigned)grid), dim3(kBlock), args, 0, c.stream);
    logLaunch(fam.famGeneric, nSrcs, 1, flags);
  }
  if (err != hipSuccess) {
    std::fprintf(stderr, "nbx: %s kernel launch failed: %s\n", fam.word, hipGetErrorString(err));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}

bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1u)) == 0; }

// Elements of a family's block-kernel tile for `nSrcs` sources of type st; 0
// for a type or count the family does not take (the nbxDebugMx*TileElts hooks).
int tileElts(int fam, int st, int nSrcs) {
  if (nSrcs < 1 || nSrcs > kMaxKSrcs) return 0;
  for (const MxForm& f : kMxForms)
    if (f.fam == fam && f.st == st)
      return formUnroll(f, nSrcs) * kBlock * (kMxBlockElts / kMxFamilies[fam].groupsPerBlock);
  return 0;
}
}  // namespace

// The row of the format table that takes the call, and Sum / PreMulSum with
// its scalar by the wide sum's rule.
ncclResult_t checkMxTypes(ncclDataType_t srcType, ncclDataType_t dstType, const nbxDevRedOpFull& op, bool scaled,
                          bool dstScaled, int* kind, int* out) {
  const int st = (int)srcType, dt = (int)dstType;
  if (eltBits(dt) == 0 || dstScaled == (dt == kF32)) return ncclInvalidArgument;
  for (int k = 0; k < kMxKinds; k++) {
    const MxForm& f = kMxForms[k];
    if (f.st != st || f.scaled != scaled) continue;
    for (int o = 0; o < kMxOuts; o++)
      if (f.outs[o] == dt) {
        *kind = k;
        *out = o;
        return checkWideOp((ncclDataType_t)f.opType, (ncclDataType_t)f.opType, op);
      }
  }
  return ncclInvalidArgument;
}

ncclResult_t checkMxBucket(int st, int dt, void* const* dsts, void* const* dstScales, int nDsts,
                           const void* const* srcs, const void* const* srcScales, int nSrcs, size_t count) {
  const bool scaled = srcScales != nullptr, out32 = dt == kF32;
  if (!pointersOk(eltAlign(st), eltAlign(dt), dsts, nDsts, srcs, nSrcs)) return ncclInvalidArgument;
  for (int s = 0; scaled && s < nSrcs; s++)
    if (srcScales[s] == nullptr) return ncclInvalidArgument;
  for (int d = 0; !out32 && d < nDsts; d++)
    if (dstScales[d] == nullptr) return ncclInvalidArgument;
  // A destination may be one of the sources when the types agree (a lane
  // reads the bytes it writes before it writes them), and its scales then are
  // that source's; everything else a destination owns is apart from
  // everything a source owns, and its two arrays from each other.
  const size_t nScales = (count + kMxBlockElts - 1) / kMxBlockElts;
  const size_t sBytes = arrayBytes(st, count), dBytes = arrayBytes(dt, count);
  for (int d = 0; d < nDsts; d++) {
    if (!out32 && overlaps(dsts[d], dBytes, dstScales[d], nScales)) return ncclInvalidArgument;
    for (int s = 0; s < nSrcs; s++) {
      const bool same = st == dt && dsts[d] == srcs[s];
      if (!same && overlaps(dsts[d], dBytes, srcs[s], sBytes)) return ncclInvalidArgument;
      if (same && scaled && dstScales[d] != srcScales[s]) return ncclInvalidArgument;
      if (scaled && overlaps(dsts[d], dBytes, srcScales[s], nScales)) return ncclInvalidArgument;
      if (out32) continue;
      if (overlaps(dstScales[d], nScales, srcs[s], sBytes)) return ncclInvalidArgument;
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
    fillMx4F16(g_mx);
    fillMx4BF16(g_mx);
    fillMx4Fp4(g_mx);
    fillMx6F16(g_mx);
    fillMx6BF16(g_mx);
    fillMx6E2M3(g_mx);
    fillMx6E3M2(g_mx);
  });
  return g_mx;
}

}  // namespace nbx

using namespace nbx;

NBX_EXPORT ncclResult_t nbxReduceMultiWideMx(void* const* dsts, void* const* dstScales, int nDsts,
                                             const void* const* srcs, const void* const* srcScales, int nSrcs,
                                             size_t count, ncclDataType_t srcType, ncclDataType_t dstType,
                                             nbxDevRedOpFull op, int nPreOpSrcs, ncclStream_t stream) {
  // ---- checks: all of them before any device call ----
  if (!argArraysOk(dsts, nDsts, srcs, nSrcs)) return ncclInvalidArgument;
  const bool scaled = srcScales != nullptr;
  int kind, out;
  ncclResult_t cr = checkMxTypes(srcType, dstType, op, scaled, dstScales != nullptr, &kind, &out);
  if (cr != ncclSuccess) return cr;
  if (count == 0) return ncclSuccess;
  cr = checkMxBucket((int)srcType, (int)dstType, dsts, dstScales, nDsts, srcs, srcScales, nSrcs, count);
  if (cr != ncclSuccess) return cr;

  // ---- layout: the block kernel needs 16-byte element pointers and 4-byte
  // destination scale pointers (the partial, scratch or dsts[0], follows) ----
  MxCall c;
  c.f = &kMxForms[kind];
  c.ms = &mxTable()[kind];
  c.out = out;
  c.count = count;
  c.dstScales = dstScales;
  c.srcScales = srcScales;
  c.op = wideScalarOp(op);
  c.stream = (hipStream_t)stream;
  const bool out32 = out == c.f->partOut;
  c.blocks = mxBlockLayout(dsts, out32 ? nullptr : dstScales, nDsts, srcs, nSrcs);
  if (nPreOpSrcs < 0) nPreOpSrcs = 0;
  const bool pre = op.op == nbxDevPreMulSum;

  if (nSrcs <= kMaxKSrcs)
    return launchMxPass(c, out, false, dsts, nDsts, srcs, nSrcs, 0, preMask(pre, nPreOpSrcs, 0, nSrcs, 0));

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
                        return launchMxPass(c, last ? out : c.f->partOut, partFirst, d, nd, s, n, first,
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
    cr = launchMxPass(c, out, true, dsts, nDsts, ps, kMaxKSrcs, first,
                      preMask(pre, nPreOpSrcs, first, kMaxKSrcs - 1, 1));
  }
  if (hipFreeAsync(scratch, c.stream) != hipSuccess && cr == ncclSuccess) cr = ncclUnhandledCudaError;
  return cr;
}

// Elements of the block kernel's tile for `nSrcs` sources of srcType, family
// by family (test hooks, include/nbx_debug.h).
NBX_EXPORT int nbxDebugMxTileElts(ncclDataType_t srcType, int nSrcs) { return tileElts(kMx8, (int)srcType, nSrcs); }
NBX_EXPORT int nbxDebugMx4TileElts(ncclDataType_t srcType, int nSrcs) { return tileElts(kMx4, (int)srcType, nSrcs); }
NBX_EXPORT int nbxDebugMx6TileElts(ncclDataType_t srcType, int nSrcs) { return tileElts(kMx6, (int)srcType, nSrcs); }
