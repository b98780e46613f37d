// nbx_reduce_mx2d.cc — host side of nbxReduceMultiWideMx2d (nbx_mx2d.h): the
// checks, the layout decision, the one 2-D kernel pass, and the fold of > 8
// sources, whose earlier passes are the flat fp32 passes of nbxReduceMultiWide
// (plain sources) or nbxReduceMultiWideMx (scaled sources).
#include <cstdio>
#include <mutex>

#include "nbx_launch.h"

namespace nbx {
namespace {
Mx2dTable g_mx2d;
std::once_flag g_mx2dOnce;

const Mx2dTable& mx2dTable() {
  std::call_once(g_mx2dOnce, [] {
    std::memset(&g_mx2d, 0, sizeof(g_mx2d));
    fillMx2dF16(g_mx2d);
    fillMx2dBF16(g_mx2d);
    fillMx2dE4M3(g_mx2d);
    fillMx2dE5M2(g_mx2d);
    fillMx2dE4M3Scaled(g_mx2d);
    fillMx2dE5M2Scaled(g_mx2d);
  });
  return g_mx2d;
}

struct Span {
  const void* p;
  size_t bytes;
};

bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1u)) == 0; }

struct Mx2dCall {
  const Mx2dSet* ms;
  int out;
  bool scaled, rowOut;
  size_t rows, cols;
  void* const* rowDsts;
  void* const* rowScales;
  void* const* colScales;
  const void* const* srcScales;
  nbxDevRedOpFull op;
  hipStream_t stream;
};

// The one 2-D pass over <= kMaxKSrcs sources. partFirst: srcs[0] is the fp32
// partial and the caller's sources, and their scales, start at `first`.
ncclResult_t launchMx2dPass(const Mx2dCall& c, bool partFirst, void* const* colDsts, int nDsts, const void* const* srcs,
                            int nSrcs, int first, uint32_t mask) {
  KArgs a;
  fillKArgs(a, colDsts, nDsts, srcs, nSrcs, c.rows * c.cols, c.op, mask);
  Mx2dArgs x;
  std::memset(&x, 0, sizeof(x));
  const int slot0 = partFirst ? 1 : 0;
  if (c.scaled)
    for (int s = slot0; s < nSrcs; s++) x.srcScale[s] = (const uint8_t*)c.srcScales[first + s - slot0];
  for (int d = 0; d < kMaxKDsts; d++) {
    const int k = d < nDsts ? d : 0;
    x.colScale[d] = (uint8_t*)c.colScales[k];
    if (c.rowOut) {
      x.rowDst[d] = c.rowDsts[k];
      x.rowScale[d] = (uint8_t*)c.rowScales[k];
    }
  }
  x.rows = c.rows;
  x.cols = c.cols;
  x.rowOut = c.rowOut ? 1 : 0;

  // ---- layout: the tile kernel needs whole 16-byte groups everywhere and
  // 4-byte destination scale pointers (the partial is scratch: aligned) ----
  bool tiles = c.cols % kMxGroupElts == 0;
  for (int s = 0; s < nSrcs; s++) tiles &= aligned(srcs[s], 16);
  for (int d = 0; d < nDsts; d++) {
    tiles &= aligned(colDsts[d], 16) && aligned(c.colScales[d], 4);
    if (c.rowOut) tiles &= aligned(c.rowDsts[d], 16) && aligned(c.rowScales[d], 4);
  }

  const size_t cus = (size_t)cuCount(launchDevice(c.stream));
  const int flags = (partFirst ? kLaunchPartFirst : 0) | (c.scaled ? kLaunchMxScaled : 0);
  const size_t tr = (c.rows + kMx2dTileRows - 1) / kMx2dTileRows;
  void* args[] = {&a, &x};
  hipError_t err;
  if (tiles) {
    // the small-tile rule of the pack launches: one group per lane and source
    const size_t nTiles = tr * ((c.cols + kMx2dTileCols - 1) / kMx2dTileCols);
    const size_t grid = cappedGrid(nTiles, cus * (size_t)maxBlocksPerCU(false, nSrcs));
    err = hipLaunchKernel(c.ms->tiles[c.out][slot0][nSrcs - 1], dim3((unsigned)grid), dim3(kBlock), args, 0, c.stream);
    logLaunch(kFamMx2dTiles, nSrcs, 1, flags);
  } else {
    const size_t waves = tr * ((c.cols + kMx2dWaveCols - 1) / kMx2dWaveCols), perWG = kBlock / 64;
    const size_t grid = cappedGrid((waves + perWG - 1) / perWG, cus * (size_t)maxBlocksPerCU(false, nSrcs, true));
    err = hipLaunchKernel(c.ms->generic[c.out][slot0], dim3((unsigned)grid), dim3(kBlock), args, 0, c.stream);
    logLaunch(kFamMx2dGeneric, nSrcs, 1, flags);
  }
  if (err != hipSuccess) {
    std::fprintf(stderr, "nbx: MX 2-D kernel launch failed: %s\n", hipGetErrorString(err));
    return ncclUnhandledCudaError;
  }
  return ncclSuccess;
}
}  // namespace
}  // namespace nbx

using namespace nbx;

NBX_EXPORT ncclResult_t nbxReduceMultiWideMx2d(void* const* rowDsts, void* const* rowScales, void* const* colDsts,
                                               void* const* colScales, int nDsts, const void* const* srcs,
                                               const void* const* srcScales, int nSrcs, size_t rows, size_t cols,
                                               ncclDataType_t srcType, ncclDataType_t dstType, nbxDevRedOpFull op,
                                               int nPreOpSrcs, ncclStream_t stream) {
  // ---- checks: all of them before any device call ----
  if (!argArraysOk(colDsts, nDsts, srcs, nSrcs) || colScales == nullptr) return ncclInvalidArgument;
  const bool rowOut = rowDsts != nullptr;
  if (rowOut != (rowScales != nullptr)) return ncclInvalidArgument;
  const bool scaled = srcScales != nullptr;
  int kind, out;
  ncclResult_t cr = checkMxTypes(srcType, dstType, op, scaled, true, &kind, &out);
  if (cr != ncclSuccess) return cr;
  if (kind >= kMxFp8Kinds) return ncclInvalidArgument;   // the MXFP8 kinds, and so the MX fp8 outputs, alone
  if (rows == 0 || cols == 0) return ncclSuccess;
  if (rows > SIZE_MAX / cols) return ncclInvalidArgument;
  if (scaled && cols % kMxBlockElts != 0) return ncclInvalidArgument;   // the sources' blocks are the flat bucket's
  const size_t count = rows * cols;
  const size_t eb = (size_t)typeSize((int)srcType);
  if (!pointersOk(eb, 1, colDsts, nDsts, srcs, nSrcs)) return ncclInvalidArgument;
  // every array written, then every array read; nothing written may overlap anything else
  Span sp[4 * NBX_MAX_DSTS + 2 * NBX_MAX_SRCS];
  int nw = 0;
  const size_t colScaleBytes = (rows + kMxBlockElts - 1) / kMxBlockElts * cols;
  const size_t rowScaleBytes = rows * ((cols + kMxBlockElts - 1) / kMxBlockElts);
  for (int d = 0; d < nDsts; d++) {
    sp[nw++] = {colDsts[d], count};
    sp[nw++] = {colScales[d], colScaleBytes};
    if (rowOut) {
      sp[nw++] = {rowDsts[d], count};
      sp[nw++] = {rowScales[d], rowScaleBytes};
    }
  }
  int n = nw;
  for (int s = 0; s < nSrcs; s++) {
    sp[n++] = {srcs[s], count * eb};
    if (scaled) sp[n++] = {srcScales[s], count / kMxBlockElts};
  }
  for (int i = 0; i < n; i++)
    if (sp[i].p == nullptr) return ncclInvalidArgument;
  for (int i = 0; i < nw; i++)
    for (int j = i + 1; j < n; j++)
      if (overlaps(sp[i].p, sp[i].bytes, sp[j].p, sp[j].bytes)) return ncclInvalidArgument;

  Mx2dCall c;
  c.ms = &mx2dTable()[kind];
  c.out = out;
  c.scaled = scaled;
  c.rowOut = rowOut;
  c.rows = rows;
  c.cols = cols;
  c.rowDsts = rowDsts;
  c.rowScales = rowScales;
  c.colScales = colScales;
  c.srcScales = srcScales;
  c.op = wideScalarOp(op);
  c.stream = (hipStream_t)stream;
  if (nPreOpSrcs < 0) nPreOpSrcs = 0;
  const bool pre = op.op == nbxDevPreMulSum;
  if (nSrcs <= kMaxKSrcs)
    return launchMx2dPass(c, false, colDsts, nDsts, srcs, nSrcs, 0, preMask(pre, nPreOpSrcs, 0, nSrcs, 0));

  // > 8 sources: the flat fp32 left fold of all but the last 7 goes to
  // stream-ordered scratch, never narrowed (itself in passes beyond 8: the same
  // ordered fp32 operations however the passes are cut), and the 2-D pass is
  // the PART kernel over the partial and the last 7.
  void* part = nullptr;
  if (hipMallocAsync(&part, count * sizeof(float), c.stream) != hipSuccess) return ncclUnhandledCudaError;
  const int first = nSrcs - (kMaxKSrcs - 1);
  void* partDst[1] = {part};
  cr = scaled ? nbxReduceMultiWideMx(partDst, nullptr, 1, srcs, srcScales, first, count, srcType, ncclFloat32, op,
                                     nPreOpSrcs, stream)
              : reduceMultiWideEx(partDst, 1, srcs, first, count, srcType, ncclFloat32, op, nPreOpSrcs, stream, 0);
  if (cr == ncclSuccess) {
    const void* ps[kMaxKSrcs];
    ps[0] = part;
    for (int k = 1; k < kMaxKSrcs; k++) ps[k] = srcs[first + k - 1];
    cr = launchMx2dPass(c, true, colDsts, nDsts, ps, kMaxKSrcs, first,
                        preMask(pre, nPreOpSrcs, first, kMaxKSrcs - 1, 1));
  }
  if (hipFreeAsync(part, c.stream) != hipSuccess && cr == ncclSuccess) cr = ncclUnhandledCudaError;
  return cr;
}

// The tile kernel's tile (test hook, include/nbx_debug.h).
NBX_EXPORT int nbxDebugMx2dTileShape(int* tileRows, int* tileCols) {
  if (tileRows) *tileRows = kMx2dTileRows;
  if (tileCols) *tileCols = kMx2dTileCols;
  return kMx2dTileRows * kMx2dTileCols;
}
