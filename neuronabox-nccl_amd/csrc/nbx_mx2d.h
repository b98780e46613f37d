// nbx_mx2d.h — 2-D form of the MXFP8 block-scaled sums (nbxReduceMultiWideMx2d,
// include/nbx_reduce.h): a row-major rows x cols bucket folded once and stored
// twice, with 32-element blocks down the columns and (when asked) along the
// rows. The fold and the per-block rule are nbx_mx.h's (mxFoldAcc, mxFoldElt,
// mxScaleOut); new is that a column block spans 32 rows, which is several
// waves.
//
// Two kernels per (source kind, output, partial-first):
//   * kMx2dTiles<W, SCALED, O, NSRC, PART>: every element pointer 16-byte
//     aligned, cols a multiple of 16, every destination scale pointer 4-byte
//     aligned. A workgroup owns a tile of 32 rows x 128 columns; lane l holds
//     the 16-element group l % 8 of row l / 8, kMxBlocks's register shape, so a
//     wave holds 8 rows x 128 columns. Loads source-major ahead of the fold
//     (mxLoadTile), the fold is mxFoldAcc, and the 16 accumulators then stay in
//     registers until both copies are stored.
//       row-wise   as kMxBlocks: the lane's maximum, mxPairSwap for the block's,
//                  one multiply, narrowWord, one dwordx4 store. With cols a
//                  multiple of 128 a row's four scale bytes of the tile leave
//                  as one dword over DPP row shifts, else as bytes.
//       column-wise the lane's 16 magnitudes are reduced over the wave's 8 rows
//                  (lanes l, l + 8, ..., l + 56: one DPP row_ror:8 inside the
//                  row of 16, then xor 16 and xor 32 across rows), lanes 0 - 7
//                  of each wave write the wave's 128 column maxima to LDS
//                  (4 waves x 512 bytes), one workgroup barrier, and every lane
//                  reads the four partials of its 16 columns (ds_read_b128),
//                  derives 16 (S, R) pairs, multiplies, narrows and stores one
//                  dwordx4. The lanes of the tile's first row store its 128
//                  scale bytes, 16 each.
//     The LDS block is double-buffered by tile parity, so one barrier per tile
//     is enough: a wave cannot reach the write of tile t + 2 before every wave
//     has passed the barrier of tile t + 1, which lies behind its reads of tile
//     t. Static tile schedule; all 256 lanes reach the barrier in every tile.
//     Rows past `rows` and groups past `cols` load and store nothing and
//     contribute magnitude 0. No fp32 value goes to memory, nothing is read twice.
//   * kMx2dGeneric<W, SCALED, O, PART>: any layout. A wave takes 32 rows x 64
//     columns, one column per lane (loads coalesce across lanes). Pass 1 folds
//     the lane's 32 elements for the column's maximum, and stores the row-wise
//     copy on the way (a row block is half a wave: mxEltLane's xor butterfly);
//     pass 2 folds them again and stores the column-wise codes. The sources
//     are read twice, which is why the call has no in-place form.
// The same operations on the same values in the same order: the same bits.
#pragma once
#include "nbx_mx.h"

namespace nbx {

// The value of lane ^ 8 (row_ror:8 in the row of 16).
__device__ __forceinline__ uint32_t mxRowRor8(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t mxMaxU(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ u32x4 mxMaxU4(u32x4 a, u32x4 b) {
  return u32x4{mxMaxU(a.x, b.x), mxMaxU(a.y, b.y), mxMaxU(a.z, b.z), mxMaxU(a.w, b.w)};
}
// 16 bytes at a 4-byte aligned address (the column scales of a group)
typedef u32x4 u32x4a4 __attribute__((aligned(4)));

template <class W, bool SCALED, class O, int NSRC, bool PART>
__global__ __launch_bounds__(kBlock) void kMx2dTiles(KArgs a, Mx2dArgs x) {
  constexpr int NPK = 16 / W::kEPP;
  constexpr int kWaves = kBlock / 64, kQuads = kMx2dTileCols / 4;
  static_assert(!PART || NSRC >= 2, "a pass that reads a partial folds at least one more source");
  __shared__ u32x4 colMax[2][kWaves][kQuads];   // [tile parity][wave][column / 4]
  const float sc = loadWideArg(a.argPtr, a.arg);
  const u32x4* src[NSRC];
  const uint8_t* ss[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) {
    src[s] = (const u32x4*)a.src[s];
    ss[s] = x.srcScale[s];
  }
  u32x4* cdst[kMaxKDsts];
  u32x4* rdst[kMaxKDsts];
  uint8_t* cs[kMaxKDsts];
  uint8_t* rs[kMaxKDsts];
#pragma unroll
  for (int d = 0; d < kMaxKDsts; d++) {
    cdst[d] = (u32x4*)a.dst[d];
    rdst[d] = (u32x4*)x.rowDst[d];
    cs[d] = x.colScale[d];
    rs[d] = x.rowScale[d];
  }
  const int nDsts = a.nDsts;
  const bool pre = a.preMask != 0;      // uniform
  const bool rowOut = x.rowOut != 0;    // uniform
  float mul[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) mul[s] = ((a.preMask >> s) & 1u) ? sc : 1.0f;
  const uint64_t rows = x.rows, cols = x.cols;
  const uint64_t tilesC = (cols + kMx2dTileCols - 1) / kMx2dTileCols;
  const uint64_t tilesR = (rows + kMx2dTileRows - 1) / kMx2dTileRows;
  const uint64_t rowBlocks = (cols + kMxBlockElts - 1) / kMxBlockElts;   // scale bytes per row of the row-wise copy
  const bool gather = cols % kMx2dTileCols == 0;   // uniform: no partial tile across, rowBlocks a multiple of 4
  const int lane = (int)threadIdx.x, wave = lane >> 6, grp = lane & 7;
  int par = 0;
  forEachTile(a, tilesR * tilesC, [&](uint64_t t) {
    const uint64_t tr = t / tilesC, tc = t - tr * tilesC;
    const uint64_t r = tr * kMx2dTileRows + (uint64_t)(lane >> 3);
    const uint64_t c = tc * kMx2dTileCols + (uint64_t)grp * kMxGroupElts;
    const bool on = r < rows && c < cols;
    const uint64_t q = (r * cols + c) / kMxGroupElts;   // the group's index in the flat bucket (cols % 16 == 0)
    f32x2 acc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = f32x2{0.0f, 0.0f};
    if (on) {
      u32x4 part[1][4];
      u32x4 v[NSRC][1][NPK];
      uint32_t e[NSRC][1];
      mxLoadTile<W, SCALED, NSRC, 1, PART>(part, v, e, src, ss, q);
      __builtin_amdgcn_sched_barrier(0);
      if (pre) mxFoldAcc<W, SCALED, NSRC, 1, PART, true>(part, v, e, mul, 0, acc);
      else mxFoldAcc<W, SCALED, NSRC, 1, PART, false>(part, v, e, mul, 0, acc);
    }
    uint32_t mag[16];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      mag[2 * k] = mxMag(acc[k][0]);
      mag[2 * k + 1] = mxMag(acc[k][1]);
    }

    // ---- row-wise copy: kMxBlocks's rule; a lane that is off holds zeros ----
    if (rowOut) {
      uint32_t mb = 0;
#pragma unroll
      for (int k = 0; k < 16; k++) mb = mxMaxU(mb, mag[k]);
      mb = mxMaxU(mb, mxPairSwap(mb));
      uint32_t S;
      float R;
      mxScaleOut<O::kEmax>(mb, S, R);
      const f32x2 rr = {R, R};
      f32x2 sa[8];
#pragma unroll
      for (int k = 0; k < 8; k++) sa[k] = acc[k] * rr;
      u32x4 o;
#pragma unroll
      for (int w = 0; w < 4; w++) o[w] = O::W::narrowWord(&sa[w * 2]);
      if (on) {
#pragma unroll
        for (int d = 0; d < kMaxKDsts; d++)
          if (d < nDsts) stPack(rdst[d] + q, o);
      }
      if (gather) {
        // lane 8 j holds the first of its row's four blocks of this tile
        const uint32_t word = S | (mxRowShl<2>(S) << 8) | (mxRowShl<4>(S) << 16) | (mxRowShl<6>(S) << 24);
        if (on && grp == 0) {
          const uint64_t at = r * rowBlocks + tc * (kMx2dTileCols / kMxBlockElts);
#pragma unroll
          for (int d = 0; d < kMaxKDsts; d++)
            if (d < nDsts) *(uint32_t*)(rs[d] + at) = word;
        }
      } else if (on && (grp & 1) == 0) {
        const uint64_t at = r * rowBlocks + c / kMxBlockElts;
#pragma unroll
        for (int d = 0; d < kMaxKDsts; d++)
          if (d < nDsts) rs[d][at] = (uint8_t)S;
      }
    }

    // ---- column-wise copy: the wave's 8 rows, then the 4 waves through LDS ----
#pragma unroll
    for (int k = 0; k < 16; k++) {
      uint32_t m = mxMaxU(mag[k], mxRowRor8(mag[k]));
      m = mxMaxU(m, (uint32_t)__shfl_xor((int)m, 16, 64));
      mag[k] = mxMaxU(m, (uint32_t)__shfl_xor((int)m, 32, 64));
    }
    if ((lane & 63) < 8) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        colMax[par][wave][grp * 4 + j] = u32x4{mag[4 * j], mag[4 * j + 1], mag[4 * j + 2], mag[4 * j + 3]};
    }
    __syncthreads();
    u32x4 sw;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      u32x4 m = colMax[par][0][grp * 4 + j];
#pragma unroll
      for (int w = 1; w < kWaves; w++) m = mxMaxU4(m, colMax[par][w][grp * 4 + j]);
      uint32_t word = 0;
#pragma unroll
      for (int i = 0; i < 4; i += 2) {
        uint32_t S0, S1;
        float R0, R1;
        mxScaleOut<O::kEmax>(m[i], S0, R0);
        mxScaleOut<O::kEmax>(m[i + 1], S1, R1);
        acc[2 * j + i / 2] = acc[2 * j + i / 2] * f32x2{R0, R1};
        word |= (S0 << (8 * i)) | (S1 << (8 * i + 8));
      }
      sw[j] = word;
    }
    par ^= 1;
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; w++) o[w] = O::W::narrowWord(&acc[w * 2]);
    if (on) {
#pragma unroll
      for (int d = 0; d < kMaxKDsts; d++)
        if (d < nDsts) stPack(cdst[d] + q, o);
    }
    // the tile's first row (always inside the bucket) stores the scale bytes
    if (lane < 8 && c < cols) {
      const uint64_t at = tr * cols + c;
#pragma unroll
      for (int d = 0; d < kMaxKDsts; d++)
        if (d < nDsts) *(u32x4a4*)(cs[d] + at) = sw;
    }
  });
}

// Any layout: a wave per 32 rows x 64 columns, a lane per column. The trip
// counts are the wave's, so every shuffle is converged.
template <class W, bool SCALED, class O, bool PART>
__global__ __launch_bounds__(kBlock) void kMx2dGeneric(KArgs a, Mx2dArgs x) {
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint64_t rows = x.rows, cols = x.cols;
  const uint64_t tilesC = (cols + kMx2dWaveCols - 1) / kMx2dWaveCols;
  const uint64_t tilesR = (rows + kMx2dTileRows - 1) / kMx2dTileRows;
  const uint64_t rowBlocks = (cols + kMxBlockElts - 1) / kMxBlockElts;
  constexpr uint64_t kWaves = kBlock / 64;
  const int lane = (int)(threadIdx.x & 63u);
  const bool rowOut = x.rowOut != 0;   // uniform
  const int nSrcs = a.nSrcs;
  for (uint64_t wt = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); wt < tilesR * tilesC;
       wt += (uint64_t)gridDim.x * kWaves) {
    const uint64_t tr = wt / tilesC, tc = wt - tr * tilesC;
    const uint64_t r0 = tr * kMx2dTileRows, c = tc * kMx2dWaveCols + (uint64_t)lane;
    const bool on = c < cols;
    const int nr = rows - r0 < (uint64_t)kMx2dTileRows ? (int)(rows - r0) : kMx2dTileRows;
    // pass 1: the column's maximum, and the row-wise copy on the way
    uint32_t cm = 0;
    for (int i = 0; i < nr; i++) {
      const uint64_t idx = (r0 + (uint64_t)i) * cols + c;
      const float acc = on ? mxFoldElt<W, SCALED, PART>(a, x.srcScale, sc, nSrcs, idx, idx / kMxBlockElts) : 0.0f;
      const uint32_t m = mxMag(acc);
      cm = mxMaxU(cm, m);
      if (rowOut) {
        uint32_t mb = m;
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) mb = mxMaxU(mb, (uint32_t)__shfl_xor((int)mb, o, 64));
        uint32_t S;
        float R;
        mxScaleOut<O::kEmax>(mb, S, R);
        if (on) {
          const uint8_t code = O::W::narrow(acc * R);
          const uint64_t at = (r0 + (uint64_t)i) * rowBlocks + c / kMxBlockElts;
#pragma unroll
          for (int d = 0; d < kMaxKDsts; d++) {
            if (d < a.nDsts) {
              ((uint8_t*)x.rowDst[d])[idx] = code;
              if ((lane & 31) == 0) x.rowScale[d][at] = (uint8_t)S;
            }
          }
        }
      }
    }
    uint32_t S;
    float R;
    mxScaleOut<O::kEmax>(cm, S, R);
    if (on) {
#pragma unroll
      for (int d = 0; d < kMaxKDsts; d++)
        if (d < a.nDsts) x.colScale[d][tr * cols + c] = (uint8_t)S;
      // pass 2: the same fold again, stored under the column's scale
      for (int i = 0; i < nr; i++) {
        const uint64_t idx = (r0 + (uint64_t)i) * cols + c;
        const float acc = mxFoldElt<W, SCALED, PART>(a, x.srcScale, sc, nSrcs, idx, idx / kMxBlockElts);
        const uint8_t code = O::W::narrow(acc * R);
#pragma unroll
        for (int d = 0; d < kMaxKDsts; d++)
          if (d < a.nDsts) ((uint8_t*)a.dst[d])[idx] = code;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Launch table of one source kind (Mx2dSet, nbx_kargs.h).

template <class W, bool SCALED, class O, int... I, int... J>
void fillMx2dOut(Mx2dSet& ms, std::integer_sequence<int, I...>, std::integer_sequence<int, J...>) {
  const void* first[] = {(const void*)&kMx2dTiles<W, SCALED, O, I + 1, false>...};
  const void* later[] = {nullptr, (const void*)&kMx2dTiles<W, SCALED, O, J + 2, true>...};
  for (int i = 0; i < kMaxKSrcs; i++) {
    ms.tiles[O::kIndex][0][i] = first[i];
    ms.tiles[O::kIndex][1][i] = later[i];
  }
  ms.generic[O::kIndex][0] = (const void*)&kMx2dGeneric<W, SCALED, O, false>;
  ms.generic[O::kIndex][1] = (const void*)&kMx2dGeneric<W, SCALED, O, true>;
}

template <class Ty, bool SCALED>
Mx2dSet makeMx2dSet() {
  using W = WideTy<Ty>;
  Mx2dSet ms{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs> all{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs - 1> fromTwo{};
  fillMx2dOut<W, SCALED, MxOutE4M3>(ms, all, fromTwo);
  fillMx2dOut<W, SCALED, MxOutE5M2>(ms, all, fromTwo);
  ms.valid = 1;
  return ms;
}

}  // namespace nbx
