// nbx_mx_batch.h — work-list batch of the MXFP8 block-scaled sums
// (nbxReduceMultiWideMxBatch, include/nbx_reduce.h).
//
// kMxBatchList<W, SCALED, O, NSRC> is kWideBatchList's scheduler
// (nbx_wide_batch.inc: the records in BatchListArgs::recs, the running tile
// totals in the kernel arguments, chunks of `chunk` consecutive tiles taken
// round-robin, the 64-wide ballot search for a tile's record, no LDS and no
// barrier) around kMxBlocks' per-tile work at U = 1 (nbx_mx.h: mxLoadTile and
// mxFoldStore as they are, so the bits are the single call's).
//
// Tile: one 16-element group per lane, kMxBatchTileGroups = 256 groups = 128
// blocks = 4096 elements for every source type (a 16-bit group is two adjacent
// packs). A bucket of n groups owns ceil(n / 256) tiles, at least one. Blocks
// count from the bucket's element 0 and every element pointer is 16-byte
// aligned, so there is no head: the record (nbx_kargs.h) has no such field.
//   * a full tile stores its scale bytes in the GATHER form, 8 dwords per
//     wave: tile t of a bucket starts at scale byte 128 t of a 4-byte aligned
//     array, and lane 8 j's dword covers the blocks of lanes 8 j .. 8 j + 7;
//   * the bucket's last, partial tile stores them as bytes from the even
//     lanes (a dword could reach past the array);
//   * the count % 32 elements of a partial last block are done at the
//     bucket's last tile by half of wave 0, one element per lane: mxEltLane on
//     a view of the record's pointers. A bucket below one block is that alone.
// Not here: a partial-first form (a bucket of more than 8 sources never enters
// a table), a dynamic tile schedule, statistics.
#pragma once
#include "nbx_mx.h"

namespace nbx {

template <class W, bool SCALED, class O, int NSRC>
__global__ __launch_bounds__(kBlock) void kMxBatchList(BatchListArgs a) {
  constexpr int NPK = 16 / W::kEPP;
  constexpr bool MXOUT = !O::kF32;
  // word offsets in a record: the sources, their scales, the destinations
  constexpr int kSrcAt = 3, kSrcScaleAt = kSrcAt + NSRC, kDstAt = kSrcAt + NSRC * (SCALED ? 2 : 1);
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint32_t preMask = a.preMask;
  const bool pre = preMask != 0;   // uniform per launch: the fold is chosen per tile
  float mul[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) mul[s] = ((preMask >> s) & 1u) ? sc : 1.0f;
  const uint64_t T = a.totalTiles, C = a.chunk, step = (uint64_t)gridDim.x * C;
  const int nRecs = a.nRecs, lane = (int)(threadIdx.x & 63u);
  // destinations of the launch's widest record: its destination scales start behind them
  const int maxD = ((int)a.recWords - kDstAt) / (MXOUT ? 2 : 1);
  int k = -1;
  uint64_t tBegin = 0, tEnd = 0, nElts = 0, n = 0;
  int nDsts = 1;
  const u32x4* src[NSRC];
  const uint8_t* ss[NSRC];
  u32x4* dst[kMaxKDsts];
  uint8_t* ds[kMaxKDsts];
#pragma unroll
  for (int s = 0; s < NSRC; s++) ss[s] = nullptr;
#pragma unroll
  for (int d = 0; d < kMaxKDsts; d++) ds[d] = nullptr;
  for (uint64_t c0 = (uint64_t)blockIdx.x * C; c0 < T; c0 += step) {
    const uint64_t c1 = c0 + C < T ? c0 + C : T;
    for (uint64_t tile = c0; tile < c1; tile++) {
      if (tile >= tEnd) {   // next bucket holding this tile (uniform per wave)
        for (int base = k + 1;; base += 64) {
          const int idx = base + lane;
          const uint64_t e = idx < nRecs ? (uint64_t)a.tileEnd[idx] : ~0ull;
          const uint64_t m = __ballot(e > tile);
          if (m != 0) {
            k = __builtin_amdgcn_readfirstlane(base + (int)__builtin_ctzll(m));
            break;
          }
        }
        const uint64_t* r = a.recs + (uint64_t)k * a.recWords;
        tBegin = r[0];
        tEnd = r[1];
        const uint64_t meta = r[2];
        nDsts = (int)(meta >> 60);
        nElts = meta & kBatchCountMask;
        n = (nElts / kMxBlockElts) * (kMxBlockElts / kMxGroupElts);   // the groups of the full blocks: even
#pragma unroll
        for (int s = 0; s < NSRC; s++) {
          src[s] = (const u32x4*)r[kSrcAt + s];
          if constexpr (SCALED) ss[s] = (const uint8_t*)r[kSrcScaleAt + s];
        }
#pragma unroll
        for (int d = 0; d < kMaxKDsts; d++) {
          const int slot = d < nDsts ? d : 0;
          dst[d] = (u32x4*)r[kDstAt + slot];
          if constexpr (MXOUT) ds[d] = (uint8_t*)r[kDstAt + maxD + slot];
        }
      }
      const uint64_t g0 = (tile - tBegin) * kMxBatchTileGroups;
      const uint64_t g = g0 + threadIdx.x;
      u32x4 part[1][4];   // no partial-first form: unused
      u32x4 v[NSRC][1][NPK];
      uint32_t e[NSRC][1];
      if (g0 + kMxBatchTileGroups <= n) {
        // full tile (uniform): every load issued before the fold starts
        mxLoadTile<W, SCALED, NSRC, 1, false>(part, v, e, src, ss, g);
        __builtin_amdgcn_sched_barrier(0);
        if (pre) mxFoldStore<W, SCALED, O, NSRC, 1, false, true, true>(part, v, e, mul, dst, ds, nDsts, g);
        else mxFoldStore<W, SCALED, O, NSRC, 1, false, false, true>(part, v, e, mul, dst, ds, nDsts, g);
      } else if (g < n) {
        // the bucket's last, partial tile: n is even, so a pair is in or out together
        mxLoadTile<W, SCALED, NSRC, 1, false>(part, v, e, src, ss, g);
        mxFoldStore<W, SCALED, O, NSRC, 1, false, true, false>(part, v, e, mul, dst, ds, nDsts, g);
      }
      // the partial last block (count % 32 elements), at the bucket's last tile
      const int rest = (int)(nElts & (uint64_t)(kMxBlockElts - 1));
      if (tile == tEnd - 1 && rest != 0 && threadIdx.x < 64) {
        KArgs ea;   // the fields mxEltLane reads, from the record
        MxArgs ex;
#pragma unroll
        for (int s = 0; s < NSRC; s++) {
          ea.src[s] = src[s];
          ex.srcScale[s] = ss[s];
        }
#pragma unroll
        for (int d = 0; d < kMaxKDsts; d++) {
          ea.dst[d] = dst[d];
          ex.dstScale[d] = ds[d];
        }
        ea.preMask = preMask;
        ea.nDsts = nDsts;
        mxEltLane<W, SCALED, O, false>(ea, ex, sc, NSRC, n >> 1, lane & 31, lane < 32 ? rest : 0);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Launch table of one source kind (MxBatchSet, nbx_kargs.h).

template <class W, bool SCALED, class O, int... I>
void fillMxBatchOut(MxBatchSet& bs, std::integer_sequence<int, I...>) {
  const void* list[] = {(const void*)&kMxBatchList<W, SCALED, O, I + 1>...};
  for (int i = 0; i < kMaxKSrcs; i++) bs.list[O::kIndex][i] = list[i];
}

// The outputs of makeMxSet: MX for every kind, fp32 for the scaled ones.
template <class Ty, bool SCALED>
MxBatchSet makeMxBatchSet() {
  using W = WideTy<Ty>;
  MxBatchSet bs{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs> all{};
  fillMxBatchOut<W, SCALED, MxOutE4M3>(bs, all);
  fillMxBatchOut<W, SCALED, MxOutE5M2>(bs, all);
  if constexpr (SCALED) fillMxBatchOut<W, SCALED, MxOutF32>(bs, all);
  bs.valid = 1;
  return bs;
}

}  // namespace nbx
