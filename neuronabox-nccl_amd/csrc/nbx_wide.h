// nbx_wide.h — fp32-accumulating ("wide") multi-source sums for f16, bf16 and
// fp8 sources (nbxReduceMultiWide, include/nbx_reduce.h).
//
// The per-step kernels (nbx_kernels.h) narrow the accumulator to the element
// type after every source, as the reference's functors do. Here every source
// is widened once (the exact Ty*::wide / wide4 of nbx_functors.h), the sources
// are folded in order with fp32 adds (v_pk_add_f32; PreMulSum's multiply is a
// separate v_pk_mul_f32, never fused: -ffp-contract=off), and the accumulator
// is either narrowed once (the type's own narrowing: RNE, fp8 behind
// satFinite) or stored as fp32.
//
// Three kernels per (type, output kind, partial-first):
//   * kWidePacks<W, NSRC, U, OUT32, PART>: the kReducePacks shape — each lane
//     issues all NSRC x U 16-byte nt loads of a tile, then folds pack by pack
//     (8 fp32 accumulators for a 16-bit pack, 16 for an fp8 pack) and stores
//     one dwordx4 per destination (narrow output) or 2 / 4 of them (fp32
//     output). Needs every source on one misalignment modulo 16 and every
//     destination 16-byte aligned after the head elements are peeled.
//   * kWideShiftedLds<W, NSRC, OUT32, PART>: the kReduceShiftedLds shape —
//     packs on the destinations' side, the typed sources through LDS by
//     LDS-DMA and realigned on the LDS read. Needs the destinations on one
//     address modulo 16; taken from NBX_WIDE_SHIFT_MIN_ELTS elements.
//   * kWideElts<W, OUT32, PART>: one element per lane, any alignment: the
//     destinations on different alignments, and calls below that threshold.
// PART: source 0 is the fp32 partial of an earlier pass (more than 8 sources
// fold in passes of 8 + 7 + 7 ...; the partial is never narrowed, so the
// result is the single fp32 left fold over all sources).
// A third family, kWideBatchList<W, NSRC, OUT32>, runs many buckets from a
// work-list table in one launch (nbxReduceMultiWideBatch; below).
#pragma once
#include "nbx_kernels.h"   // ldPack / stPack, forEachTile

namespace nbx {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// Wide view of an element type: kEPP elements per 16-byte pack, kWP fp32
// pairs per dword of codes.
template <class Ty>
struct WideTy;

template <>
struct WideTy<TyF16> {
  using Elt = uint16_t;
  static constexpr int kEPP = 8, kWP = 1;
  __device__ static float wide(Elt e) { return (float)TyF16::wide(e); }
  __device__ static Elt narrow(float c) { return TyF16::narrow((_Float16)c); }
  __device__ static void wideWord(uint32_t w, f32x2* f) {
    f[0] = __builtin_convertvector(__builtin_bit_cast(f16x2, w), f32x2);
  }
  __device__ static uint32_t narrowWord(const f32x2* f) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f[0], f16x2));
  }
};

template <>
struct WideTy<TyBF16> {
  using Elt = uint16_t;
  static constexpr int kEPP = 8, kWP = 1;
  __device__ static float wide(Elt e) { return TyBF16::wide(e); }
  __device__ static Elt narrow(float c) { return TyBF16::narrow(c); }
  __device__ static void wideWord(uint32_t w, f32x2* f) {
    f[0] = f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
  }
  __device__ static uint32_t narrowWord(const f32x2* f) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f[0], bf16x2));   // v_cvt_pk_bf16_f32
  }
};

template <class Ty>
struct WideTyF8 {
  using Elt = uint8_t;
  static constexpr int kEPP = 16, kWP = 2;
  __device__ static float wide(Elt e) { return Ty::wide(e); }
  __device__ static Elt narrow(float c) { return Ty::narrow(c); }
  __device__ static void wideWord(uint32_t w, f32x2* f) {
    float x[4];
    Ty::wide4(w, x);
    f[0] = f32x2{x[0], x[1]};
    f[1] = f32x2{x[2], x[3]};
  }
  __device__ static uint32_t narrowWord(const f32x2* f) {
    const uint32_t lo = Ty::narrow2(f[0][0], f[0][1], 0u, false);
    return Ty::narrow2(f[1][0], f[1][1], lo, true);
  }
};
template <>
struct WideTy<TyE4M3> : WideTyF8<TyE4M3> {};
template <>
struct WideTy<TyE5M2> : WideTyF8<TyE5M2> {};

// The PreMulSum scalar is an fp32 value: the low 32 bits of scalarArg, or a
// float in device memory read while the kernel runs.
__device__ __forceinline__ float loadWideArg(const void* argPtr, uint64_t arg) {
  return argPtr != nullptr ? *(const float*)argPtr : __uint_as_float((uint32_t)arg);
}

// One element, any source count <= kMaxKSrcs (uniform guards, as reduceElt).
template <class W, bool OUT32, bool PART>
__device__ __forceinline__ void wideElt(const KArgs& a, float sc, int nSrcs, uint64_t i) {
  using E = typename W::Elt;
  float acc;
  if constexpr (PART) {
    acc = ((const float*)a.src[0])[i];
  } else {
    acc = W::wide(((const E*)a.src[0])[i]);
    if (a.preMask & 1u) acc = acc * sc;
  }
#pragma unroll
  for (int s = 1; s < kMaxKSrcs; s++) {
    if (s < nSrcs) {
      float v = W::wide(((const E*)a.src[s])[i]);
      if ((a.preMask >> s) & 1u) v = v * sc;
      acc = acc + v;
    }
  }
#pragma unroll
  for (int d = 0; d < kMaxKDsts; d++) {
    if (d < a.nDsts) {
      if constexpr (OUT32) ((float*)a.dst[d])[i] = acc;
      else ((E*)a.dst[d])[i] = W::narrow(acc);
    }
  }
}

// One 16-byte pack of codes -> its kEPP / 2 fp32 pairs.
template <class W>
__device__ __forceinline__ void widePack(const u32x4& v, f32x2 (&f)[W::kEPP / 2]) {
#pragma unroll
  for (int w = 0; w < 4; w++) W::wideWord(v[w], &f[w * W::kWP]);
}

// Fold U packs already in registers and store them. part[u][j] is source 0
// as fp32 (PART), v[s][u] the codes of source s (v[0] unused with PART).
// PRE (PreMulSum): source s is multiplied by mul[s], the scalar for a
// pre-multiplied source and 1.0 for the others — x * 1.0 is x, so one
// multiply per element whatever the mask, and no multiply at all in the
// plain sum (a per-source test of the mask inside the fold compiled into a
// multiply AND a select per element for every source).
template <class W, int NSRC, int U, bool OUT32, bool PART, bool PRE>
__device__ __forceinline__ void wideFoldStore(const u32x4 (&part)[U][W::kEPP / 4], const u32x4 (&v)[NSRC][U],
                                              const float (&mul)[NSRC], u32x4* const (&dst)[kMaxKDsts], int nDsts,
                                              uint64_t p) {
  constexpr int NP = W::kEPP / 2;   // fp32 pairs per pack
  constexpr int Q = W::kEPP / 4;    // dwordx4 per pack of fp32
#pragma unroll
  for (int u = 0; u < U; u++) {
    f32x2 acc[NP];
    if constexpr (PART) {
#pragma unroll
      for (int j = 0; j < Q; j++) {
        acc[2 * j] = f32x2{__uint_as_float(part[u][j].x), __uint_as_float(part[u][j].y)};
        acc[2 * j + 1] = f32x2{__uint_as_float(part[u][j].z), __uint_as_float(part[u][j].w)};
      }
    } else {
      widePack<W>(v[0][u], acc);
      if constexpr (PRE) {
        const f32x2 m = {mul[0], mul[0]};
#pragma unroll
        for (int k = 0; k < NP; k++) acc[k] = acc[k] * m;
      }
    }
#pragma unroll
    for (int s = 1; s < NSRC; s++) {
      f32x2 t[NP];
      widePack<W>(v[s][u], t);
      if constexpr (PRE) {
        const f32x2 m = {mul[s], mul[s]};
#pragma unroll
        for (int k = 0; k < NP; k++) t[k] = t[k] * m;
      }
#pragma unroll
      for (int k = 0; k < NP; k++) acc[k] = acc[k] + t[k];
    }
    const uint64_t q = p + (uint64_t)u * kBlock;
    if constexpr (OUT32) {
#pragma unroll
      for (int j = 0; j < Q; j++) {
        const u32x4 o = {__float_as_uint(acc[2 * j][0]), __float_as_uint(acc[2 * j][1]),
                         __float_as_uint(acc[2 * j + 1][0]), __float_as_uint(acc[2 * j + 1][1])};
        stPack(dst[0] + q * Q + j, o);
#pragma unroll
        for (int d = 1; d < kMaxKDsts; d++)
          if (d < nDsts) stPack(dst[d] + q * Q + j, o);
      }
    } else {
      u32x4 o;
#pragma unroll
      for (int w = 0; w < 4; w++) o[w] = W::narrowWord(&acc[w * W::kWP]);
      stPack(dst[0] + q, o);
#pragma unroll
      for (int d = 1; d < kMaxKDsts; d++)
        if (d < nDsts) stPack(dst[d] + q, o);
    }
  }
}

// Source-major issue order, as loadTile; the fp32 partial first.
template <class W, int NSRC, int U, bool PART>
__device__ __forceinline__ void wideLoadTile(u32x4 (&part)[U][W::kEPP / 4], u32x4 (&v)[NSRC][U],
                                             const u32x4* const (&src)[NSRC], uint64_t p) {
  constexpr int Q = W::kEPP / 4;
  if constexpr (PART) {
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int j = 0; j < Q; j++) part[u][j] = ldPack(src[0] + (p + (uint64_t)u * kBlock) * Q + j);
  }
#pragma unroll
  for (int s = PART ? 1 : 0; s < NSRC; s++)
#pragma unroll
    for (int u = 0; u < U; u++) v[s][u] = ldPack(src[s] + p + (uint64_t)u * kBlock);
}

template <class W, int NSRC, int U, bool OUT32, bool PART>
__global__ __launch_bounds__(kBlock) void kWidePacks(KArgs a) {
  using E = typename W::Elt;
  constexpr int EPP = W::kEPP, Q = EPP / 4;
  static_assert(!PART || NSRC >= 2, "a pass that reads a partial folds at least one more source");
  acquirePeerData(a);   // a clique's fold reads its peers' buffers (reduceMultiWideEx)
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint64_t head = (uint64_t)a.headElts;
  const u32x4* src[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++)
    src[s] = (const u32x4*)((const char*)a.src[s] + head * (PART && s == 0 ? sizeof(float) : sizeof(E)));
  u32x4* dst[kMaxKDsts];
#pragma unroll
  for (int d = 0; d < kMaxKDsts; d++) dst[d] = (u32x4*)((char*)a.dst[d] + head * (OUT32 ? sizeof(float) : sizeof(E)));
  const int nDsts = a.nDsts;
  const bool pre = a.preMask != 0;   // uniform: the fold is chosen per tile, never per element
  float mul[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) mul[s] = ((a.preMask >> s) & 1u) ? sc : 1.0f;
  const uint64_t n = a.nPacks;
  constexpr uint64_t kTile = (uint64_t)U * kBlock;
  forEachTile(a, (n + kTile - 1) / kTile, [&](uint64_t t) {
    const uint64_t p = t * kTile + threadIdx.x;
    if (p + (uint64_t)(U - 1) * kBlock < n) {
      // full tile: issue every load first, then fold
      u32x4 part[U][Q];
      u32x4 v[NSRC][U];
      wideLoadTile<W, NSRC, U, PART>(part, v, src, p);
      __builtin_amdgcn_sched_barrier(0);
      if (pre) wideFoldStore<W, NSRC, U, OUT32, PART, true>(part, v, mul, dst, nDsts, p);
      else wideFoldStore<W, NSRC, U, OUT32, PART, false>(part, v, mul, dst, nDsts, p);
    } else {
      // last, partial tile
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t q = p + (uint64_t)u * kBlock;
        if (q < n) {
          u32x4 part1[1][Q];
          u32x4 v1[NSRC][1];
          wideLoadTile<W, NSRC, 1, PART>(part1, v1, src, q);
          wideFoldStore<W, NSRC, 1, OUT32, PART, true>(part1, v1, mul, dst, nDsts, q);
        }
      }
    }
  });

  // head (< EPP elements before the aligned body) and tail (< EPP after it)
  if (blockIdx.x == gridDim.x - 1) {
    const int h = a.headElts;
    const uint64_t tailStart = head + n * EPP;
    const int tail = (int)(a.nElts - tailStart);
    const int t = (int)threadIdx.x;
    if (t < h) wideElt<W, OUT32, PART>(a, sc, NSRC, (uint64_t)t);
    else if (t < h + tail) wideElt<W, OUT32, PART>(a, sc, NSRC, tailStart + (uint64_t)(t - h));
  }
}

// Element kernel: sources on different alignments modulo 16, or a destination
// that is not 16-byte aligned behind the head.
template <class W, bool OUT32, bool PART>
__global__ __launch_bounds__(kBlock) void kWideElts(KArgs a) {
  acquirePeerData(a);
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < a.nElts; i += stride)
    wideElt<W, OUT32, PART>(a, sc, a.nSrcs, i);
}

// Realigning kernel: kReduceShiftedLds' staging (nbx_kernels.h — the typed
// sources through LDS by global_load_lds dwordx4 nt, a private two-stage buffer
// per wave, counted vmcnt between the stages, each output's 16 source bytes
// read back at its byte offset and funnelled with v_alignbyte) around
// wideFoldStore at one pack per call. The body is addressed on the destination
// side: `head` elements bring every destination to a 16-byte boundary, output
// pack q is one dwordx4 store per destination (source-type output) or kEPP / 4
// of them (fp32), and the sources sit on any alignment of their own. The fp32
// partial of a PART pass is 16-byte aligned behind `head` (nbxReduceMultiWide
// places it so), so it is read straight from global memory with ldPack —
// before the next tile's DMA is issued, so that the counted wait retires it
// together with this tile's DMA — and only the NSRC - 1 typed sources are
// staged. Static schedule only: wave gw takes wave tiles gw, gw + nWaves, ...
// Memory safety is kReduceShiftedLds': pack indices clamp to the last pack
// holding a byte of the source's range, and a body of 0 packs has 0 tiles, so
// no DMA is issued at all.
template <class W, int NSRC, bool OUT32, bool PART>
__global__ __launch_bounds__(kShiftLdsWaves * 64) void kWideShiftedLds(KArgs a) {
  using E = typename W::Elt;
  constexpr int EPP = W::kEPP, Q = EPP / 4;
  static_assert(!PART || NSRC >= 2, "a pass that reads a partial folds at least one more source");
  static_assert(kShiftLdsWaves * 64 == kBlock, "the head and tail elements count on kBlock lanes");
  constexpr int F = PART ? 1 : 0;   // first staged source
  constexpr int NST = NSRC - F;     // staged sources
  constexpr int U = shiftLdsUnroll(NSRC), S = kShiftLdsStages, WV = kShiftLdsWaves;
  constexpr int P = U * 64 + 1;     // packs per source per stage
  constexpr uint64_t kTile = (uint64_t)U * 64;
  __shared__ u32x4 sm[WV][S][NST][P];
  acquirePeerData(a);
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint64_t head = (uint64_t)a.headElts;
  const uint64_t n = a.nPacks;
  const u32x4* base[NSRC];
  uint32_t sh[NSRC];
  uint64_t lim[NSRC];
#pragma unroll
  for (int s = F; s < NSRC; s++) {
    alignDown16((uintptr_t)a.src[s] + head * sizeof(E), base[s], sh[s]);
    lim[s] = sh[s] ? n : (n ? n - 1 : 0);
  }
  const u32x4* partial = (const u32x4*)((const char*)a.src[0] + head * sizeof(float));   // PART only
  u32x4* dst[kMaxKDsts];
#pragma unroll
  for (int d = 0; d < kMaxKDsts; d++) dst[d] = (u32x4*)((char*)a.dst[d] + head * (OUT32 ? sizeof(float) : sizeof(E)));
  const int nDsts = a.nDsts;
  const bool pre = a.preMask != 0;   // uniform: the fold is chosen per tile, never per element
  float mul[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) mul[s] = ((a.preMask >> s) & 1u) ? sc : 1.0f;
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
  const uint64_t nTiles = (n + kTile - 1) / kTile;
  const uint64_t nWaves = (uint64_t)gridDim.x * WV, gw = (uint64_t)blockIdx.x * WV + (uint64_t)wave;
  auto issue = [&](uint64_t t, int st) {
    const uint64_t p0 = t * kTile;
#pragma unroll
    for (int s = F; s < NSRC; s++) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t q = p0 + (uint64_t)(u * 64 + lane);
        __builtin_amdgcn_global_load_lds((const void*)(base[s] + (q < lim[s] ? q : lim[s])),
                                         (__attribute__((address_space(3))) void*)&sm[wave][st][s - F][u * 64], 16, 0,
                                         2 /* nt */);
      }
      if (lane == 0) {
        const uint64_t q = p0 + kTile;
        __builtin_amdgcn_global_load_lds((const void*)(base[s] + (q < lim[s] ? q : lim[s])),
                                         (__attribute__((address_space(3))) void*)&sm[wave][st][s - F][kTile], 16, 0,
                                         2);
      }
    }
  };
  // the fp32 partial of wave tile t (lanes past the body read its last pack)
  auto loadPart = [&](uint64_t t, u32x4 (&part)[U][Q]) {
    if constexpr (PART) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t q = t * kTile + (uint64_t)(u * 64 + lane);
        const uint64_t qc = q < n ? q : n - 1;
#pragma unroll
        for (int j = 0; j < Q; j++) part[u][j] = ldPack(partial + qc * Q + j);
      }
    }
  };
  // fold wave tile t from stage st (its DMA has landed) and store it
  auto foldTile = [&](uint64_t t, int st, const u32x4 (&part)[U][Q]) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint64_t q = t * kTile + (uint64_t)(u * 64 + lane);
      if (q < n) {
        u32x4 part1[1][Q];
        u32x4 v1[NSRC][1];
        if constexpr (PART) {
#pragma unroll
          for (int j = 0; j < Q; j++) part1[0][j] = part[u][j];
        }
#pragma unroll
        for (int s = F; s < NSRC; s++) {
          v1[s][0] = stageRead(&sm[wave][st][s - F][0], sh[s], (uint32_t)(u * 64 + lane));
        }
        if (pre) wideFoldStore<W, NSRC, 1, OUT32, PART, true>(part1, v1, mul, dst, nDsts, q);
        else wideFoldStore<W, NSRC, 1, OUT32, PART, false>(part1, v1, mul, dst, nDsts, q);
      }
    }
    // this stage's LDS reads have returned before a later iteration refills it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
#pragma unroll
  for (int k = 0; k < S - 1; k++) {
    const uint64_t t = gw + (uint64_t)k * nWaves;
    if (t < nTiles) issue(t, k);
  }
  int st = 0;
  for (uint64_t t = gw; t < nTiles; t += nWaves) {
    u32x4 part[U][Q];
    loadPart(t, part);
    if (t + (uint64_t)(S - 1) * nWaves < nTiles) {
      issue(t + (uint64_t)(S - 1) * nWaves, (st + S - 1) % S);
      // everything but the newer tiles' DMA (NST x (U + 1) instructions each)
      // has landed: this tile's DMA and its partial; stores counted in vmcnt
      // only make the wait stricter
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((S - 1) * NST * (U + 1)) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    foldTile(t, st, part);
    st = st + 1 == S ? 0 : st + 1;
  }

  // head (before the destinations' 16-B boundary) and tail elements
  if (blockIdx.x == gridDim.x - 1) {
    const int h = a.headElts;
    const uint64_t tailStart = head + n * EPP;
    const int tail = (int)(a.nElts - tailStart);
    const int th = (int)threadIdx.x;
    if (th < h) wideElt<W, OUT32, PART>(a, sc, NSRC, (uint64_t)th);
    else if (th < h + tail) wideElt<W, OUT32, PART>(a, sc, NSRC, tailStart + (uint64_t)(th - h));
  }
}

// ---------------------------------------------------------------------------
// Batched buckets (nbxReduceMultiWideBatch): kReduceBatchList's scheduler
// (nbx_kernels.h — records from the table in BatchListArgs::recs, running tile
// totals in the kernel arguments, chunks of consecutive tiles round-robin, the
// 64-wide ballot search, no LDS and no barrier) around kWidePacks' per-tile
// work at U = 1. The record layout is the per-step one; `head` counts
// elements (<= 15, fp8), so an fp32 destination's body starts head floats in.
// Buckets of more than 8 sources never enter a batch: no partial-first form.

// One head or tail element: wideElt's arithmetic, the source count a
// template argument (as batchElt).
template <class W, int NSRC, bool OUT32>
__device__ __forceinline__ void wideBatchElt(const typename W::Elt* const (&src)[NSRC], void* const (&dst)[kMaxKDsts],
                                             int nDsts, uint32_t preMask, float sc, uint64_t i) {
  using E = typename W::Elt;
  float acc = W::wide(src[0][i]);
  if (preMask & 1u) acc = acc * sc;
#pragma unroll
  for (int s = 1; s < NSRC; s++) {
    float v = W::wide(src[s][i]);
    if ((preMask >> s) & 1u) v = v * sc;
    acc = acc + v;
  }
#pragma unroll
  for (int d = 0; d < kMaxKDsts; d++) {
    if (d < nDsts) {
      if constexpr (OUT32) ((float*)dst[d])[i] = acc;
      else ((E*)dst[d])[i] = W::narrow(acc);
    }
  }
}

template <class W, int NSRC, bool OUT32>
__global__ __launch_bounds__(kBlock) void kWideBatchList(BatchListArgs a) {
  using E = typename W::Elt;
  constexpr int EPP = W::kEPP, Q = EPP / 4;
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint32_t preMask = a.preMask;
  const bool pre = preMask != 0;   // uniform per launch: the fold is never chosen per element
  float mul[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) mul[s] = ((preMask >> s) & 1u) ? sc : 1.0f;
  const uint64_t T = a.totalTiles, C = a.chunk, step = (uint64_t)gridDim.x * C;
  const int nRecs = a.nRecs, lane = (int)(threadIdx.x & 63u);
  int k = -1;
  uint64_t tBegin = 0, tEnd = 0, nElts = 0, n = 0;
  int nDsts = 1, head = 0;
  const E* sb[NSRC];
  void* db[kMaxKDsts];
  const u32x4* src[NSRC];
  u32x4* dst[kMaxKDsts];
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
        head = (int)((meta >> 56) & 15u);
        n = (nElts - (uint64_t)head) / EPP;
#pragma unroll
        for (int s = 0; s < NSRC; s++) {
          sb[s] = (const E*)r[3 + s];
          src[s] = (const u32x4*)(sb[s] + head);
        }
#pragma unroll
        for (int d = 0; d < kMaxKDsts; d++) {
          db[d] = (void*)r[3 + NSRC + (d < nDsts ? d : 0)];
          dst[d] = (u32x4*)((char*)db[d] + (uint64_t)head * (OUT32 ? sizeof(float) : sizeof(E)));
        }
      }
      const uint64_t p = (tile - tBegin) * kBatchTilePacks + threadIdx.x;
      if (p < n) {
        u32x4 part[1][Q];   // no partial-first form: unused
        u32x4 v[NSRC][1];
#pragma unroll
        for (int s = 0; s < NSRC; s++) v[s][0] = ldPack(src[s] + p);
        // every load issued before the fold starts, as in kWidePacks (without
        // this the widening of the first sources is scheduled between the
        // loads, and a flat load's wait is a wait for all of them)
        __builtin_amdgcn_sched_barrier(0);
        if (pre) wideFoldStore<W, NSRC, 1, OUT32, false, true>(part, v, mul, dst, nDsts, p);
        else wideFoldStore<W, NSRC, 1, OUT32, false, false>(part, v, mul, dst, nDsts, p);
      }
      if (tile == tEnd - 1) {   // the bucket's last tile: its head and tail elements
        const uint64_t tailStart = (uint64_t)head + n * EPP;
        const int tail = (int)(nElts - tailStart);
        const int th = (int)threadIdx.x;
        if (th < head) wideBatchElt<W, NSRC, OUT32>(sb, db, nDsts, preMask, sc, (uint64_t)th);
        else if (th < head + tail)
          wideBatchElt<W, NSRC, OUT32>(sb, db, nDsts, preMask, sc, tailStart + (uint64_t)(th - head));
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Launch table for one source type (WideSet, nbx_kargs.h).

template <class W, bool OUT32, int... I, int... J>
void fillWidePacks(WideSet& ws, std::integer_sequence<int, I...>, std::integer_sequence<int, J...>) {
  const void* first[] = {(const void*)&kWidePacks<W, I + 1, wideUnroll(I + 1), OUT32, false>...};
  // a pass that reads a partial has two sources or more: slot 0 stays empty
  const void* later[] = {nullptr, (const void*)&kWidePacks<W, J + 2, wideUnroll(J + 2), OUT32, true>...};
  for (int i = 0; i < kMaxKSrcs; i++) {
    ws.packs[OUT32 ? 1 : 0][0][i] = first[i];
    ws.packs[OUT32 ? 1 : 0][1][i] = later[i];
  }
}

template <class W, bool OUT32, int... I>
void fillWideBatch(WideSet& ws, std::integer_sequence<int, I...>) {
  const void* list[] = {(const void*)&kWideBatchList<W, I + 1, OUT32>...};
  for (int i = 0; i < kMaxKSrcs; i++) ws.batchList[OUT32 ? 1 : 0][i] = list[i];
}

template <class W, bool OUT32, int... I, int... J>
void fillWideShifted(WideSet& ws, std::integer_sequence<int, I...>, std::integer_sequence<int, J...>) {
  const void* first[] = {(const void*)&kWideShiftedLds<W, I + 1, OUT32, false>...};
  const void* later[] = {nullptr, (const void*)&kWideShiftedLds<W, J + 2, OUT32, true>...};
  for (int i = 0; i < kMaxKSrcs; i++) {
    ws.shiftedLds[OUT32 ? 1 : 0][0][i] = first[i];
    ws.shiftedLds[OUT32 ? 1 : 0][1][i] = later[i];
  }
}

// The realigning kernels of one source type, added to its set by a unit of
// their own (inst_wide_shift*.hip: 30 kernels per type, compiled in parallel
// with the pack kernels).
template <class Ty>
void addWideShifted(WideSet& ws) {
  using W = WideTy<Ty>;
  constexpr std::make_integer_sequence<int, kMaxKSrcs> all{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs - 1> fromTwo{};
  fillWideShifted<W, false>(ws, all, fromTwo);
  fillWideShifted<W, true>(ws, all, fromTwo);
}

template <class Ty>
WideSet makeWideSet(int blocksPerCU) {
  using W = WideTy<Ty>;
  WideSet ws{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs> all{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs - 1> fromTwo{};
  fillWidePacks<W, false>(ws, all, fromTwo);
  fillWidePacks<W, true>(ws, all, fromTwo);
  fillWideBatch<W, false>(ws, all);
  fillWideBatch<W, true>(ws, all);
  ws.elts[0][0] = (const void*)&kWideElts<W, false, false>;
  ws.elts[0][1] = (const void*)&kWideElts<W, false, true>;
  ws.elts[1][0] = (const void*)&kWideElts<W, true, false>;
  ws.elts[1][1] = (const void*)&kWideElts<W, true, true>;
  ws.eltBytes = (int)sizeof(typename W::Elt);
  ws.blocksPerCU = blocksPerCU;
  ws.valid = 1;
  return ws;
}

}  // namespace nbx
