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
// Every kernel has a STATS form (k...Stats, nbxReduceMultiWideStats): the same
// body with the bucket statistics of the final accumulators folded in
// ("Bucket statistics" below). A plain kernel and its STATS form share their
// body as text (nbx_wide_*.inc), and the plain kernels are what they were.
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

// ---------------------------------------------------------------------------
// Bucket statistics (nbxReduceMultiWideStats): amax = max |acc| and sumSq =
// sum acc^2 over the final fp32 accumulators, taken where they sit in
// registers. A lane keeps two fp32 square-sums (one per half of an accumulator
// pair, one fma per element: one rounding) and one fp32 running max for the
// duration of ONE tile; at the tile's end the two sums are widened to fp64 and
// added, the wave folds sum and max over a fixed xor butterfly (fp64 adds are
// commutative, so every lane ends on the same bits) and lane 0 stores one
// 16-byte WideSlot at an index that depends on the tile and the wave alone:
//   pack kernel       tile * 4 + wave; head and tail elements: nTiles * 4
//   realigning kernel wave tile; head and tail elements: nTiles
//   element kernel    tile * 4 + wave, a tile being kWideEltsStatTile x kBlock elements
//   batch kernel      tile * 4 + k + wave for global tile `tile` of record k;
//                     record k's head and tail elements: tileEnd[k] * 4 + k
// Every slot of the range is written exactly once (zeros by a wave with no
// element), by whichever workgroup ran the tile: no LDS, no barrier, no
// atomic, and nothing depends on the grid or the tile schedule. kWideStatsReduce
// / kWideStatsBatch (inst_wide_stats_sum.hip) sum the slots in a fixed tree.
// IEEE max drops a NaN, the square-sum keeps it (every term is >= 0 or NaN, so
// no inf - inf): the final kernel reports amax = NaN exactly when sumSq is.
// fp32 roundings into one fp64 partial: packs per lane per tile x kEPP / 2 —
// at most 4 x 8 = 32 (fp8 from 4 sources); include/nbx_reduce.h states it.
struct WideLaneStats {
  f32x2 sq;
  float mx;
  __device__ __forceinline__ void reset() {
    sq = f32x2{0.0f, 0.0f};
    mx = 0.0f;
  }
  __device__ __forceinline__ void add(const f32x2& a) {
    sq[0] = __builtin_fmaf(a[0], a[0], sq[0]);
    sq[1] = __builtin_fmaf(a[1], a[1], sq[1]);
    mx = __builtin_fmaxf(mx, __builtin_fmaxf(__builtin_fabsf(a[0]), __builtin_fabsf(a[1])));   // v_max3_f32 |a0|, |a1|
  }
  __device__ __forceinline__ void add(float a) {
    sq[0] = __builtin_fmaf(a, a, sq[0]);
    mx = __builtin_fmaxf(mx, __builtin_fabsf(a));
  }
};

// End of a tile: called by all 64 lanes of the wave, converged.
__device__ __forceinline__ void wideStatsFlush(WideLaneStats& ls, WideSlot* slot) {
  double s = (double)ls.sq[0] + (double)ls.sq[1];
  float m = ls.mx;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s = s + __shfl_xor(s, o, 64);
    m = __builtin_fmaxf(m, __shfl_xor(m, o, 64));
  }
  if ((threadIdx.x & 63u) == 0) *slot = WideSlot{s, m, 0u};
  ls.reset();
}

// One element, any source count <= kMaxKSrcs (uniform guards, as reduceElt).
template <class W, bool OUT32, bool PART, bool STATS = false>
__device__ __forceinline__ void wideElt(const KArgs& a, float sc, int nSrcs, uint64_t i, WideLaneStats* ls = nullptr) {
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
  if constexpr (STATS) ls->add(acc);
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
// STATS: the final accumulators also go into *ls.
template <class W, int NSRC, int U, bool OUT32, bool PART, bool PRE, bool STATS = false>
__device__ __forceinline__ void wideFoldStore(const u32x4 (&part)[U][W::kEPP / 4], const u32x4 (&v)[NSRC][U],
                                              const float (&mul)[NSRC], u32x4* const (&dst)[kMaxKDsts], int nDsts,
                                              uint64_t p, WideLaneStats* ls = nullptr) {
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
    if constexpr (STATS) {
#pragma unroll
      for (int k = 0; k < NP; k++) ls->add(acc[k]);
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

// The helper calls of a shared body: the plain kernel's is the call it always
// made, the STATS kernel's passes the lane's statistics as the last argument.
#define NBX_WIDE_FOLD(U_, PART_, PRE_, ...)                                                       \
  do {                                                                                            \
    if constexpr (STATS) wideFoldStore<W, NSRC, U_, OUT32, PART_, PRE_, true>(__VA_ARGS__, &ls);  \
    else wideFoldStore<W, NSRC, U_, OUT32, PART_, PRE_>(__VA_ARGS__);                             \
  } while (0)
#define NBX_WIDE_ELT(...)                                                  \
  do {                                                                     \
    if constexpr (STATS) wideElt<W, OUT32, PART, true>(__VA_ARGS__, &ls);  \
    else wideElt<W, OUT32, PART>(__VA_ARGS__);                             \
  } while (0)
#define NBX_WIDE_BATCH_ELT(...)                                                 \
  do {                                                                          \
    if constexpr (STATS) wideBatchElt<W, NSRC, OUT32, true>(__VA_ARGS__, &ls);  \
    else wideBatchElt<W, NSRC, OUT32>(__VA_ARGS__);                             \
  } while (0)

// The body is text shared by the plain and the STATS kernel
// (nbx_wide_packs.inc: it reads `a`, `slots` and the constant STATS), so that
// the plain kernel keeps reading its own kernel argument, as it always did.
template <class W, int NSRC, int U, bool OUT32, bool PART>
__global__ __launch_bounds__(kBlock) void kWidePacks(KArgs a) {
  constexpr bool STATS = false;
  WideSlot* const slots = nullptr;
#include "nbx_wide_packs.inc"
}

template <class W, int NSRC, int U, bool OUT32, bool PART>
__global__ __launch_bounds__(kBlock) void kWidePacksStats(KArgs a, WideSlot* slots) {
  constexpr bool STATS = true;
#include "nbx_wide_packs.inc"
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

// Its STATS form: tiles of kWideEltsStatTile x kBlock elements whatever the
// grid is, one slot per tile and wave (kWideEltsStatTile = 8 fp32 roundings
// into a slot's fp64 partial: one square-sum chain per lane).
template <class W, bool OUT32, bool PART>
__global__ __launch_bounds__(kBlock) void kWideEltsStats(KArgs a, WideSlot* slots) {
  acquirePeerData(a);
  const float sc = loadWideArg(a.argPtr, a.arg);
  constexpr uint64_t kTile = (uint64_t)kWideEltsStatTile * kBlock;
  const uint64_t nTiles = (a.nElts + kTile - 1) / kTile;
  WideLaneStats ls;
  ls.reset();
  for (uint64_t t = blockIdx.x; t < nTiles; t += gridDim.x) {
#pragma unroll
    for (int j = 0; j < kWideEltsStatTile; j++) {
      const uint64_t i = t * kTile + (uint64_t)j * kBlock + threadIdx.x;
      if (i < a.nElts) wideElt<W, OUT32, PART, true>(a, sc, a.nSrcs, i, &ls);
    }
    wideStatsFlush(ls, slots + t * (kBlock / 64) + (threadIdx.x >> 6));
  }
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
  constexpr bool STATS = false;
  WideSlot* const slots = nullptr;
#include "nbx_wide_shifted.inc"
}

template <class W, int NSRC, bool OUT32, bool PART>
__global__ __launch_bounds__(kShiftLdsWaves * 64) void kWideShiftedLdsStats(KArgs a, WideSlot* slots) {
  constexpr bool STATS = true;
#include "nbx_wide_shifted.inc"
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
template <class W, int NSRC, bool OUT32, bool STATS = false>
__device__ __forceinline__ void wideBatchElt(const typename W::Elt* const (&src)[NSRC], void* const (&dst)[kMaxKDsts],
                                             int nDsts, uint32_t preMask, float sc, uint64_t i,
                                             WideLaneStats* ls = nullptr) {
  using E = typename W::Elt;
  float acc = W::wide(src[0][i]);
  if (preMask & 1u) acc = acc * sc;
#pragma unroll
  for (int s = 1; s < NSRC; s++) {
    float v = W::wide(src[s][i]);
    if ((preMask >> s) & 1u) v = v * sc;
    acc = acc + v;
  }
  if constexpr (STATS) ls->add(acc);
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
  constexpr bool STATS = false;
  WideSlot* const slots = nullptr;
#include "nbx_wide_batch.inc"
}

template <class W, int NSRC, bool OUT32>
__global__ __launch_bounds__(kBlock) void kWideBatchListStats(BatchListArgs a, WideSlot* slots) {
  constexpr bool STATS = true;
#include "nbx_wide_batch.inc"
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

// The STATS forms of one source type, in a WideSet of the statistics' own
// table (WideStatsTable): the same indices, every entry a k...Stats kernel.
// Every (output kind, partial-first, source count) can be a call's last pass,
// so all of them exist.
template <class W, bool OUT32, int... I, int... J>
void fillWideStats(WideSet& ws, std::integer_sequence<int, I...>, std::integer_sequence<int, J...>) {
  const void* first[] = {(const void*)&kWidePacksStats<W, I + 1, wideUnroll(I + 1), OUT32, false>...};
  const void* later[] = {nullptr, (const void*)&kWidePacksStats<W, J + 2, wideUnroll(J + 2), OUT32, true>...};
  const void* list[] = {(const void*)&kWideBatchListStats<W, I + 1, OUT32>...};
  for (int i = 0; i < kMaxKSrcs; i++) {
    ws.packs[OUT32 ? 1 : 0][0][i] = first[i];
    ws.packs[OUT32 ? 1 : 0][1][i] = later[i];
    ws.batchList[OUT32 ? 1 : 0][i] = list[i];
  }
  ws.elts[OUT32 ? 1 : 0][0] = (const void*)&kWideEltsStats<W, OUT32, false>;
  ws.elts[OUT32 ? 1 : 0][1] = (const void*)&kWideEltsStats<W, OUT32, true>;
}

template <class W, bool OUT32, int... I, int... J>
void fillWideShiftedStats(WideSet& ws, std::integer_sequence<int, I...>, std::integer_sequence<int, J...>) {
  const void* first[] = {(const void*)&kWideShiftedLdsStats<W, I + 1, OUT32, false>...};
  const void* later[] = {nullptr, (const void*)&kWideShiftedLdsStats<W, J + 2, OUT32, true>...};
  for (int i = 0; i < kMaxKSrcs; i++) {
    ws.shiftedLds[OUT32 ? 1 : 0][0][i] = first[i];
    ws.shiftedLds[OUT32 ? 1 : 0][1][i] = later[i];
  }
}

template <class Ty>
void addWideShiftedStats(WideSet& ws) {
  using W = WideTy<Ty>;
  constexpr std::make_integer_sequence<int, kMaxKSrcs> all{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs - 1> fromTwo{};
  fillWideShiftedStats<W, false>(ws, all, fromTwo);
  fillWideShiftedStats<W, true>(ws, all, fromTwo);
}

// blocksPerCU: the plain set's (the grid does not enter the statistics).
template <class Ty>
WideSet makeWideStatsSet(int blocksPerCU) {
  using W = WideTy<Ty>;
  WideSet ws{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs> all{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs - 1> fromTwo{};
  fillWideStats<W, false>(ws, all, fromTwo);
  fillWideStats<W, true>(ws, all, fromTwo);
  ws.eltBytes = (int)sizeof(typename W::Elt);
  ws.blocksPerCU = blocksPerCU;
  ws.valid = 1;
  return ws;
}

}  // namespace nbx
