// nbx_mx.h — MXFP8 block-scaled form of the fp32-accumulating sums
// (nbxReduceMultiWideMx, include/nbx_reduce.h).
//
// The fold is nbx_wide.h's: every source widened exactly, one unfused fp32
// multiply or add per step in source order. New is what a source is — fp8
// codes with one E8M0 scale byte per 32-element block, each element one more
// fp32 multiply by 2^(e-127) — and what is stored: per block the maximum of
// the final accumulators picks a power-of-two scale, the accumulators are
// multiplied by its inverse, narrowed with the type's own narrowing
// (WideTy::narrowWord: RNE behind satFinite) and stored with the scale byte.
//
// Two kernels per (source kind, output, partial-first):
//   * kMxBlocks<W, SCALED, O, NSRC, U, PART>: every element pointer 16-byte
//     aligned, every destination scale pointer 4-byte aligned. A lane holds
//     one 16-element group — one dwordx4 of destination codes, fed by one
//     source pack (fp8) or two adjacent ones (16-bit) — and a block is the
//     lane pair (2k, 2k+1). All loads of a tile are issued source-major ahead
//     of the fold (wideLoadTile's order, the scale bytes first). Each lane
//     takes the integer maximum of its 16 accumulators' magnitude bits — as
//     unsigned integers NaN > inf > every finite value, the statistics' amax
//     rule — one DPP quad_perm exchange gives the pair the block's maximum,
//     and both lanes derive the scale byte and its inverse from the exponent
//     field. In a full tile the 32 scale bytes of a wave's step are gathered
//     over three DPP row shifts into one dword per 8 lanes; the blocks of the
//     last, partial tile store theirs as bytes (a dword could reach past the
//     array). The elements of a partial last block are done by one half wave
//     of the last workgroup, one element per lane (mxEltLane). No LDS and no
//     barrier (static tile schedule), nothing is read twice.
//   * kMxGeneric<W, SCALED, O, PART>: any alignment. Half a wave per block,
//     one element per lane with element-sized loads and stores, the block's
//     maximum over a 5-step xor butterfly. The same operations on the same
//     values in the same order as the block kernel: the same bits.
// PART: source 0 is the fp32 partial of earlier passes, as in nbx_wide.h.
#pragma once
#include "nbx_wide.h"

namespace nbx {

// Output kinds: the fp8 type and its emax (OCP MX v1.0: the exponent of the
// largest power of two the element type represents), or fp32 (no scaling).
struct MxOutE4M3 {
  using W = WideTy<TyE4M3>;
  static constexpr bool kF32 = false;
  static constexpr int kEmax = 8, kIndex = 0;
};
struct MxOutE5M2 {
  using W = WideTy<TyE5M2>;
  static constexpr bool kF32 = false;
  static constexpr int kEmax = 15, kIndex = 1;
};
struct MxOutF32 {
  using W = WideTy<TyE4M3>;   // unused
  static constexpr bool kF32 = true;
  static constexpr int kEmax = 0, kIndex = 2;
};

// A source block's scale 2^(e-127) as fp32: e << 23 is the value for e in
// [1, 254]; e = 0 is the denormal 2^-127 and e = 0xFF (MX's NaN block) a NaN.
__device__ __forceinline__ float mxScaleIn(uint32_t e) {
  return __uint_as_float((e << 23) | (((e + 1u) & 0xffu) <= 1u ? 0x400000u : 0u));
}

// Magnitude bits of an accumulator: ordered as unsigned integers like the
// statistics' amax (NaN above inf above every finite value).
__device__ __forceinline__ uint32_t mxMag(float a) { return __float_as_uint(a) & 0x7fffffffu; }

// The block's scale byte S and the fp32 factor R = 2^(127-S) from the
// magnitude bits of its maximum: S = max(be - emax, 0) for a finite maximum
// with biased exponent be, so the factor's exponent field 254 - S is always a
// normal number's. A non-finite maximum: S = 0xFF and the elements unscaled.
template <int EMAX>
__device__ __forceinline__ void mxScaleOut(uint32_t mb, uint32_t& S, float& R) {
  const bool fin = mb < 0x7f800000u;
  const int be = (int)(mb >> 23) - EMAX;
  S = fin ? (uint32_t)(be > 0 ? be : 0) : 0xffu;
  R = fin ? __uint_as_float((254u - S) << 23) : 1.0f;
}

// The value of lane ^ 1 (quad_perm [1, 0, 3, 2]) and of lane + N in the row of 16.
__device__ __forceinline__ uint32_t mxPairSwap(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);
}
template <int N>
__device__ __forceinline__ uint32_t mxRowShl(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + N, 0xf, 0xf, false);
}

// The fold of element idx (of source block b): every source widened, scaled
// and pre-multiplied, one fp32 add per further source in source order.
template <class W, bool SCALED, bool PART>
__device__ __forceinline__ float mxFoldElt(const KArgs& a, const uint8_t* const (&ss)[kMaxKSrcs], float sc, int nSrcs,
                                           uint64_t idx, uint64_t b) {
  using E = typename W::Elt;
  float acc = 0.0f;
#pragma unroll
  for (int s = 0; s < kMaxKSrcs; s++) {
    if (s < nSrcs) {
      float v;
      if (PART && s == 0) {
        v = ((const float*)a.src[0])[idx];
      } else {
        v = W::wide(((const E*)a.src[s])[idx]);
        if constexpr (SCALED) v = v * mxScaleIn(ss[s][b]);
        if ((a.preMask >> s) & 1u) v = v * sc;
      }
      acc = s == 0 ? v : acc + v;
    }
  }
  return acc;
}

// One element of block b per lane: i < len lanes hold element 32 b + i, the
// others nothing (len = 0: an idle half wave). Called by whole waves,
// converged; the two halves of a wave may hold different blocks.
template <class W, bool SCALED, class O, bool PART>
__device__ __forceinline__ void mxEltLane(const KArgs& a, const MxArgs& x, float sc, int nSrcs, uint64_t b, int i,
                                          int len) {
  const bool on = i < len;
  const uint64_t idx = b * kMxBlockElts + (uint64_t)i;
  const float acc = on ? mxFoldElt<W, SCALED, PART>(a, x.srcScale, sc, nSrcs, idx, b) : 0.0f;
  if constexpr (O::kF32) {
    if (on) {
#pragma unroll
      for (int d = 0; d < kMaxKDsts; d++)
        if (d < a.nDsts) ((float*)a.dst[d])[idx] = acc;
    }
  } else {
    uint32_t mb = mxMag(acc);
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)mb, o, 64);
      mb = mb > other ? mb : other;
    }
    uint32_t S;
    float R;
    mxScaleOut<O::kEmax>(mb, S, R);
    if (on) {
      const uint8_t code = O::W::narrow(acc * R);
#pragma unroll
      for (int d = 0; d < kMaxKDsts; d++) {
        if (d < a.nDsts) {
          ((uint8_t*)a.dst[d])[idx] = code;
          if (i == 0) x.dstScale[d][b] = (uint8_t)S;
        }
      }
    }
  }
}

// Source-major issue order, as wideLoadTile: the scale bytes (one per source
// and group; both lanes of a pair read their block's byte with the one wave
// instruction), the fp32 partial, then every source's packs.
template <class W, bool SCALED, int NSRC, int U, bool PART>
__device__ __forceinline__ void mxLoadTile(u32x4 (&part)[U][4], u32x4 (&v)[NSRC][U][16 / W::kEPP],
                                           uint32_t (&e)[NSRC][U], const u32x4* const (&src)[NSRC],
                                           const uint8_t* const (&ss)[NSRC], uint64_t g) {
  constexpr int NPK = 16 / W::kEPP;
  if constexpr (SCALED) {
#pragma unroll
    for (int s = PART ? 1 : 0; s < NSRC; s++)
#pragma unroll
      for (int u = 0; u < U; u++) e[s][u] = ss[s][(g + (uint64_t)u * kBlock) >> 1];
  }
  if constexpr (PART) {
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int j = 0; j < 4; j++) part[u][j] = ldPack(src[0] + (g + (uint64_t)u * kBlock) * 4 + j);
  }
#pragma unroll
  for (int s = PART ? 1 : 0; s < NSRC; s++)
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int k = 0; k < NPK; k++) v[s][u][k] = ldPack(src[s] + (g + (uint64_t)u * kBlock) * NPK + k);
}

// The fold of group u of a tile already in registers: 16 fp32 accumulators as
// 8 pairs, every step one unfused multiply or add in source order.
template <class W, bool SCALED, int NSRC, int U, bool PART, bool PRE>
__device__ __forceinline__ void mxFoldAcc(const u32x4 (&part)[U][4], const u32x4 (&v)[NSRC][U][16 / W::kEPP],
                                          const uint32_t (&e)[NSRC][U], const float (&mul)[NSRC], int u,
                                          f32x2 (&acc)[8]) {
  constexpr int NPK = 16 / W::kEPP, NP = W::kEPP / 2;
#pragma unroll
  for (int s = 0; s < NSRC; s++) {
    f32x2 t[8];
    if (PART && s == 0) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        t[2 * j] = f32x2{__uint_as_float(part[u][j].x), __uint_as_float(part[u][j].y)};
        t[2 * j + 1] = f32x2{__uint_as_float(part[u][j].z), __uint_as_float(part[u][j].w)};
      }
    } else {
#pragma unroll
      for (int k = 0; k < NPK; k++)
#pragma unroll
        for (int w = 0; w < 4; w++) W::wideWord(v[s][u][k][w], &t[k * NP + w * W::kWP]);
      if constexpr (SCALED) {
        const float xs = mxScaleIn(e[s][u]);
        const f32x2 m = {xs, xs};
#pragma unroll
        for (int k = 0; k < 8; k++) t[k] = t[k] * m;
      }
      if constexpr (PRE) {
        const f32x2 m = {mul[s], mul[s]};
#pragma unroll
        for (int k = 0; k < 8; k++) t[k] = t[k] * m;
      }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = s == 0 ? t[k] : acc[k] + t[k];
  }
}

// Fold U groups already in registers, scale and store them. mul: as
// wideFoldStore's (the scalar or 1.0 per source, PRE only). GATHER: all 64
// lanes of the wave are here with full blocks, and each step's 32 scale bytes
// leave as 8 dword stores; else the even lane of a pair stores its byte.
template <class W, bool SCALED, class O, int NSRC, int U, bool PART, bool PRE, bool GATHER>
__device__ __forceinline__ void mxFoldStore(const u32x4 (&part)[U][4], const u32x4 (&v)[NSRC][U][16 / W::kEPP],
                                            const uint32_t (&e)[NSRC][U], const float (&mul)[NSRC],
                                            u32x4* const (&dst)[kMaxKDsts], uint8_t* const (&ds)[kMaxKDsts],
                                            int nDsts, uint64_t g) {
#pragma unroll
  for (int u = 0; u < U; u++) {
    f32x2 acc[8];
    mxFoldAcc<W, SCALED, NSRC, U, PART, PRE>(part, v, e, mul, u, acc);
    const uint64_t q = g + (uint64_t)u * kBlock;
    if constexpr (O::kF32) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const u32x4 o = {__float_as_uint(acc[2 * j][0]), __float_as_uint(acc[2 * j][1]),
                         __float_as_uint(acc[2 * j + 1][0]), __float_as_uint(acc[2 * j + 1][1])};
        stPack(dst[0] + q * 4 + j, o);
#pragma unroll
        for (int d = 1; d < kMaxKDsts; d++)
          if (d < nDsts) stPack(dst[d] + q * 4 + j, o);
      }
    } else {
      uint32_t mb = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t m0 = mxMag(acc[k][0]), m1 = mxMag(acc[k][1]);
        const uint32_t m01 = m0 > m1 ? m0 : m1;
        mb = mb > m01 ? mb : m01;   // v_max3_u32
      }
      const uint32_t other = mxPairSwap(mb);
      mb = mb > other ? mb : other;
      uint32_t S;
      float R;
      mxScaleOut<O::kEmax>(mb, S, R);
      const f32x2 r = {R, R};
#pragma unroll
      for (int k = 0; k < 8; k++) acc[k] = acc[k] * r;
      u32x4 o;
#pragma unroll
      for (int w = 0; w < 4; w++) o[w] = O::W::narrowWord(&acc[w * 2]);
      stPack(dst[0] + q, o);
#pragma unroll
      for (int d = 1; d < kMaxKDsts; d++)
        if (d < nDsts) stPack(dst[d] + q, o);
      // group q is half of block q / 2: lanes 8 j .. 8 j + 7 hold blocks
      // q / 2 .. q / 2 + 3 of lane 8 j, whose byte address is 4-byte aligned
      if constexpr (GATHER) {
        const uint32_t word = S | (mxRowShl<2>(S) << 8) | (mxRowShl<4>(S) << 16) | (mxRowShl<6>(S) << 24);
        if ((threadIdx.x & 7u) == 0) {
          *(uint32_t*)(ds[0] + (q >> 1)) = word;
#pragma unroll
          for (int d = 1; d < kMaxKDsts; d++)
            if (d < nDsts) *(uint32_t*)(ds[d] + (q >> 1)) = word;
        }
      } else {
        if ((threadIdx.x & 1u) == 0) {
          ds[0][q >> 1] = (uint8_t)S;
#pragma unroll
          for (int d = 1; d < kMaxKDsts; d++)
            if (d < nDsts) ds[d][q >> 1] = (uint8_t)S;
        }
      }
    }
  }
}

// a.nPacks: the 16-element groups of the call's full blocks (an even number).
template <class W, bool SCALED, class O, int NSRC, int U, bool PART>
__global__ __launch_bounds__(kBlock) void kMxBlocks(KArgs a, MxArgs x) {
  constexpr int NPK = 16 / W::kEPP;
  static_assert(!PART || NSRC >= 2, "a pass that reads a partial folds at least one more source");
  const float sc = loadWideArg(a.argPtr, a.arg);
  const u32x4* src[NSRC];
  const uint8_t* ss[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) {
    src[s] = (const u32x4*)a.src[s];
    ss[s] = x.srcScale[s];
  }
  u32x4* dst[kMaxKDsts];
  uint8_t* ds[kMaxKDsts];
#pragma unroll
  for (int d = 0; d < kMaxKDsts; d++) {
    dst[d] = (u32x4*)a.dst[d];
    ds[d] = x.dstScale[d];
  }
  const int nDsts = a.nDsts;
  const bool pre = a.preMask != 0;   // uniform: the fold is chosen per tile
  float mul[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) mul[s] = ((a.preMask >> s) & 1u) ? sc : 1.0f;
  const uint64_t n = a.nPacks;
  constexpr uint64_t kTile = (uint64_t)U * kBlock;
  forEachTile(a, (n + kTile - 1) / kTile, [&](uint64_t t) {
    const uint64_t g = t * kTile + threadIdx.x;
    if ((t + 1) * kTile <= n) {
      // full tile (uniform): issue every load first, then fold
      u32x4 part[U][4];
      u32x4 v[NSRC][U][NPK];
      uint32_t e[NSRC][U];
      mxLoadTile<W, SCALED, NSRC, U, PART>(part, v, e, src, ss, g);
      __builtin_amdgcn_sched_barrier(0);
      if (pre) mxFoldStore<W, SCALED, O, NSRC, U, PART, true, true>(part, v, e, mul, dst, ds, nDsts, g);
      else mxFoldStore<W, SCALED, O, NSRC, U, PART, false, true>(part, v, e, mul, dst, ds, nDsts, g);
    } else {
      // last, partial tile: n is even, so a pair is in or out together
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t q = g + (uint64_t)u * kBlock;
        if (q < n) {
          u32x4 part1[1][4];
          u32x4 v1[NSRC][1][NPK];
          uint32_t e1[NSRC][1];
          mxLoadTile<W, SCALED, NSRC, 1, PART>(part1, v1, e1, src, ss, q);
          mxFoldStore<W, SCALED, O, NSRC, 1, PART, true, false>(part1, v1, e1, mul, dst, ds, nDsts, q);
        }
      }
    }
  });

  // the partial last block (count % 32 elements): wave 0 of the last workgroup
  const int rest = (int)(a.nElts & (uint64_t)(kMxBlockElts - 1));
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < 64 && rest != 0) {
    const int lane = (int)threadIdx.x;
    mxEltLane<W, SCALED, O, PART>(a, x, sc, NSRC, n >> 1, lane & 31, lane < 32 ? rest : 0);
  }
}

// Any alignment: half a wave per block, one element per lane. The trip count
// is the wave's (both halves loop together), so every shuffle is converged.
template <class W, bool SCALED, class O, bool PART>
__global__ __launch_bounds__(kBlock) void kMxGeneric(KArgs a, MxArgs x) {
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint64_t nBlocks = (a.nElts + kMxBlockElts - 1) / kMxBlockElts;
  constexpr uint64_t kPerWG = kBlock / kMxBlockElts;
  const int i = (int)(threadIdx.x & 31u);
  const uint64_t half = (threadIdx.x >> 5) & 1u;
  for (uint64_t wb = (uint64_t)blockIdx.x * kPerWG + ((threadIdx.x >> 6) << 1); wb < nBlocks;
       wb += (uint64_t)gridDim.x * kPerWG) {
    const uint64_t b = wb + half;
    int len = 0;
    if (b < nBlocks) {
      const uint64_t left = a.nElts - b * kMxBlockElts;
      len = left < (uint64_t)kMxBlockElts ? (int)left : kMxBlockElts;
    }
    mxEltLane<W, SCALED, O, PART>(a, x, sc, a.nSrcs, b, i, len);
  }
}

// ---------------------------------------------------------------------------
// Launch table of one source kind (MxSet, nbx_kargs.h).

template <class W, bool SCALED, class O, int... I, int... J>
void fillMxOut(MxSet& ms, std::integer_sequence<int, I...>, std::integer_sequence<int, J...>) {
  constexpr int EB = (int)sizeof(typename W::Elt);
  const void* first[] = {(const void*)&kMxBlocks<W, SCALED, O, I + 1, mxUnroll(I + 1, EB), false>...};
  const void* later[] = {nullptr, (const void*)&kMxBlocks<W, SCALED, O, J + 2, mxUnroll(J + 2, EB), true>...};
  setMxOut(ms, O::kIndex, first, later, (const void*)&kMxGeneric<W, SCALED, O, false>,
           (const void*)&kMxGeneric<W, SCALED, O, true>);
}

// Plain sources store MX only (their fp32 sum is nbxReduceMultiWide's);
// scaled sources also store fp32.
template <class Ty, bool SCALED>
MxSet makeMxSet() {
  using W = WideTy<Ty>;
  MxSet ms{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs> all{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs - 1> fromTwo{};
  fillMxOut<W, SCALED, MxOutE4M3>(ms, all, fromTwo);
  fillMxOut<W, SCALED, MxOutE5M2>(ms, all, fromTwo);
  if constexpr (SCALED) fillMxOut<W, SCALED, MxOutF32>(ms, all, fromTwo);
  ms.scaled = SCALED ? 1 : 0;
  ms.valid = 1;
  return ms;
}

}  // namespace nbx
