// nbx_mx6.h — MXFP6 (E2M3, E3M2) elements in the block-scaled fp32-accumulating
// sum (nbxReduceMultiWideMx with NBX_FLOAT6_E2M3 / NBX_FLOAT6_E3M2,
// include/nbx_reduce.h).
//
// The fold, the block maximum and the scale rule are nbx_mx.h's (mxScaleIn,
// mxMag, mxScaleOut with emax = 2 / 4). New is the element: a 6-bit code in a
// dense little-endian bit stream (element i in bits [6 i, 6 i + 6)), so a block
// of 32 is 24 bytes, four elements are three bytes and codes straddle bytes.
// Neither type has a NaN or inf code: a non-finite block stores the scale byte
// 0xFF over all-zero codes, and a 0xFF source block reads as NaN through its
// scale. gfx950's FP6 converters work on a whole block held by ONE lane
// (v_cvt_scalef32_2xpk16_{fp6,bf6}_f32: 32 fp32 -> 6 dwords,
// v_cvt_scalef32_pk32_f32_{fp6,bf6}: back), so the block kernel ends — and for
// MXFP6 sources also begins — with a block per lane.
//
// Source kinds: plain f16 / bf16 (Mx4Src16, MXFP6 output only) and MXFP6
// (Mx6SrcFp6<F>, the same type or fp32 out). Two kernels per (kind, output, PART):
//   * kMx6Blocks<S, O, NSRC, U, PART>: every element pointer 16-byte aligned,
//     every destination scale pointer 4-byte aligned. A lane ends up owning U
//     blocks per tile, so a tile is U x 256 blocks.
//     16-bit sources fold in the MXFP4 quad layout: a wave takes 64 consecutive
//     blocks in four sub-steps, in each a lane holds one 8-element group (one
//     dwordx4 per source at unit stride, 1 KiB contiguous per wave instruction;
//     the fp32 partial two dwordx4), the block is the lane quad and its maximum
//     crosses two DPP quad_perm exchanges. Every lane scales its accumulators
//     by the block's R. Then the four sub-steps are transposed 4 x 4 inside the
//     quad (two DPP quad_perm stages of select / move / select, once per
//     output, not per source): lane j of quad w holds all of block 16 j + w of
//     the wave's 64.
//     MXFP6 sources are loaded a block per lane from the start: three dwordx2
//     (24 bytes at a 24-byte lane stride, so a wave instruction triple reads
//     1536 contiguous bytes and no line is touched twice), one scale byte per
//     lane, decoded by the pk32 converter, the fold and the maximum all inside
//     the lane: no exchange at all. The fp32 partial and an fp32 output are
//     eight dwordx4 per lane.
//     Either way a lane then narrows its block with ONE 2xpk16 instruction and
//     stores 24 bytes as three dwordx2; the wave's stores cover one contiguous
//     1536-byte run. In a full tile four blocks' scale bytes are gathered over
//     DPP row_shl into one dword (mx4FoldStore's GATHER); the last, partial tile
//     predicates loads and stores per block and stores scale bytes as bytes.
//     Static tile schedule, no LDS, no barrier, nothing read twice; in place a
//     lane overwrites exactly the 24 bytes it read. The count % 32 tail is
//     mx6QuadLane's, run by eight lanes of wave 0 of the last workgroup.
//   * kMx6Generic<S, O, PART>: any alignment. A lane holds four elements — three
//     destination bytes, so two lanes never share a byte — a block is 8 lanes,
//     its maximum a 3-step xor butterfly, loads and stores byte and element
//     sized. A final group of r = count % 4 elements stores ceil(6 r / 8) bytes
//     with zeroed spare bits. The block kernel's operations on the same values
//     in the same order.
//
// Converters (scripts/probe_fp6_cvt.hip, profiles/r17/probe_fp6_cvt_mi355x.txt):
// at scale 1.0 both decoders give the contract's table for all 64 codes in all
// 32 places (element i of the v32f32 is field i of the stream), and both
// narrowing converters equal RNE in integer arithmetic on 4.7 M inputs —
// subnormal grid, ties, signed zeros, fp32 denormals, everything above the
// largest (inf too) stored as the largest. Operand a[i] of the 2xpk16 form lands
// in field 2 i and b[i] in field 2 i + 1: the operands are the even and the odd
// elements. So nothing was forced into software; the block kernel uses all four
// instructions. The generic kernel and the tail hold 4 elements per lane, which
// is no converter's shape, and run mx6Decode / mx6Narrow in integer arithmetic:
// the tests hold both to the same bits. The source scale does NOT go through
// the decoder's scale operand (nbx_mx4.h: its NaN for e = 0xFF has other bits).
#pragma once
#include "nbx_mx4.h"

namespace nbx {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

// Element formats: kMB mantissa bits, exponent bias, the MX emax.
struct Mx6E2M3 {
  static constexpr int kMB = 3, kBias = 1, kEmax = 2;
  static constexpr bool kF32 = false;
  __device__ static u32x6 narrow32(f32x16 even, f32x16 odd) {
    return __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(even, odd, 1.0f);
  }
  __device__ static f32x32 wide32(u32x6 w) { return __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(w, 1.0f); }
};
struct Mx6E3M2 {
  static constexpr int kMB = 2, kBias = 3, kEmax = 4;
  static constexpr bool kF32 = false;
  __device__ static u32x6 narrow32(f32x16 even, f32x16 odd) {
    return __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(even, odd, 1.0f);
  }
  __device__ static f32x32 wide32(u32x6 w) { return __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(w, 1.0f); }
};
struct Mx6OutF32 {
  static constexpr int kEmax = 0;
  static constexpr bool kF32 = true;
};

// One code in integer arithmetic (generic kernel and tail). Exponent field 0 is
// m steps of 2^(1 - bias - MB); else the fields move into fp32's.
template <class F>
__device__ __forceinline__ float mx6Decode(uint32_t c) {
  const uint32_t mag = c & 31u, m = mag & ((1u << F::kMB) - 1u);
  const float sub = (float)m * __uint_as_float((uint32_t)(128 - F::kBias - F::kMB) << 23);
  const uint32_t nrm = (mag << (23 - F::kMB)) + ((uint32_t)(127 - F::kBias) << 23);
  return __uint_as_float(((mag >> F::kMB) ? nrm : __float_as_uint(sub)) | ((c & 32u) << 26));
}

// narrow6: RNE onto the type's grid, everything above the largest stored as
// the largest (0x1F), the sign kept. Below the smallest normal the grid is
// uniform: adding 2^23 steps makes the step fp32's ulp, so the ADD rounds
// (an fp32 denormal, kept or flushed, adds nothing). Above, the usual
// round-half-even on the bits.
template <class F>
__device__ __forceinline__ uint32_t mx6Narrow(float v) {
  constexpr int SH = 23 - F::kMB;
  constexpr uint32_t kMinNormal = (uint32_t)(128 - F::kBias) << 23;
  constexpr uint32_t kMagic = (uint32_t)(151 - F::kBias - F::kMB) << 23;
  const uint32_t b = __float_as_uint(v), u = b & 0x7fffffffu;
  const uint32_t sub = __float_as_uint(__uint_as_float(u) + __uint_as_float(kMagic)) - kMagic;
  const uint32_t r = u + ((1u << (SH - 1)) - 1u) + ((u >> SH) & 1u);
  const uint32_t nrm = (r >> SH) - ((uint32_t)(127 - F::kBias) << F::kMB);
  return (u < kMinNormal ? sub : (nrm < 31u ? nrm : 31u)) | ((b >> 26) & 32u);
}

template <class F>
struct Mx6SrcFp6;
template <class S>
struct Mx6IsFp6 { static constexpr bool value = false; };
template <class F>
struct Mx6IsFp6<Mx6SrcFp6<F>> { static constexpr bool value = true; };
template <class S>
constexpr bool mx6IsFp6() { return Mx6IsFp6<S>::value; }

template <class F>
struct Mx6SrcFp6 {
  using Fmt = F;
  // elements 4 j .. 4 j + 3 of the bucket, the first k of them: ceil(6 k / 8) bytes
  __device__ static void wide4(const void* p, uint64_t j, int k, float (&t)[4]) {
    const uint8_t* e = (const uint8_t*)p + 3 * j;
    uint32_t w = e[0];
    if (k >= 2) w |= (uint32_t)e[1] << 8;
    if (k >= 3) w |= (uint32_t)e[2] << 16;
#pragma unroll
    for (int i = 0; i < 4; i++) t[i] = i < k ? mx6Decode<F>(w >> (6 * i)) : 0.0f;   // a last byte's spare bits are ignored
  }
};

// the plain 16-bit kinds are nbx_mx4.h's (a dwordx4 is 8 elements); the generic lane function's 4
template <class S>
__device__ __forceinline__ void mx6Wide4(const void* p, uint64_t j, int k, float (&t)[4]) {
  if constexpr (mx6IsFp6<S>()) {
    S::wide4(p, j, k, t);
  } else {
    const uint16_t* e = (const uint16_t*)p + 4 * j;
#pragma unroll
    for (int i = 0; i < 4; i++) t[i] = i < k ? S::W::wide(e[i]) : 0.0f;
  }
}

// ---------------------------------------------------------------------------
// Four elements of block b per lane: lane i of 8 holds elements 32 b + 4 i ..
// + 3, those below len (len = 0: idle lanes). Called by whole waves, converged;
// the eight octets of a wave may hold different blocks.
template <class S, class O, bool PART>
__device__ __forceinline__ void mx6QuadLane(const KArgs& a, const MxArgs& x, float sc, int nSrcs, uint64_t b, int i,
                                            int len) {
  constexpr bool FP6 = mx6IsFp6<S>();
  const int k = len - 4 * i < 0 ? 0 : (len - 4 * i > 4 ? 4 : len - 4 * i);   // this lane's elements
  const uint64_t j = b * (kMxBlockElts / 4) + (uint64_t)i;                  // the 4-element group
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // an element that is not there takes no part in the maximum
  if (k > 0) {
#pragma unroll
    for (int s = 0; s < kMaxKSrcs; s++) {
      if (s < nSrcs) {
        float v[4];
        if (PART && s == 0) {
          const float* p = (const float*)a.src[0] + 4 * j;
#pragma unroll
          for (int e = 0; e < 4; e++) v[e] = e < k ? p[e] : 0.0f;
        } else {
          mx6Wide4<S>(a.src[s], j, k, v);
          if constexpr (FP6) {
            const float xs = mxScaleIn(x.srcScale[s][b]);
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = v[e] * xs;
          }
          if ((a.preMask >> s) & 1u) {
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = v[e] * sc;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) acc[e] = s == 0 ? v[e] : acc[e] + v[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (e >= k) acc[e] = 0.0f;
  }
  if constexpr (O::kF32) {
#pragma unroll
    for (int d = 0; d < kMaxKDsts; d++) {
      if (d < a.nDsts) {
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (e < k) ((float*)a.dst[d])[4 * j + e] = acc[e];
      }
    }
  } else {
    uint32_t mb = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const uint32_t m = mxMag(acc[e]);
      mb = mb > m ? mb : m;
    }
#pragma unroll
    for (int o = 4; o >= 1; o >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)mb, o, 64);
      mb = mb > other ? mb : other;
    }
    uint32_t Sb;
    float R;
    mxScaleOut<O::kEmax>(mb, Sb, R);
    if (k > 0) {
      uint32_t w = 0;
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (e < k) w |= mx6Narrow<O>(acc[e] * R) << (6 * e);   // spare bits of a last byte stay 0
      if (Sb == 0xffu) w = 0;                                  // no NaN code: the scale byte says it
#pragma unroll
      for (int d = 0; d < kMaxKDsts; d++) {
        if (d < a.nDsts) {
          uint8_t* p = (uint8_t*)a.dst[d] + 3 * j;
          p[0] = (uint8_t)w;
          if (k >= 2) p[1] = (uint8_t)(w >> 8);
          if (k >= 3) p[2] = (uint8_t)(w >> 16);
          if (i == 0) x.dstScale[d][b] = (uint8_t)Sb;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// The block kernel's back end: a lane holds one block as its even and odd
// elements, already scaled. One converter instruction, three dwordx2 stores,
// the scale byte. GATHER: the whole wave is here with full blocks; SHL lanes
// apart hold consecutive blocks, and the first of four stores their dword.
template <class O, int SHL, bool GATHER>
__device__ __forceinline__ void mx6StoreBlock(f32x16 even, f32x16 odd, uint32_t Sb, bool first, bool on, uint64_t blk,
                                              void* const (&dst)[kMaxKDsts], uint8_t* const (&ds)[kMaxKDsts],
                                              int nDsts) {
  u32x6 o = O::narrow32(even, odd);
  if (Sb == 0xffu) o = u32x6{0u, 0u, 0u, 0u, 0u, 0u};   // no NaN code: the scale byte says it
  if (GATHER || on) {
#pragma unroll
    for (int d = 0; d < kMaxKDsts; d++) {
      if (d == 0 || d < nDsts) {
        u32x2* p = (u32x2*)dst[d] + blk * 3;
        p[0] = u32x2{o[0], o[1]};
        p[1] = u32x2{o[2], o[3]};
        p[2] = u32x2{o[4], o[5]};
      }
    }
  }
  if constexpr (GATHER) {
    const uint32_t word =
        Sb | (mxRowShl<SHL>(Sb) << 8) | (mxRowShl<2 * SHL>(Sb) << 16) | (mxRowShl<3 * SHL>(Sb) << 24);
    if (first) {
#pragma unroll
      for (int d = 0; d < kMaxKDsts; d++)
        if (d == 0 || d < nDsts) *(uint32_t*)(ds[d] + blk) = word;
    }
  } else if (on) {
#pragma unroll
    for (int d = 0; d < kMaxKDsts; d++)
      if (d == 0 || d < nDsts) ds[d][blk] = (uint8_t)Sb;
  }
}

// One stage of the 4 x 4 transpose inside a quad: lanes whose bit is clear keep
// lo and hand hi to the partner, the others the reverse. XOR2: the partner is
// lane ^ 2 (quad_perm [2,3,0,1]), else lane ^ 1 ([1,0,3,2]).
template <bool XOR2>
__device__ __forceinline__ void mx6Swap(float& lo, float& hi, bool bit) {
  const uint32_t send = __float_as_uint(bit ? lo : hi);
  const float recv = __uint_as_float(XOR2 ? mx4QuadSwap2(send) : mxPairSwap(send));
  lo = bit ? recv : lo;
  hi = bit ? hi : recv;
}

// ---- 16-bit sources: the quad layout --------------------------------------
// Group index of sub-step k for this lane: c0 is the wave's first group (a
// multiple of 256). Source-major issue order: the fp32 partial, the elements.
template <class S, int NSRC, int U, bool PART, bool GUARD>
__device__ __forceinline__ void mx6Load16(u32x4 (&part)[U][4][2], u32x4 (&v)[NSRC][U][4], const void* const (&src)[NSRC],
                                          uint64_t c0, uint64_t nGroups) {
  const u32x4 zero = {0u, 0u, 0u, 0u};
  const uint32_t lane = threadIdx.x & 63u;
  if constexpr (PART) {
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int k = 0; k < 4; k++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const uint64_t q = c0 + (uint64_t)u * (4 * kBlock) + (uint64_t)(k * 64) + lane;
          part[u][k][h] = (!GUARD || q < nGroups) ? ldPack((const u32x4*)src[0] + q * 2 + h) : zero;
        }
  }
#pragma unroll
  for (int s = PART ? 1 : 0; s < NSRC; s++)
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint64_t q = c0 + (uint64_t)u * (4 * kBlock) + (uint64_t)(k * 64) + lane;
        v[s][u][k] = (!GUARD || q < nGroups) ? S::load(src[s], q) : zero;
      }
}

template <class S, class O, int NSRC, int U, bool PART, bool PRE, bool GUARD>
__device__ __forceinline__ void mx6FoldStore16(const u32x4 (&part)[U][4][2], const u32x4 (&v)[NSRC][U][4],
                                               const float (&mul)[NSRC], void* const (&dst)[kMaxKDsts],
                                               uint8_t* const (&ds)[kMaxKDsts], int nDsts, uint64_t c0,
                                               uint64_t nBlocks) {
  const uint32_t lane = threadIdx.x & 63u, j = lane & 3u;
#pragma unroll
  for (int u = 0; u < U; u++) {
    float y[4][8];      // [sub-step][element of the group], scaled
    uint32_t sb[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      f32x2 acc[4];
#pragma unroll
      for (int s = 0; s < NSRC; s++) {
        f32x2 t[4];
        if (PART && s == 0) {
#pragma unroll
          for (int h = 0; h < 2; h++) {
            t[2 * h] = f32x2{__uint_as_float(part[u][k][h].x), __uint_as_float(part[u][k][h].y)};
            t[2 * h + 1] = f32x2{__uint_as_float(part[u][k][h].z), __uint_as_float(part[u][k][h].w)};
          }
        } else {
          S::wide8(v[s][u][k], t);
          if constexpr (PRE) {
            const f32x2 m = {mul[s], mul[s]};
#pragma unroll
            for (int e = 0; e < 4; e++) t[e] = t[e] * m;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) acc[e] = s == 0 ? t[e] : acc[e] + t[e];
      }
      uint32_t mb = 0;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const uint32_t m0 = mxMag(acc[e][0]), m1 = mxMag(acc[e][1]);
        const uint32_t m01 = m0 > m1 ? m0 : m1;
        mb = mb > m01 ? mb : m01;   // v_max3_u32
      }
      uint32_t other = mxPairSwap(mb);
      mb = mb > other ? mb : other;
      other = mx4QuadSwap2(mb);
      mb = mb > other ? mb : other;
      float R;
      mxScaleOut<O::kEmax>(mb, sb[k], R);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        y[k][2 * e] = acc[e][0] * R;
        y[k][2 * e + 1] = acc[e][1] * R;
      }
    }
    // y[k][e] of lane m -> y[m][e] of lane k: lane j ends with quarter m of the
    // block of sub-step j in y[m][.]
#pragma unroll
    for (int e = 0; e < 8; e++) {
      mx6Swap<false>(y[0][e], y[1][e], (j & 1u) != 0);
      mx6Swap<false>(y[2][e], y[3][e], (j & 1u) != 0);
      mx6Swap<true>(y[0][e], y[2][e], (j & 2u) != 0);
      mx6Swap<true>(y[1][e], y[3][e], (j & 2u) != 0);
    }
    const uint32_t Sb = j == 0 ? sb[0] : j == 1 ? sb[1] : j == 2 ? sb[2] : sb[3];
    f32x16 even, odd;
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int e = 0; e < 4; e++) {
        even[4 * m + e] = y[m][2 * e];
        odd[4 * m + e] = y[m][2 * e + 1];
      }
    // the wave's 64 blocks start at group c0 / 4; sub-step j holds blocks 16 j .. 16 j + 15, quad w the w-th
    const uint64_t blk = ((c0 + (uint64_t)u * (4 * kBlock)) >> 2) + (uint64_t)(j * 16u + (lane >> 2));
    mx6StoreBlock<O, 4, !GUARD>(even, odd, Sb, (lane & 12u) == 0, blk < nBlocks, blk, dst, ds, nDsts);
  }
}

// ---- MXFP6 sources: a block per lane from the start -----------------------
// b0: the lane's block of step 0; step u is kBlock blocks on. Source-major issue
// order: the scale bytes, the fp32 partial, the codes.
template <int NSRC, int U, bool PART, bool GUARD>
__device__ __forceinline__ void mx6Load6(u32x4 (&part)[U][8], u32x2 (&v)[NSRC][U][3], uint32_t (&e)[NSRC][U],
                                         const void* const (&src)[NSRC], const uint8_t* const (&ss)[NSRC], uint64_t b0,
                                         uint64_t nBlocks) {
#pragma unroll
  for (int s = PART ? 1 : 0; s < NSRC; s++)
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint64_t b = b0 + (uint64_t)u * kBlock;
      e[s][u] = (!GUARD || b < nBlocks) ? (uint32_t)ss[s][b] : 127u;
    }
  if constexpr (PART) {
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int h = 0; h < 8; h++) {
        const uint64_t b = b0 + (uint64_t)u * kBlock;
        part[u][h] = (!GUARD || b < nBlocks) ? ldPack((const u32x4*)src[0] + b * 8 + h) : u32x4{0u, 0u, 0u, 0u};
      }
  }
#pragma unroll
  for (int s = PART ? 1 : 0; s < NSRC; s++)
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int h = 0; h < 3; h++) {
        const uint64_t b = b0 + (uint64_t)u * kBlock;
        v[s][u][h] = (!GUARD || b < nBlocks) ? __builtin_nontemporal_load((const u32x2*)src[s] + b * 3 + h) : u32x2{0u, 0u};
      }
}

template <class S, class O, int NSRC, int U, bool PART, bool PRE, bool GUARD>
__device__ __forceinline__ void mx6FoldStore6(const u32x4 (&part)[U][8], const u32x2 (&v)[NSRC][U][3],
                                              const uint32_t (&e)[NSRC][U], const float (&mul)[NSRC],
                                              void* const (&dst)[kMaxKDsts], uint8_t* const (&ds)[kMaxKDsts], int nDsts,
                                              uint64_t b0, uint64_t nBlocks) {
#pragma unroll
  for (int u = 0; u < U; u++) {
    f32x32 acc;
#pragma unroll
    for (int s = 0; s < NSRC; s++) {
      f32x32 t;
      if (PART && s == 0) {
#pragma unroll
        for (int h = 0; h < 8; h++) {
          t[4 * h] = __uint_as_float(part[u][h].x);
          t[4 * h + 1] = __uint_as_float(part[u][h].y);
          t[4 * h + 2] = __uint_as_float(part[u][h].z);
          t[4 * h + 3] = __uint_as_float(part[u][h].w);
        }
      } else {
        t = S::Fmt::wide32(u32x6{v[s][u][0].x, v[s][u][0].y, v[s][u][1].x, v[s][u][1].y, v[s][u][2].x, v[s][u][2].y});
        t = t * mxScaleIn(e[s][u]);
        if constexpr (PRE) t = t * mul[s];
      }
      acc = s == 0 ? t : acc + t;
    }
    const uint64_t blk = b0 + (uint64_t)u * kBlock;
    const bool on = !GUARD || blk < nBlocks;
    if constexpr (O::kF32) {
      if (on) {
#pragma unroll
        for (int h = 0; h < 8; h++) {
          const u32x4 o = {__float_as_uint(acc[4 * h]), __float_as_uint(acc[4 * h + 1]), __float_as_uint(acc[4 * h + 2]),
                           __float_as_uint(acc[4 * h + 3])};
#pragma unroll
          for (int d = 0; d < kMaxKDsts; d++)
            if (d == 0 || d < nDsts) stPack((u32x4*)dst[d] + blk * 8 + h, o);
        }
      }
    } else {
      uint32_t mb = 0;
#pragma unroll
      for (int i = 0; i < 32; i += 2) {
        const uint32_t m0 = mxMag(acc[i]), m1 = mxMag(acc[i + 1]);
        const uint32_t m01 = m0 > m1 ? m0 : m1;
        mb = mb > m01 ? mb : m01;   // v_max3_u32
      }
      uint32_t Sb;
      float R;
      mxScaleOut<O::kEmax>(mb, Sb, R);
      f32x16 even, odd;
#pragma unroll
      for (int i = 0; i < 16; i++) {
        even[i] = acc[2 * i] * R;
        odd[i] = acc[2 * i + 1] * R;
      }
      mx6StoreBlock<O, 1, !GUARD>(even, odd, Sb, (threadIdx.x & 3u) == 0, on, blk, dst, ds, nDsts);
    }
  }
}

// a.nPacks: the call's full blocks. U: blocks a lane owns per tile.
template <class S, class O, int NSRC, int U, bool PART>
__global__ __launch_bounds__(kBlock) void kMx6Blocks(KArgs a, MxArgs x) {
  constexpr bool FP6 = mx6IsFp6<S>();
  static_assert(!PART || NSRC >= 2, "a pass that reads a partial folds at least one more source");
  static_assert(FP6 || !O::kF32, "plain sources into fp32 is nbxReduceMultiWide");
  const float sc = loadWideArg(a.argPtr, a.arg);
  const void* src[NSRC];
  const uint8_t* ss[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; s++) {
    src[s] = a.src[s];
    ss[s] = x.srcScale[s];
  }
  void* dst[kMaxKDsts];
  uint8_t* ds[kMaxKDsts];
#pragma unroll
  for (int d = 0; d < kMaxKDsts; d++) {
    dst[d] = a.dst[d];
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
    const bool full = (t + 1) * kTile <= n;   // uniform
    if constexpr (FP6) {
      const uint64_t b0 = t * kTile + threadIdx.x;
      if (full) {
        // issue every load first, then fold
        u32x4 part[U][8];
        u32x2 v[NSRC][U][3];
        uint32_t e[NSRC][U];
        mx6Load6<NSRC, U, PART, false>(part, v, e, src, ss, b0, n);
        __builtin_amdgcn_sched_barrier(0);
        if (pre) mx6FoldStore6<S, O, NSRC, U, PART, true, false>(part, v, e, mul, dst, ds, nDsts, b0, n);
        else mx6FoldStore6<S, O, NSRC, U, PART, false, false>(part, v, e, mul, dst, ds, nDsts, b0, n);
      } else {
        // last, partial tile: loads and stores predicated per block
#pragma unroll 1
        for (int u = 0; u < U; u++) {
          u32x4 part1[1][8];
          u32x2 v1[NSRC][1][3];
          uint32_t e1[NSRC][1];
          mx6Load6<NSRC, 1, PART, true>(part1, v1, e1, src, ss, b0 + (uint64_t)u * kBlock, n);
          mx6FoldStore6<S, O, NSRC, 1, PART, true, true>(part1, v1, e1, mul, dst, ds, nDsts,
                                                          b0 + (uint64_t)u * kBlock, n);
        }
      }
    } else {
      // the wave's first group: step u of the tile is 4 x kBlock groups (256 blocks), a wave's share 256 groups
      const uint64_t c0 = t * kTile * 4 + (uint64_t)(threadIdx.x >> 6) * 256;
      if (full) {
        u32x4 part[U][4][2];
        u32x4 v[NSRC][U][4];
        mx6Load16<S, NSRC, U, PART, false>(part, v, src, c0, n * 4);
        __builtin_amdgcn_sched_barrier(0);
        if (pre) mx6FoldStore16<S, O, NSRC, U, PART, true, false>(part, v, mul, dst, ds, nDsts, c0, n);
        else mx6FoldStore16<S, O, NSRC, U, PART, false, false>(part, v, mul, dst, ds, nDsts, c0, n);
      } else {
        // last, partial tile: whole quads stay in (the exchanges need them), loads and stores predicated
#pragma unroll 1
        for (int u = 0; u < U; u++) {
          u32x4 part1[1][4][2];
          u32x4 v1[NSRC][1][4];
          const uint64_t c = c0 + (uint64_t)u * (4 * kBlock);
          mx6Load16<S, NSRC, 1, PART, true>(part1, v1, src, c, n * 4);
          mx6FoldStore16<S, O, NSRC, 1, PART, true, true>(part1, v1, mul, dst, ds, nDsts, c, n);
        }
      }
    }
  });

  // the partial last block (count % 32 elements): eight lanes of wave 0 of the last workgroup
  const int rest = (int)(a.nElts & (uint64_t)(kMxBlockElts - 1));
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < 64 && rest != 0) {
    const int lane = (int)threadIdx.x;
    mx6QuadLane<S, O, PART>(a, x, sc, NSRC, n, lane & 7, lane < 8 ? rest : 0);
  }
}

// Any alignment: eight lanes per block, four elements per lane. The trip count
// is the wave's (its eight octets loop together): shuffles are converged.
template <class S, class O, bool PART>
__global__ __launch_bounds__(kBlock) void kMx6Generic(KArgs a, MxArgs x) {
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint64_t nBlocks = (a.nElts + kMxBlockElts - 1) / kMxBlockElts;
  constexpr uint64_t kPerWG = kBlock / 8;
  const int i = (int)(threadIdx.x & 7u);
  const uint64_t octet = (threadIdx.x >> 3) & 7u;
  for (uint64_t wb = (uint64_t)blockIdx.x * kPerWG + ((threadIdx.x >> 6) << 3); wb < nBlocks;
       wb += (uint64_t)gridDim.x * kPerWG) {
    const uint64_t b = wb + octet;
    int len = 0;
    if (b < nBlocks) {
      const uint64_t left = a.nElts - b * kMxBlockElts;
      len = left < (uint64_t)kMxBlockElts ? (int)left : kMxBlockElts;
    }
    mx6QuadLane<S, O, PART>(a, x, sc, a.nSrcs, b, i, len);
  }
}

// ---------------------------------------------------------------------------
// Launch table of one source kind (MxSet, nbx_kargs.h).

template <class S, class O, int OUT, int... I, int... J>
void fillMx6Out(MxSet& ms, std::integer_sequence<int, I...>, std::integer_sequence<int, J...>) {
  constexpr bool FP6 = mx6IsFp6<S>();
  const void* first[] = {(const void*)&kMx6Blocks<S, O, I + 1, mx6Unroll(I + 1, FP6), false>...};
  const void* later[] = {nullptr, (const void*)&kMx6Blocks<S, O, J + 2, mx6Unroll(J + 2, FP6), true>...};
  setMxOut(ms, OUT, first, later, (const void*)&kMx6Generic<S, O, false>, (const void*)&kMx6Generic<S, O, true>);
}

// Plain sources store either MXFP6 type (output 0 E2M3, 1 E3M2); MXFP6 sources
// store their own type (output 0) or fp32 (output 1).
template <class S>
MxSet makeMx6Set() {
  MxSet ms{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs> all{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs - 1> fromTwo{};
  if constexpr (mx6IsFp6<S>()) {
    fillMx6Out<S, typename S::Fmt, 0>(ms, all, fromTwo);
    fillMx6Out<S, Mx6OutF32, 1>(ms, all, fromTwo);
    ms.scaled = 1;
  } else {
    fillMx6Out<S, Mx6E2M3, 0>(ms, all, fromTwo);
    fillMx6Out<S, Mx6E3M2, 1>(ms, all, fromTwo);
    ms.scaled = 0;
  }
  ms.valid = 1;
  return ms;
}

}  // namespace nbx
