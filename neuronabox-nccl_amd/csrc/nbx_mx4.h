// nbx_mx4.h — MXFP4 (E2M1) elements in the block-scaled fp32-accumulating sum
// (nbxReduceMultiWideMx with NBX_FLOAT4_E2M1, include/nbx_reduce.h).
//
// The fold, the block maximum and the scale rule are nbx_mx.h's (mxScaleIn,
// mxMag, mxScaleOut with emax = 2). New is the element: two 4-bit codes share a
// byte (element 2 j the low nibble of byte j), a block of 32 is 16 bytes, and
// the type has no NaN or inf code — a non-finite block stores the scale byte
// 0xFF over all-zero codes, and a 0xFF source block reads as NaN through its
// scale. At half a byte per element the MXFP8 lane-pair layout no longer fits
// (a 16-element group would be an 8-byte load), so the layout is its own.
//
// Source kinds: plain f16 / bf16 (Mx4Src16, MXFP4 output only) and MXFP4
// (Mx4SrcFp4, MXFP4 or fp32 output). Two kernels per (kind, output, PART):
//   * kMx4Blocks<S, OUT32, NSRC, U, PART>: every element pointer 16-byte
//     aligned, every destination scale pointer 4-byte aligned. The quad
//     layout: a lane holds one 8-element group and a block is four adjacent
//     lanes. Per lane and step a 16-bit source is one dwordx4 at unit stride
//     (1 KiB contiguous per wave instruction), an FP4 source one dword, the
//     fp32 partial two dwordx4; an FP4 destination is one dword store, an fp32
//     destination two dwordx4. U steps are issued source-major ahead of the
//     fold (mxLoadTile's order: scale bytes, partial, elements). Each lane takes
//     the integer maximum of its 8 magnitudes, two DPP quad_perm exchanges
//     ([1,0,3,2], then [2,3,0,1]) give all four lanes the block's, and every
//     lane derives S and R. Source scale bytes are read by all four lanes of a
//     quad: one byte-load wave instruction. In a full tile a row of 16 lanes
//     holds four consecutive blocks, whose scale bytes are gathered over DPP
//     row_shl 4 / 8 / 12 into one dword stored by the row's first lane; the
//     last, partial tile stores bytes. The count % 32 tail is mx4ByteLane's,
//     run by a quarter wave of the last workgroup. Static tile schedule: no
//     LDS, no barrier, nothing read twice; in place a lane overwrites exactly
//     the bytes it read.
//   * kMx4Generic<S, OUT32, PART>: any alignment. A lane holds one FP4 byte
//     (two elements, so two lanes never share a destination byte), a block is
//     16 lanes, its maximum a 4-step xor butterfly, loads and stores element
//     sized. The block kernel's operations on the same values in the same order.
//
// Converters (scripts/probe_fp4_cvt.hip, profiles/r15/probe_fp4_cvt_mi355x.txt):
// v_cvt_scalef32_pk_f32_fp4 at scale 1.0 is the 16-entry table exactly, signed
// zeros included, and v_cvt_scalef32_pk_fp4_f32 at scale 1.0 is RNE onto the
// eight magnitudes with everything above 6 (inf too) stored as +-6, equal to
// seven compares on 1.18 M inputs; both are used. The source scale does NOT go
// through the decoder's scale operand: it is equal for e <= 254 (e = 0 and
// denormal products included) but gives 0xffc00000 where the contract's
// multiply by the 0xFF block's NaN gives 0x7fc00000.
#pragma once
#include "nbx_mx.h"

namespace nbx {

template <class Ty>
struct Mx4Src16 {
  using W = WideTy<Ty>;
  using Raw = u32x4;                         // a lane's 8 elements of one step
  static constexpr bool kFp4 = false;
  __device__ static Raw load(const void* p, uint64_t g) { return ldPack((const u32x4*)p + g); }
  __device__ static void wide8(const Raw& v, f32x2 (&t)[4]) {
#pragma unroll
    for (int w = 0; w < 4; w++) W::wideWord(v[w], &t[w]);
  }
  // elements 2 j, 2 j + 1 of the bucket (generic kernel and tail); on: which exist
  __device__ static f32x2 wide2(const void* p, uint64_t j, bool on0, bool on1) {
    const uint16_t* e = (const uint16_t*)p + 2 * j;
    return f32x2{on0 ? W::wide(e[0]) : 0.0f, on1 ? W::wide(e[1]) : 0.0f};
  }
};

struct Mx4SrcFp4 {
  using Raw = uint32_t;
  static constexpr bool kFp4 = true;
  __device__ static Raw load(const void* p, uint64_t g) { return __builtin_nontemporal_load((const uint32_t*)p + g); }
  __device__ static void wide8(const Raw& v, f32x2 (&t)[4]) {
    t[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, 1.0f, 0);
    t[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, 1.0f, 1);
    t[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, 1.0f, 2);
    t[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, 1.0f, 3);
  }
  // an odd count's last high nibble is ignored: it decodes, and on1 drops it
  __device__ static f32x2 wide2(const void* p, uint64_t j, bool on0, bool on1) {
    const f32x2 t = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(on0 ? (uint32_t)((const uint8_t*)p)[j] : 0u, 1.0f, 0);
    return f32x2{t[0], on1 ? t[1] : 0.0f};
  }
};

// narrow4 of two / eight scaled accumulators: RNE onto E2M1, above 6 stores +-6.
__device__ __forceinline__ uint32_t mx4Narrow2(float lo, float hi) {
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, lo, hi, 1.0f, 0) & 0xffu;
}
__device__ __forceinline__ uint32_t mx4Narrow8(const f32x2 (&a)[4]) {
  uint32_t w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, a[0][0], a[0][1], 1.0f, 0);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, a[1][0], a[1][1], 1.0f, 1);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, a[2][0], a[2][1], 1.0f, 2);
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, a[3][0], a[3][1], 1.0f, 3);
}

// quad_perm [2, 3, 0, 1]: the value of lane ^ 2.
__device__ __forceinline__ uint32_t mx4QuadSwap2(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);
}

// One FP4 byte of block b per lane: lane i of 16 holds elements 32 b + 2 i and
// + 1, those below len (len = 0: an idle quarter wave). Called by whole waves,
// converged; the four quarters of a wave may hold different blocks.
template <class S, bool OUT32, bool PART>
__device__ __forceinline__ void mx4ByteLane(const KArgs& a, const MxArgs& x, float sc, int nSrcs, uint64_t b, int i,
                                            int len) {
  const bool on0 = 2 * i < len, on1 = 2 * i + 1 < len;
  const uint64_t j = b * (kMxBlockElts / 2) + (uint64_t)i;   // the byte, and the element pair
  f32x2 acc = {0.0f, 0.0f};
  if (on0) {
#pragma unroll
    for (int s = 0; s < kMaxKSrcs; s++) {
      if (s < nSrcs) {
        f32x2 v;
        if (PART && s == 0) {
          const float* p = (const float*)a.src[0] + 2 * j;
          v = f32x2{p[0], on1 ? p[1] : 0.0f};
        } else {
          v = S::wide2(a.src[s], j, on0, on1);
          if constexpr (S::kFp4) {
            const float xs = mxScaleIn(x.srcScale[s][b]);
            v = f32x2{v[0] * xs, v[1] * xs};
          }
          if ((a.preMask >> s) & 1u) v = f32x2{v[0] * sc, v[1] * sc};
        }
        acc = s == 0 ? v : f32x2{acc[0] + v[0], acc[1] + v[1]};
      }
    }
    if (!on1) acc[1] = 0.0f;   // an element that is not there takes no part in the maximum
  }
  if constexpr (OUT32) {
#pragma unroll
    for (int d = 0; d < kMaxKDsts; d++) {
      if (d < a.nDsts) {
        if (on0) ((float*)a.dst[d])[2 * j] = acc[0];
        if (on1) ((float*)a.dst[d])[2 * j + 1] = acc[1];
      }
    }
  } else {
    const uint32_t m0 = mxMag(acc[0]), m1 = mxMag(acc[1]);
    uint32_t mb = m0 > m1 ? m0 : m1;
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)mb, o, 64);
      mb = mb > other ? mb : other;
    }
    uint32_t Sb;
    float R;
    mxScaleOut<2>(mb, Sb, R);
    if (on0) {
      uint32_t code = mx4Narrow2(acc[0] * R, acc[1] * R);
      if (!on1) code &= 0xfu;          // an odd count's last high nibble is stored as 0
      if (Sb == 0xffu) code = 0;       // no NaN code: the scale byte says it
#pragma unroll
      for (int d = 0; d < kMaxKDsts; d++) {
        if (d < a.nDsts) {
          ((uint8_t*)a.dst[d])[j] = (uint8_t)code;
          if (i == 0) x.dstScale[d][b] = (uint8_t)Sb;
        }
      }
    }
  }
}

// Source-major issue order: the scale bytes (all four lanes of a quad read
// their block's with the one wave instruction), the fp32 partial, the elements.
template <class S, int NSRC, int U, bool PART>
__device__ __forceinline__ void mx4LoadTile(u32x4 (&part)[U][2], typename S::Raw (&v)[NSRC][U], uint32_t (&e)[NSRC][U],
                                            const void* const (&src)[NSRC], const uint8_t* const (&ss)[NSRC],
                                            uint64_t g) {
  if constexpr (S::kFp4) {
#pragma unroll
    for (int s = PART ? 1 : 0; s < NSRC; s++)
#pragma unroll
      for (int u = 0; u < U; u++) e[s][u] = ss[s][(g + (uint64_t)u * kBlock) >> 2];
  }
  if constexpr (PART) {
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int k = 0; k < 2; k++) part[u][k] = ldPack((const u32x4*)src[0] + (g + (uint64_t)u * kBlock) * 2 + k);
  }
#pragma unroll
  for (int s = PART ? 1 : 0; s < NSRC; s++)
#pragma unroll
    for (int u = 0; u < U; u++) v[s][u] = S::load(src[s], g + (uint64_t)u * kBlock);
}

// Fold U groups already in registers, scale and store them. mul: the scalar or
// 1.0 per source (PRE only). GATHER: all 64 lanes of the wave are here with
// full blocks, and each step's 16 scale bytes leave as 4 dword stores; else
// the first lane of a quad stores its byte.
template <class S, bool OUT32, int NSRC, int U, bool PART, bool PRE, bool GATHER>
__device__ __forceinline__ void mx4FoldStore(const u32x4 (&part)[U][2], const typename S::Raw (&v)[NSRC][U],
                                             const uint32_t (&e)[NSRC][U], const float (&mul)[NSRC],
                                             void* const (&dst)[kMaxKDsts], uint8_t* const (&ds)[kMaxKDsts], int nDsts,
                                             uint64_t g) {
#pragma unroll
  for (int u = 0; u < U; u++) {
    f32x2 acc[4];
#pragma unroll
    for (int s = 0; s < NSRC; s++) {
      f32x2 t[4];
      if (PART && s == 0) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
          t[2 * k] = f32x2{__uint_as_float(part[u][k].x), __uint_as_float(part[u][k].y)};
          t[2 * k + 1] = f32x2{__uint_as_float(part[u][k].z), __uint_as_float(part[u][k].w)};
        }
      } else {
        S::wide8(v[s][u], t);
        if constexpr (S::kFp4) {
          const float xs = mxScaleIn(e[s][u]);
          const f32x2 m = {xs, xs};
#pragma unroll
          for (int k = 0; k < 4; k++) t[k] = t[k] * m;
        }
        if constexpr (PRE) {
          const f32x2 m = {mul[s], mul[s]};
#pragma unroll
          for (int k = 0; k < 4; k++) t[k] = t[k] * m;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; k++) acc[k] = s == 0 ? t[k] : acc[k] + t[k];
    }
    const uint64_t q = g + (uint64_t)u * kBlock;
    if constexpr (OUT32) {
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const u32x4 o = {__float_as_uint(acc[2 * k][0]), __float_as_uint(acc[2 * k][1]),
                         __float_as_uint(acc[2 * k + 1][0]), __float_as_uint(acc[2 * k + 1][1])};
        stPack((u32x4*)dst[0] + q * 2 + k, o);
#pragma unroll
        for (int d = 1; d < kMaxKDsts; d++)
          if (d < nDsts) stPack((u32x4*)dst[d] + q * 2 + k, o);
      }
    } else {
      uint32_t mb = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t m0 = mxMag(acc[k][0]), m1 = mxMag(acc[k][1]);
        const uint32_t m01 = m0 > m1 ? m0 : m1;
        mb = mb > m01 ? mb : m01;   // v_max3_u32
      }
      uint32_t other = mxPairSwap(mb);
      mb = mb > other ? mb : other;
      other = mx4QuadSwap2(mb);
      mb = mb > other ? mb : other;
      uint32_t Sb;
      float R;
      mxScaleOut<2>(mb, Sb, R);
      const f32x2 r = {R, R};
#pragma unroll
      for (int k = 0; k < 4; k++) acc[k] = acc[k] * r;
      const uint32_t o = Sb == 0xffu ? 0u : mx4Narrow8(acc);   // no NaN code: the scale byte says it
      ((uint32_t*)dst[0])[q] = o;
#pragma unroll
      for (int d = 1; d < kMaxKDsts; d++)
        if (d < nDsts) ((uint32_t*)dst[d])[q] = o;
      // group q is a quarter of block q / 4: lanes 16 j .. 16 j + 15 hold blocks
      // q / 4 .. q / 4 + 3 of lane 16 j, whose byte address is 4-byte aligned
      if constexpr (GATHER) {
        const uint32_t word = Sb | (mxRowShl<4>(Sb) << 8) | (mxRowShl<8>(Sb) << 16) | (mxRowShl<12>(Sb) << 24);
        if ((threadIdx.x & 15u) == 0) {
          *(uint32_t*)(ds[0] + (q >> 2)) = word;
#pragma unroll
          for (int d = 1; d < kMaxKDsts; d++)
            if (d < nDsts) *(uint32_t*)(ds[d] + (q >> 2)) = word;
        }
      } else {
        if ((threadIdx.x & 3u) == 0) {
          ds[0][q >> 2] = (uint8_t)Sb;
#pragma unroll
          for (int d = 1; d < kMaxKDsts; d++)
            if (d < nDsts) ds[d][q >> 2] = (uint8_t)Sb;
        }
      }
    }
  }
}

// a.nPacks: the 8-element groups of the call's full blocks (a multiple of 4).
template <class S, bool OUT32, int NSRC, int U, bool PART>
__global__ __launch_bounds__(kBlock) void kMx4Blocks(KArgs a, MxArgs x) {
  static_assert(!PART || NSRC >= 2, "a pass that reads a partial folds at least one more source");
  static_assert(S::kFp4 || !OUT32, "plain sources into fp32 is nbxReduceMultiWide");
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
    const uint64_t g = t * kTile + threadIdx.x;
    if ((t + 1) * kTile <= n) {
      // full tile (uniform): issue every load first, then fold
      u32x4 part[U][2];
      typename S::Raw v[NSRC][U];
      uint32_t e[NSRC][U];
      mx4LoadTile<S, NSRC, U, PART>(part, v, e, src, ss, g);
      __builtin_amdgcn_sched_barrier(0);
      if (pre) mx4FoldStore<S, OUT32, NSRC, U, PART, true, true>(part, v, e, mul, dst, ds, nDsts, g);
      else mx4FoldStore<S, OUT32, NSRC, U, PART, false, true>(part, v, e, mul, dst, ds, nDsts, g);
    } else {
      // last, partial tile: n is a multiple of 4, so a quad is in or out together
#pragma unroll 1
      for (int u = 0; u < U; u++) {
        const uint64_t q = g + (uint64_t)u * kBlock;
        if (q < n) {
          u32x4 part1[1][2];
          typename S::Raw v1[NSRC][1];
          uint32_t e1[NSRC][1];
          mx4LoadTile<S, NSRC, 1, PART>(part1, v1, e1, src, ss, q);
          mx4FoldStore<S, OUT32, NSRC, 1, PART, true, false>(part1, v1, e1, mul, dst, ds, nDsts, q);
        }
      }
    }
  });

  // the partial last block (count % 32 elements): wave 0 of the last workgroup
  const int rest = (int)(a.nElts & (uint64_t)(kMxBlockElts - 1));
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < 64 && rest != 0) {
    const int lane = (int)threadIdx.x;
    mx4ByteLane<S, OUT32, PART>(a, x, sc, NSRC, n >> 2, lane & 15, lane < 16 ? rest : 0);
  }
}

// Any alignment: a quarter wave per block, one FP4 byte per lane. The trip
// count is the wave's (its four quarters loop together): shuffles are converged.
template <class S, bool OUT32, bool PART>
__global__ __launch_bounds__(kBlock) void kMx4Generic(KArgs a, MxArgs x) {
  const float sc = loadWideArg(a.argPtr, a.arg);
  const uint64_t nBlocks = (a.nElts + kMxBlockElts - 1) / kMxBlockElts;
  constexpr uint64_t kPerWG = kBlock / (kMxBlockElts / 2);
  const int i = (int)(threadIdx.x & 15u);
  const uint64_t quarter = (threadIdx.x >> 4) & 3u;
  for (uint64_t wb = (uint64_t)blockIdx.x * kPerWG + ((threadIdx.x >> 6) << 2); wb < nBlocks;
       wb += (uint64_t)gridDim.x * kPerWG) {
    const uint64_t b = wb + quarter;
    int len = 0;
    if (b < nBlocks) {
      const uint64_t left = a.nElts - b * kMxBlockElts;
      len = left < (uint64_t)kMxBlockElts ? (int)left : kMxBlockElts;
    }
    mx4ByteLane<S, OUT32, PART>(a, x, sc, a.nSrcs, b, i, len);
  }
}

// ---------------------------------------------------------------------------
// Launch table of one source kind (MxSet, nbx_kargs.h).

template <class S, bool OUT32, int... I, int... J>
void fillMx4Out(MxSet& ms, std::integer_sequence<int, I...>, std::integer_sequence<int, J...>) {
  const void* first[] = {(const void*)&kMx4Blocks<S, OUT32, I + 1, mx4Unroll(I + 1, S::kFp4), false>...};
  const void* later[] = {nullptr, (const void*)&kMx4Blocks<S, OUT32, J + 2, mx4Unroll(J + 2, S::kFp4), true>...};
  setMxOut(ms, OUT32, first, later, (const void*)&kMx4Generic<S, OUT32, false>,
           (const void*)&kMx4Generic<S, OUT32, true>);
}

// Plain sources store MXFP4 only (output 0); MXFP4 sources also store fp32 (output 1).
template <class S>
MxSet makeMx4Set() {
  MxSet ms{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs> all{};
  constexpr std::make_integer_sequence<int, kMaxKSrcs - 1> fromTwo{};
  fillMx4Out<S, false>(ms, all, fromTwo);
  if constexpr (S::kFp4) fillMx4Out<S, true>(ms, all, fromTwo);
  ms.scaled = S::kFp4 ? 1 : 0;
  ms.valid = 1;
  return ms;
}

}  // namespace nbx
