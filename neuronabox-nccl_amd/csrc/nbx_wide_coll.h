// nbx_wide_coll.h — fp32-accumulating ("wide") sums in the collectives' direct
// schedules (nbxRedOpCreateWide, include/nbx_reduce.h).
//
// Every direct schedule moves raw inputs and folds them at the receiver:
// kLLColl / kLL128Coll hold all n inputs of a word, kLL128AllReduce2 and the
// direct Simple schedule fold block `me` from the own input and the n-1 raw
// slots and only then push finished blocks. So a wide sum is a different fold
// over the same wire bytes: FnWide below, which the fold sites of nbx_ll.h
// and nbx_simple.h take where Fn::kWide (an fp32 WideAcc beside the codes).
// Only the ring (kSimpleRing) moves partials; it has no wide form.
//
// The arithmetic is nbxReduceMultiWide's (nbx_wide.h), through the same
// WideTy<Ty> helpers: exact widening, one unfused fp32 multiply by the scalar
// for EVERY source, fp32 adds in the schedule's operand order, one narrowing.
// One instantiation serves wide Sum and wide Avg: Sum passes the scalar 1.0f,
// and x * 1.0f is x for every fp32 x that is no signalling NaN (which the add
// quiets as well), so the bits are the plain sum's — half the kernels of a
// Sum / PreMulSum pair (40 instead of 80), for one v_pk_mul_f32 per pair.
#pragma once
#include "nbx_wide.h"

namespace nbx {

template <class Ty>
struct FnWide {
  using W = WideTy<Ty>;
  using Elt = typename W::Elt;
  static constexpr bool kWide = true;
  static constexpr bool kHasPre = false;    // the scalar is part of the fold
  static constexpr bool kHasPost = false;
  static constexpr int kWP = W::kWP;        // fp32 pairs per dword of codes
  float scalar;                             // fp32 bits in the low half of the launch's scalar argument
  __device__ explicit FnWide(uint64_t arg) : scalar(__uint_as_float((uint32_t)arg)) {}
  // one dword of codes into its kWP accumulator pairs
  __device__ __forceinline__ void foldWord(f32x2* acc, uint32_t w, bool first) const {
    f32x2 t[kWP];
    W::wideWord(w, t);
    const f32x2 m = {scalar, scalar};
#pragma unroll
    for (int k = 0; k < kWP; k++) {
      t[k] = t[k] * m;
      acc[k] = first ? t[k] : acc[k] + t[k];
    }
  }
  __device__ static uint32_t narrowWord(const f32x2* acc) { return W::narrowWord(acc); }
  // one element (unaligned buffers, tails)
  __device__ float wideElt(Elt e) const { return W::wide(e) * scalar; }
  __device__ static Elt narrowElt(float c) { return W::narrow(c); }
};

// The direct Simple schedule over FnWide under a name of its own, as
// kWidePacks stands beside kReducePacks: the per-step Simple kernels (direct,
// ring, and their checking forms per functor) are counted by name
// (tests/test_code_object.py), and this one has no ring sibling.
template <class Ty, bool CHK>
__global__ __launch_bounds__(kBlock) void kWideSimpleColl(SimpleArgs a) {
  simpleCollBody<FnWide<Ty>, CHK>(a, simpleKernargSegs(), (int)blockIdx.x, (int)gridDim.x);
}

template <class Ty>
WideCollSet makeWideCollSet() {
  using Fn = FnWide<Ty>;
  WideCollSet s{};
  s.ll = (const void*)&kLLColl<Fn, false>;
  s.ll128 = (const void*)&kLL128Coll<Fn, false>;
  s.ll128x2 = (const void*)&kLL128AllReduce2<Fn, false>;
  s.llChk = (const void*)&kLLColl<Fn, true>;
  s.ll128Chk = (const void*)&kLL128Coll<Fn, true>;
  s.ll128x2Chk = (const void*)&kLL128AllReduce2<Fn, true>;
  s.simple = (const void*)&kWideSimpleColl<Ty, false>;
  s.simpleChk = (const void*)&kWideSimpleColl<Ty, true>;
  s.valid = 1;
  return s;
}

}  // namespace nbx
