// probe_fp4_cvt.hip — what gfx950's FP4 converters do at the edges, against the
// integer forms that include/nbx_reduce.h's MXFP4 contract is written in.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off scripts/probe_fp4_cvt.hip -o probe_fp4_cvt && ./probe_fp4_cvt
// 1. decode: v_cvt_scalef32_pk_f32_fp4 at scale 1.0, every byte, every byte
//    select, against the 16-entry table (signed zeros included).
// 2. decode with the block scale in the converter's scale operand, every byte
//    and every scale byte e (X = 2^(e-127), e = 0 the denormal, e = 0xFF a NaN),
//    against decode-at-1.0 followed by one fp32 multiply by X.
// 3. narrow: v_cvt_scalef32_pk_fp4_f32 at scale 1.0 against seven compares on
//    the magnitude bits (RNE, everything above 6 saturates): every tie and its
//    fp32 neighbours, zeros, denormals, (6, 8], a dense sweep of [-9, 9], huge
//    values, inf. NaN is printed, not compared: the kernels never narrow one.
// Prints one line per part; exit status 0 whatever the converters do.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ float scaleIn(uint32_t e) {
  return __uint_as_float((e << 23) | (((e + 1u) & 0xffu) <= 1u ? 0x400000u : 0u));
}

// out[(e * 256 + byte) * 2 + {0, 1}]: e < 256 the scale operand, e = 256 decode at 1.0 then multiply is
// in ref[]; sel[]: byte selects 1..3 at scale 1.0
__global__ void kDecode(uint32_t* viaOperand, uint32_t* viaMul, uint32_t* sel) {
  const uint32_t byte = threadIdx.x, e = blockIdx.x;
  const float x = scaleIn(e);
  const f32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(byte, x, 0);
  const f32x2 b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(byte, 1.0f, 0);
  const uint32_t o = (e * 256 + byte) * 2;
  viaOperand[o] = __float_as_uint(a[0]);
  viaOperand[o + 1] = __float_as_uint(a[1]);
  viaMul[o] = __float_as_uint(b[0] * x);
  viaMul[o + 1] = __float_as_uint(b[1] * x);
  if (e == 127) {
    const f32x2 s1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(byte << 8, 1.0f, 1);
    const f32x2 s2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(byte << 16, 1.0f, 2);
    const f32x2 s3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(byte << 24, 1.0f, 3);
    sel[byte] = (s1[0] == b[0] && s1[1] == b[1] && s2[0] == b[0] && s2[1] == b[1] && s3[0] == b[0] && s3[1] == b[1] &&
                 __float_as_uint(s3[0]) == __float_as_uint(b[0]))
                    ? 1u : 0u;
  }
}

__device__ uint32_t narrowInt(float v) {
  const uint32_t b = __float_as_uint(v), u = b & 0x7fffffffu;
  const uint32_t c = (u > 0x3e800000u) + (u >= 0x3f400000u) + (u > 0x3fa00000u) + (u >= 0x3fe00000u) +
                     (u > 0x40200000u) + (u >= 0x40600000u) + (u > 0x40a00000u);
  return c | ((b >> 28) & 8u);
}

__global__ void kNarrow(const float* in, uint32_t* hw, uint32_t* ref, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  hw[i] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, in[i], 0.0f, 1.0f, 0) & 0xffu;
  ref[i] = narrowInt(in[i]);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("hip: %s\n", hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  static const float kTable[8] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 4.0f, 6.0f};
  const size_t nd = 256 * 256 * 2;
  uint32_t *dOp, *dMul, *dSel;
  CK(hipMalloc(&dOp, nd * 4));
  CK(hipMalloc(&dMul, nd * 4));
  CK(hipMalloc(&dSel, 256 * 4));
  kDecode<<<256, 256>>>(dOp, dMul, dSel);
  std::vector<uint32_t> op(nd), mul(nd), sel(256);
  CK(hipMemcpy(op.data(), dOp, nd * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(mul.data(), dMul, nd * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(sel.data(), dSel, 256 * 4, hipMemcpyDeviceToHost));
  int badTable = 0, badSel = 0;
  for (uint32_t byte = 0; byte < 256; byte++) {
    for (int h = 0; h < 2; h++) {
      const uint32_t code = (byte >> (4 * h)) & 15u;
      float want = kTable[code & 7];
      uint32_t wb;
      std::memcpy(&wb, &want, 4);
      wb |= (code & 8u) << 28;
      if (op[(127 * 256 + byte) * 2 + h] != wb) badTable++;
    }
    if (!sel[byte]) badSel++;
  }
  std::printf("decode at scale 1.0: %d of 512 differ from the table; byte selects 1..3: %d of 256 bytes differ\n",
              badTable, badSel);
  long badOp = 0, badNanOnly = 0;
  int shown = 0;
  for (uint32_t e = 0; e < 256; e++) {
    long badHere = 0;
    for (uint32_t i = 0; i < 512; i++) {
      const uint32_t a = op[e * 512 + i], m = mul[e * 512 + i];
      if (a == m) continue;
      const bool bothNan = (a & 0x7fffffffu) > 0x7f800000u && (m & 0x7fffffffu) > 0x7f800000u;
      if (bothNan) badNanOnly++;
      else badHere++;
      if (shown < 12 && (e == 0 || e == 255 || !bothNan)) {
        std::printf("  e=%u byte=%02x half=%u: scale operand %08x, multiply %08x\n", e, i >> 1, i & 1, a, m);
        shown++;
      }
    }
    badOp += badHere;
  }
  std::printf("decode with the scale in the operand: %ld of 131072 differ from decode-then-multiply "
              "(plus %ld that are NaN both ways with other bits)\n", badOp, badNanOnly);

  std::vector<float> in;
  const uint32_t ties[] = {0x3e800000u, 0x3f400000u, 0x3fa00000u, 0x3fe00000u, 0x40200000u, 0x40600000u, 0x40a00000u,
                           0x40c00000u, 0x40e00000u, 0x41000000u, 0x3f000000u, 0x3f800000u, 0x40000000u, 0x40800000u};
  for (uint32_t t : ties)
    for (int d = -2; d <= 2; d++)
      for (uint32_t s = 0; s < 2; s++) {
        const uint32_t b = (t + (uint32_t)d) | (s << 31);
        float f;
        std::memcpy(&f, &b, 4);
        in.push_back(f);
      }
  const uint32_t odd[] = {0u, 0x80000000u, 1u, 0x80000001u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0xff7fffffu,
                          0x7f800000u, 0xff800000u, 0x50000000u};
  for (uint32_t b : odd) {
    float f;
    std::memcpy(&f, &b, 4);
    in.push_back(f);
  }
  for (int i = -589824; i <= 589824; i++) in.push_back((float)i / 65536.0f);   // [-9, 9] in steps of 2^-16
  const int n = (int)in.size();
  in.push_back(NAN);
  in.push_back(-NAN);
  float* dIn;
  uint32_t *dHw, *dRef;
  CK(hipMalloc(&dIn, in.size() * 4));
  CK(hipMalloc(&dHw, in.size() * 4));
  CK(hipMalloc(&dRef, in.size() * 4));
  CK(hipMemcpy(dIn, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  kNarrow<<<(unsigned)((in.size() + 255) / 256), 256>>>(dIn, dHw, dRef, (int)in.size());
  std::vector<uint32_t> hw(in.size()), ref(in.size());
  CK(hipMemcpy(hw.data(), dHw, in.size() * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(ref.data(), dRef, in.size() * 4, hipMemcpyDeviceToHost));
  int badN = 0;
  for (int i = 0; i < n; i++) {
    if (hw[i] == ref[i]) continue;
    if (badN++ < 12) {
      uint32_t b;
      std::memcpy(&b, &in[i], 4);
      std::printf("  narrow %08x (%g): converter %x, compares %x\n", b, in[i], hw[i], ref[i]);
    }
  }
  std::printf("narrow at scale 1.0: %d of %d differ from the seven compares; NaN -> %x, -NaN -> %x\n", badN, n, hw[n],
              hw[n + 1]);
  return 0;
}
