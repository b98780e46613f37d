// probe_fp6_cvt.hip — what gfx950's FP6 converters do at scale 1.0, against the
// integer forms that include/nbx_reduce.h's MXFP6 contract is written in.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off scripts/probe_fp6_cvt.hip -o probe_fp6_cvt && ./probe_fp6_cvt
// 1. order: v_cvt_scalef32_2xpk16_{fp6,bf6}_f32 takes two v16f32 and gives six
//    dwords. One element of the 32 is set to 1.0, the others 0: which 6-bit field
//    of the contract's little-endian stream (element i in bits [6 i, 6 i + 6))
//    holds the code says where operand a[i] and b[i] land.
// 2. decode: v_cvt_scalef32_pk32_f32_{fp6,bf6}, all 64 codes in all 32 places of
//    the stream, against the contract's table (signed zeros included).
// 3. narrow: every grid point, every tie and their fp32 neighbours, zeros,
//    denormals, the saturating ranges, a dense sweep, huge values and inf against
//    RNE in integer arithmetic (everything above the largest stores the largest).
//    NaN is printed, not compared: the kernels never narrow one.
// Prints a few lines per type; exit status 0 whatever the converters do.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v32f __attribute__((ext_vector_type(32)));
typedef uint32_t v6u __attribute__((ext_vector_type(6)));

// MB mantissa bits, BIAS: E2M3 (3, 1), E3M2 (2, 3)
template <int MB, int BIAS>
__host__ __device__ uint32_t narrowInt(uint32_t b) {
  const uint32_t u = b & 0x7fffffffu, sign = (b >> 26) & 0x20u;
  constexpr int SH = 23 - MB;
  constexpr uint32_t kMinNormal = (uint32_t)(128 - BIAS) << 23;   // 2^(1 - BIAS)
  uint32_t c;
  if (u > 0x7f800000u) {
    c = 0x1f;
  } else if (u < kMinNormal) {
    // subnormal grid: multiples of 2^(1 - BIAS - MB); RNE on the integer quotient
    const int e = (int)(u >> 23);
    const int drop = (127 + 1 - BIAS - MB) - e + 23;   // bits of the 24-bit significand below the grid
    const uint32_t sig = e ? ((u & 0x7fffffu) | 0x800000u) : 0u;   // fp32 denormals are far below half a step
    if (drop > 25 || sig == 0) c = 0;
    else {
      const uint32_t q = sig >> drop, r = sig & ((1u << drop) - 1u), half = 1u << (drop - 1);
      c = q + ((r > half || (r == half && (q & 1u))) ? 1u : 0u);
    }
  } else {
    const uint32_t r = u + ((1u << (SH - 1)) - 1u) + ((u >> SH) & 1u);
    c = (r >> SH) - ((uint32_t)(127 - BIAS) << MB);
    if (c > 0x1fu) c = 0x1fu;
  }
  return c | sign;
}

template <int MB, int BIAS>
float decodeTable(uint32_t code) {
  const uint32_t mag = code & 31u, e = mag >> MB, m = mag & ((1u << MB) - 1u);
  const float v = e ? std::ldexp(1.0f + (float)m / (float)(1 << MB), (int)e - BIAS)
                    : std::ldexp((float)m / (float)(1 << MB), 1 - BIAS);
  return (code & 32u) ? -v : v;
}

template <bool BF6>
__device__ v6u narrowHw(v16f a, v16f b) {
  if constexpr (BF6) return __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, 1.0f);
  else return __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, 1.0f);
}
template <bool BF6>
__device__ v32f decodeHw(v6u w) {
  if constexpr (BF6) return __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(w, 1.0f);
  else return __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(w, 1.0f);
}

// thread t < 32: a[t] = 1.0 (t < 16) or b[t - 16] = 1.0; out[t * 6 + k] the dwords
template <bool BF6>
__global__ void kOrder(uint32_t* out) {
  const int t = threadIdx.x;
  v16f a, b;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    a[i] = t == i ? 1.0f : 0.0f;
    b[i] = t == i + 16 ? 1.0f : 0.0f;
  }
  const v6u w = narrowHw<BF6>(a, b);
#pragma unroll
  for (int k = 0; k < 6; k++) out[t * 6 + k] = w[k];
}

// thread (place p = threadIdx.x < 32, code = blockIdx.x < 64): the code in field p
// of the stream, the others 0; out[(code * 32 + p) * 32 + i] = element i
template <bool BF6>
__global__ void kDecode(uint32_t* out) {
  const uint32_t p = threadIdx.x, code = blockIdx.x;
  uint32_t w[7] = {0, 0, 0, 0, 0, 0, 0};
  const uint32_t bit = 6 * p;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    if ((bit >> 5) == (uint32_t)k) {
      w[k] |= code << (bit & 31u);
      if ((bit & 31u) > 26u) w[k + 1] |= code >> (32u - (bit & 31u));
    }
  }
  v6u v;
#pragma unroll
  for (int k = 0; k < 6; k++) v[k] = w[k];
  const v32f f = decodeHw<BF6>(v);
#pragma unroll
  for (int i = 0; i < 32; i++) out[(code * 32 + p) * 32 + i] = __float_as_uint(f[i]);
}

// in[i] goes through operand a[0]; field: the stream field a[0] lands in (part 1)
template <bool BF6>
__global__ void kNarrow(const float* in, uint32_t* hw, int n, int field) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  v16f a, b;
#pragma unroll
  for (int k = 0; k < 16; k++) a[k] = b[k] = 0.0f;
  a[0] = in[i];
  const v6u w = narrowHw<BF6>(a, b);
  const uint32_t bit = 6u * (uint32_t)field;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    if ((bit >> 5) == (uint32_t)k) lo = w[k];
    if ((bit >> 5) + 1u == (uint32_t)k) hi = w[k];
  }
  const uint64_t both = ((uint64_t)hi << 32) | lo;
  hw[i] = (uint32_t)(both >> (bit & 31u)) & 63u;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("hip: %s\n", hipGetErrorString(e_)); return 1; } } while (0)

static uint32_t bitsOf(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static float floatOf(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

template <bool BF6, int MB, int BIAS>
int probe(const char* name) {
  // ---- 1. order ----
  uint32_t* dOrd;
  CK(hipMalloc(&dOrd, 32 * 6 * 4));
  kOrder<BF6><<<1, 32>>>(dOrd);
  std::vector<uint32_t> ord(32 * 6);
  CK(hipMemcpy(ord.data(), dOrd, ord.size() * 4, hipMemcpyDeviceToHost));
  const uint32_t one = narrowInt<MB, BIAS>(bitsOf(1.0f));
  int place[32];
  bool orderOk = true;
  for (int t = 0; t < 32; t++) {
    place[t] = -1;
    int set = 0;
    for (int f = 0; f < 32; f++) {
      const uint32_t bit = 6 * f;
      uint64_t both = ord[t * 6 + (bit >> 5)];
      if ((bit >> 5) + 1 < 6) both |= (uint64_t)ord[t * 6 + (bit >> 5) + 1] << 32;
      const uint32_t c = (uint32_t)(both >> (bit & 31u)) & 63u;
      if (c == one) { place[t] = f; set++; }
      else if (c != 0) set += 100;
    }
    if (set != 1) orderOk = false;
  }
  std::printf("%s order: fields of a[0..15] b[0..15]:", name);
  for (int t = 0; t < 32; t++) std::printf(" %d", place[t]);
  std::printf("%s\n", orderOk ? "" : "  (NOT one clean field each)");

  // ---- 2. decode ----
  const size_t nd = 64 * 32 * 32;
  uint32_t* dDec;
  CK(hipMalloc(&dDec, nd * 4));
  kDecode<BF6><<<64, 32>>>(dDec);
  std::vector<uint32_t> dec(nd);
  CK(hipMemcpy(dec.data(), dDec, nd * 4, hipMemcpyDeviceToHost));
  int badDec = 0, badPlace = 0, shown = 0;
  for (uint32_t code = 0; code < 64; code++)
    for (uint32_t p = 0; p < 32; p++)
      for (uint32_t i = 0; i < 32; i++) {
        const uint32_t got = dec[(code * 32 + p) * 32 + i];
        const uint32_t want = i == p ? bitsOf(decodeTable<MB, BIAS>(code)) : 0u;
        if (got == want) continue;
        if (i == p) badDec++; else badPlace++;
        if (shown++ < 8) std::printf("  decode code %02x in field %u: element %u is %08x, table %08x\n", code, p, i, got, want);
      }
  std::printf("%s decode at scale 1.0: %d of 2048 (code, field) pairs differ from the table; %d other elements not +0\n",
              name, badDec, badPlace);

  // ---- 3. narrow ----
  std::vector<float> in;
  for (uint32_t code = 0; code < 32; code++) {
    // every grid point, the midpoint to the next one, and their neighbours
    const float v = decodeTable<MB, BIAS>(code);
    const float nx = code < 31 ? decodeTable<MB, BIAS>(code + 1) : 2.0f * v - decodeTable<MB, BIAS>(code - 1);
    const uint32_t pts[2] = {bitsOf(v), bitsOf(0.5f * (v + nx))};
    for (uint32_t t : pts)
      for (int d = -2; d <= 2; d++)
        for (uint32_t s = 0; s < 2; s++) {
          if (t == 0 && d < 0) continue;
          in.push_back(floatOf((t + (uint32_t)d) | (s << 31)));
        }
  }
  const uint32_t odd[] = {0u, 0x80000000u, 1u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x7f7fffffu,
                          0xff7fffffu, 0x7f800000u, 0xff800000u, 0x50000000u, 0xd0000000u};
  for (uint32_t b : odd) in.push_back(floatOf(b));
  for (int i = -2359296; i <= 2359296; i++) in.push_back((float)i / 65536.0f);   // [-36, 36] in steps of 2^-16
  const int n = (int)in.size();
  in.push_back(NAN);
  in.push_back(-NAN);
  float* dIn;
  uint32_t* dHw;
  CK(hipMalloc(&dIn, in.size() * 4));
  CK(hipMalloc(&dHw, in.size() * 4));
  CK(hipMemcpy(dIn, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  kNarrow<BF6><<<(unsigned)((in.size() + 255) / 256), 256>>>(dIn, dHw, (int)in.size(), place[0] < 0 ? 0 : place[0]);
  std::vector<uint32_t> hw(in.size());
  CK(hipMemcpy(hw.data(), dHw, in.size() * 4, hipMemcpyDeviceToHost));
  int badN = 0;
  for (int i = 0; i < n; i++) {
    const uint32_t ref = narrowInt<MB, BIAS>(bitsOf(in[i]));
    if (hw[i] == ref) continue;
    if (badN++ < 12) std::printf("  narrow %08x (%g): converter %02x, integer form %02x\n", bitsOf(in[i]), in[i], hw[i], ref);
  }
  std::printf("%s narrow at scale 1.0: %d of %d differ from the integer form; NaN -> %02x, -NaN -> %02x\n", name, badN, n,
              hw[n], hw[n + 1]);
  CK(hipFree(dOrd));
  CK(hipFree(dDec));
  CK(hipFree(dIn));
  CK(hipFree(dHw));
  return 0;
}

int main() {
  if (probe<false, 3, 1>("fp6 (E2M3)")) return 1;
  return probe<true, 2, 3>("bf6 (E3M2)");
}
