// Shared pieces of the register-resident FFTs (stft.hip, istft.hip, tail_grad.hip): complex helpers, the W512 twiddle
// table access and the 16-point DFTs of the four-step 256 = 16 x 16 transform.
#pragma once
#include "device_common.h"

namespace sepvad {

constexpr int M256 = 256;

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 conjf2(float2 a) { return make_float2(a.x, -a.y); }

// Twiddle W512^idx, idx in [0, 512), from the half table tw = W512^0..255 (W512^(x+256) = -W512^x).
__device__ __forceinline__ float2 twid(const float2* tw, int idx) {
  const float2 w = tw[idx & 255];
  return idx < 256 ? w : make_float2(-w.x, -w.y);
}

// ------------------------------------------------------------------------------------------
// Register-resident 16-point DFTs for the four-step 256 = 16 x 16 transform (16 lanes per
// transform, 4 transforms per wave, one XOR-swizzled LDS transpose in the frame's own row).
// dft4: X_k = sum_n v_n W4^(nk), W4 = -i (forward) or +i (inverse), in place.
template <bool INV>
__device__ __forceinline__ void dft4(float2& v0, float2& v1, float2& v2, float2& v3) {
  const float2 s0 = cadd(v0, v2), d0 = csub(v0, v2), s1 = cadd(v1, v3);
  float2 d1 = csub(v1, v3);
  d1 = INV ? make_float2(-d1.y, d1.x) : make_float2(d1.y, -d1.x);
  v0 = cadd(s0, s1);
  v1 = cadd(d0, d1);
  v2 = csub(s0, s1);
  v3 = csub(d0, d1);
}
// slot of output k of dft16 (n = na + 4 nb in, k = kb + 4 ka out; the 4 x 4 index transpose is a renaming)
__host__ __device__ constexpr int d16(int k) { return (k >> 2) + 4 * (k & 3); }
// W16^p (forward e^{-2 pi i p / 16}, inverse conjugate) for p = na kb in {1, 2, 3, 4, 6, 9}; float
// roundings of the same cosines as the W512 table (tw[32 p])
template <bool INV>
__device__ __forceinline__ float2 w16(int p) {
  constexpr float C1 = 0.9238795042037964f, S1 = 0.3826834261417389f, R = 0.7071067690849304f;
  float c = 1.f, sn = 0.f;  // sn = sin(2 pi p / 16)
  switch (p) {
    case 1: c = C1; sn = S1; break;
    case 2: c = R; sn = R; break;
    case 3: c = S1; sn = C1; break;
    case 6: c = -R; sn = R; break;
    case 9: c = -C1; sn = -S1; break;
    default: break;
  }
  return make_float2(c, INV ? sn : -sn);
}
// dft16 after its first radix-4 pass (slot na + 4 kb holds that pass's output kb of input group na)
template <bool INV>
__device__ __forceinline__ void dft16_tail(float2 (&x)[16]) {
#pragma unroll
  for (int na = 1; na < 4; ++na)
#pragma unroll
    for (int kb = 1; kb < 4; ++kb) {
      const int p = na * kb;
      float2& v = x[na + 4 * kb];
      if (p == 4) v = INV ? make_float2(-v.y, v.x) : make_float2(v.y, -v.x);  // W16^4 = -+i
      else v = cmul(v, w16<INV>(p));
    }
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) dft4<INV>(x[4 * kb], x[4 * kb + 1], x[4 * kb + 2], x[4 * kb + 3]);  // slot ka + 4 kb
}
// 16-point DFT in place: x[n] in, X[k] out at slot d16(k)
template <bool INV>
__device__ __forceinline__ void dft16(float2 (&x)[16]) {
#pragma unroll
  for (int na = 0; na < 4; ++na) dft4<INV>(x[na], x[na + 4], x[na + 8], x[na + 12]);  // slot na + 4 kb
  dft16_tail<INV>(x);
}

// c ^ k computed where it is used (volatile: hipcc would otherwise hoist the 32 swizzled addresses of the
// transpose and hold them all in registers)
__device__ __forceinline__ int xor_late(int c, int k) {
  int r;
  asm volatile("v_xor_b32 %0, %1, %2" : "=v"(r) : "v"(c), "s"(k));
  return r;
}

__device__ __forceinline__ int mul_late(int c, int k) {
  int r;
  asm volatile("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(c), "s"(k));
  return r;
}

// Forward real 512-point transform of a frame whose samples are in registers (tail_grad.hip; the operations of
// stft.hip's rfft512_col after its loads, which keeps its own copy so that the forward's code is untouched): x[n1] = this
// lane's windowed column z[16 n1 + c] of the 256-point complex sequence z[m] = x[2m] + i x[2m+1] (16 lanes per frame,
// c = lane & 15). Step 1 DFT over n1, twiddle W256^(c k1), XOR-swizzled transpose through `row`, step 2 DFT over n2 ->
// Z[c + 16 k2], written to `row` in natural order for the split step (the caller syncs the wave before reading it).
__device__ __forceinline__ void rfft512_regs(float2 (&x)[16], float2* row, const float2* tw, int c) {
  dft16<false>(x);  // A[k1] at slot d16(k1)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k1 = 1; k1 < 16; ++k1) {  // W256^(c k1) = W512^(2 c k1)
    x[d16(k1)] = cmul(x[d16(k1)], twid(tw, mul_late(c, 2 * k1)));
    if (k1 % 4 == 3) {
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) row[16 * k1 + xor_late(c, k1)] = x[d16(k1)];
  wave_lds_sync();
#pragma unroll
  for (int n2 = 0; n2 < 16; ++n2) x[n2] = row[16 * c + xor_late(c, n2)];  // row k1 = c of the transpose
  wave_lds_sync();  // every lane's reads done before the natural-order writes below
  dft16<false>(x);  // Z[c + 16 k2] at slot d16(k2)
  float2* rc = row + c;
#pragma unroll
  for (int k2 = 0; k2 < 16; ++k2) rc[16 * k2] = x[d16(k2)];
}

}  // namespace sepvad
