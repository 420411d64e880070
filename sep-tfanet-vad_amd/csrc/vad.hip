// The VAD head's first layer (HBM-bound, no MFMA), up to the features k_istft_pair's VAD tail reads:
//   k_vad1          the whole VAD conv1_1 (257->4, k=5, pad 2) + bias + PReLU on the pre-sigmoid masks (or the
//                   masked magnitudes) with GroupNorm(1,4) partial statistics (model/model.py:158-161,173-176)
//   k_vad_feat      conv1_1 finished from the output head's tap products (k_tcn) + PReLU + BN_1, one workgroup
//                   per (utterance, speaker), T <= VF_ONE_T
//   k_vad_feat_rec  the same items un-normalised plus BN_1 partial records, T > VF_ONE_T
#include <type_traits>

#include "device_common.h"

namespace sepvad {

// VAD conv1_1 for VAD_ROWS = 32 frames of one (utterance, speaker). Thread = input channel c (the
// 257th channel is folded in after the lane reduction): the thread's 20 taps stay in registers, its
// R + 4 input samples (one coalesced 1 KB row read per frame, every load in flight at once) form a
// register window, and it accumulates all R x 4 outputs. The 128 partial outputs are reduced over
// the wave by recursive halving (lane L ends with outputs 2L, 2L+1: 126 lane exchanges), then over
// the 4 waves through LDS in fixed order (deterministic).
__device__ __forceinline__ float vad_in(const Vad1Args& a, int b, int s, int t, int c) {
  const int tc = min(max(t, 0), a.T - 1);
  const size_t row = (size_t)b * a.Tp + tc;
  float v = a.masks[row * MOUT_PAD + s * NBIN + c];
  if (a.masked_speakers) {
    const float2 X = a.X[row * NBIN + c];
    v = hypotf(X.x, X.y) * sigmoid_f(v);
  }
  return (t >= 0 && t < a.T) ? v : 0.f;  // conv zero padding (padding 2)
}

__global__ __launch_bounds__(256) void k_vad1(Vad1Args a) {
  constexpr int R = VAD_ROWS;
  constexpr int NV = 4 * R;   // outputs of the block, index 4 i + o
  __shared__ float part[4][NV];
  __shared__ float red[2 * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bs = blockIdx.x, b = bs >> 1, s = bs & 1;
  const int t0 = blockIdx.y * R;
  const int T = a.T;
  // diagnostics: slot 0 wall clock at entry, slots 1.. shader clock at the phase ends
  unsigned long long* const pr = a.probe ? a.probe + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 : nullptr;
  auto stamp = [&](int k) {
    if (pr && tid == 0) pr[k] = __builtin_amdgcn_s_memtime();
  };
  if (pr && tid == 0) pr[0] = wall_clock64();
  stamp(1);
  float m[R + 4];
#pragma unroll
  for (int r = 0; r < R + 4; ++r) m[r] = vad_in(a, b, s, t0 - 2 + r, tid);
  float w[4][5];
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int k = 0; k < 5; ++k) w[o][k] = a.w1[((size_t)o * NBIN + tid) * 5 + k];
  float acc[NV];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < 5; ++k) v = fmaf(w[o][k], m[i + k], v);
      acc[4 * i + o] = v;
    }
  stamp(2);
  // recursive halving over the lanes: a lane whose bit msk is clear keeps the lower half of its outputs,
  // its partner (bit set, same higher bits) the upper half. Bits 32 / 16: one v_permlane32/16_swap per pair
  // (the swap hands each lane its partner's item of the kept half: kept = own + swapped, no selects);
  // bits 8, 4: DPP row_mirror / row_half_mirror partners (lane i <-> 15 - i / 7 - i: opposite bit, same
  // higher bits), bits 2, 1: DPP quad_perm xor. Same index mapping as an xor butterfly (lane L ends with
  // outputs 2L, 2L+1); cdna_hip_programming.md T12/T21.
  // (inline asm: with this hipcc the __builtin_amdgcn_permlane{16,32}_swap pair result came back as the
  // same register twice, x + x, tools/probe_src/halving.hip; "s_nop 1" covers the VALU-write -> permlane
  // hazard, cdna_hip_programming.md T21)
#pragma unroll
  for (int j = 0; j < NV / 2; ++j) {
    float x = acc[j], y = acc[j + NV / 2];
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    acc[j] = x + y;
  }
#pragma unroll
  for (int j = 0; j < NV / 4; ++j) {
    float x = acc[j], y = acc[j + NV / 4];
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    acc[j] = x + y;
  }
  auto dpp_level = [&](auto CTRL, int msk, int n) {
    constexpr int C = decltype(CTRL)::value;
    const bool hi = (lane & msk) != 0;
#pragma unroll
    for (int j = 0; j < NV / 8; ++j) {
      if (j < n / 2) {
        const float send = hi ? acc[j] : acc[j + n / 2];
        const float keep = hi ? acc[j + n / 2] : acc[j];
        acc[j] = keep + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), C, 0xf, 0xf, false));
      }
    }
  };
  dpp_level(std::integral_constant<int, 0x140>{}, 8, NV / 4);  // row_mirror
  dpp_level(std::integral_constant<int, 0x141>{}, 4, NV / 8);  // row_half_mirror
  dpp_level(std::integral_constant<int, 0x4e>{}, 2, NV / 16);  // quad_perm [2,3,0,1]
  dpp_level(std::integral_constant<int, 0xb1>{}, 1, NV / 32);  // quad_perm [1,0,3,2]
  // channel 256 (the Nyquist bin): lane L of wave 0 adds its contribution to outputs 2L, 2L+1
  if (wave == 0) {
    const int i = lane >> 1, o0 = 2 * (lane & 1);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float x = vad_in(a, b, s, t0 + i - 2 + k, NBIN - 1);
      acc[0] = fmaf(a.w1[((size_t)o0 * NBIN + NBIN - 1) * 5 + k], x, acc[0]);
      acc[1] = fmaf(a.w1[((size_t)(o0 + 1) * NBIN + NBIN - 1) * 5 + k], x, acc[1]);
    }
  }
  stamp(3);
  part[wave][2 * lane] = acc[0];
  part[wave][2 * lane + 1] = acc[1];
  lds_sync();
  stamp(4);
  float st[2] = {0.f, 0.f};
  if (tid < NV) {
    const int ii = tid >> 2, o = tid & 3;
    const int t = t0 + ii;
    const float y = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    const float v = prelu_f(y + a.b1[o], a.alpha);
    a.vy[(((size_t)b * 2 + s) * 4 + o) * a.Tp + t] = (t < T) ? v : 0.f;
    if (t < T) { st[0] = v; st[1] = v * v; }
  }
  const int nrec = a.Tp / R;
  block_reduce_store<2>(st, red, a.out_rec + ((size_t)bs * nrec + blockIdx.y) * 2);
  stamp(5);
}

// k_vad_feat: the VAD head's conv1_1 finished from the output head's tap products (k_tcn) (fused schedule), one workgroup per
// (utterance, speaker): y[t][o] = sum_k P[t - 2 + k][4 k + o] (zero outside [0, T)), v = PReLU(y + b1),
// BN_1 = GroupNorm(1, 4) over [4, T] (block sums in double, wave order), feat = v * s[o] + h[o] for
// k_istft_pair's VAD tail (model/model.py:158-176).
// NI items (t, o) per thread: 4 for T <= 256, 16 for T <= VF_ONE_T (longer utterances: k_vad_feat_rec).
template <int NI>
__global__ __launch_bounds__(256) void k_vad_feat(VadFeatArgs a) {
  __shared__ float red[2 * 16];
  __shared__ double dacc[2];
  __shared__ float vs[4], vh[4];
  const int tid = threadIdx.x, bs = blockIdx.x, T = a.T;
  const float* P = a.vP + (size_t)bs * a.Tp * HEAD_VAD_N;
  float v[NI], st[2] = {0.f, 0.f};
#pragma unroll
  for (int it = 0; it < NI; ++it) {
    const int i = tid + 256 * it, t = i >> 2, o = i & 3;
    float y = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int tt = t - 2 + k;
      y += (i < 4 * T && tt >= 0 && tt < T) ? P[(size_t)tt * HEAD_VAD_N + 4 * k + o] : 0.f;
    }
    v[it] = prelu_f(y + a.b1[o], a.alpha);
    if (i < 4 * T) { st[0] += v[it]; st[1] += v[it] * v[it]; }
  }
  block_reduce_store<2>(st, red, dacc);
  lds_sync();
  if (tid < 4) {
    float mu, rs;
    gn_moments(dacc[0], dacc[1], 4.0 * T, a.eps, mu, rs);
    vs[tid] = rs * a.g[tid];
    vh[tid] = a.be[tid] - vs[tid] * mu;
  }
  lds_sync();
#pragma unroll
  for (int it = 0; it < NI; ++it) {
    const int i = tid + 256 * it, t = i >> 2, o = i & 3;
    if (i < 4 * T) a.feat[((size_t)bs * 4 + o) * a.Tp + t] = fmaf(v[it], vs[o], vh[o]);
  }
}

// k_vad_feat_rec: long utterances (T > VF_ONE_T). One workgroup per (utterance, speaker, VF_ROWS frames): the same
// conv1_1 + PReLU items as k_vad_feat, written un-normalised, and the chunk's BN_1 partial record {sum, sumsq} (wave
// sums, then the 4 wave totals in double in wave order); k_istft_pair sums the records in record order and applies BN_1
// (its vy_norm = 0 path). One workgroup per utterance and speaker took 35 us for two 60 s files (4 workgroups).
__global__ __launch_bounds__(256) void k_vad_feat_rec(VadFeatArgs a) {
  __shared__ float red[2 * 16];
  constexpr int NI = 4 * VF_ROWS / 256;
  const int tid = threadIdx.x, bs = blockIdx.x, T = a.T, t0 = blockIdx.y * VF_ROWS;
  const float* P = a.vP + (size_t)bs * a.Tp * HEAD_VAD_N;
  float st[2] = {0.f, 0.f};
#pragma unroll
  for (int it = 0; it < NI; ++it) {
    const int i = tid + 256 * it, t = t0 + (i >> 2), o = i & 3;
    float y = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int tt = t - 2 + k;
      y += (t < T && tt >= 0 && tt < T) ? P[(size_t)tt * HEAD_VAD_N + 4 * k + o] : 0.f;
    }
    const float v = prelu_f(y + a.b1[o], a.alpha);
    if (t < a.Tp) a.feat[((size_t)bs * 4 + o) * a.Tp + t] = t < T ? v : 0.f;
    if (t < T) { st[0] += v; st[1] += v * v; }
  }
  block_reduce_store<2>(st, red, a.out_rec + ((size_t)bs * vf_nrec(a.Tp) + blockIdx.y) * 2);
}

hipError_t launch_vad_feat(const VadFeatArgs& a, hipStream_t s) {
  if (a.T < 1 || a.T > 8192) return hipErrorInvalidValue;
  if (a.T > VF_ONE_T) {
    if (a.out_rec == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_vad_feat_rec, dim3(a.B * 2, vf_nrec(a.Tp)), dim3(256), 0, s, a);
  } else if (a.T <= 256) {
    hipLaunchKernelGGL(k_vad_feat<4>, dim3(a.B * 2), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(k_vad_feat<16>, dim3(a.B * 2), dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_vad1(const Vad1Args& a, hipStream_t s) {
  if (a.Tp % VAD_ROWS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vad1, dim3(a.B * 2, a.Tp / VAD_ROWS), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sepvad
