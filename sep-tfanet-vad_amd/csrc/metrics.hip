// Scale-invariant SDR on the device (reference model/combined_loss.py:16-56 calc_sisdr, identical to
// model/metric.py:61-101 scale_invariant_signal_distortion_ratio): for each row pair r,
//   p = P[pidx[r]], t = Tg[tidx[r]] (rows of N samples; identity indices when null), optional zero mean,
//   alpha = (<p,t> + eps) / (<t,t> + eps), ts = alpha t, e = ts - p,
//   si_sdr = 10 log10((<ts,ts> + eps) / (<e,e> + eps)),  eps = float32 machine epsilon.
// One workgroup per pair streams both rows once and accumulates five moments in double; the zero-mean and scaled
// terms follow in closed form: <p',t'> = <p,t> - N mp mt, <t',t'> = <t,t> - N mt^2,
// <e,e> = alpha^2 <t',t'> - 2 alpha <p',t'> + <p',p'>.
//
// Conditioning. The closed form loses (mean^2 / variance) (signal / residual) of the moments' precision: taken on
// the raw rows, a DC of 100 standard deviations at a 71 .. 78 dB residual moved the result by 3.1e-3 dB at N = 32 000
// and by 0.14 dB at N = 2 000 000 (1000 standard deviations: 0.35 dB and 5.8 dB; measured), as much as or more than
// the float32 reference it replaces. So with zero_mean the moments are those of p - p[0] and t - t[0]: the centred moments do not depend on
// the shift, the subtraction of two floats is exact in double, and a row's own first sample leaves a mean of the
// order of its standard deviation. Without zero_mean nothing is shifted (the raw moments are what the formula
// asks for; its error stays below 1e-5 dB up to 80 dB). A thread adds 16 samples' terms on their own before they
// join its running sum: squares of shifted floats share their low bits, and a running sum of thousands of them
// rounds with a bias (2e-4 dB at N = 2 000 000, by emulation) that sums of 16 do not have. Measured table: DESIGN.md section 12,
// tests/test_gpu_score_regimes.py.
//
// Fixed-order reductions: bitwise reproducible, and independent of the rows' alignment (the float4 and the scalar
// path give each thread the same samples in the same order). HBM-bound (8 N bytes per pair).
#include "device_common.h"

namespace sepvad {

constexpr int SD_THREADS = 256;

// explicit fma: the same rounding in both paths whatever the compiler contracts
__device__ __forceinline__ void sd_acc(double (&s)[5], float pf, float tf, double cp, double ct) {
  const double x = (double)pf - cp, y = (double)tf - ct;
  s[0] += x; s[1] += y;
  s[2] = fma(x, x, s[2]); s[3] = fma(y, y, s[3]); s[4] = fma(x, y, s[4]);
}

// Thread q takes the float4 groups q, q + 256, ... of the row, four at a time into sums of their own.
template <bool VEC>
__device__ __forceinline__ void sd_row(const float* p, const float* t, long long N, double cp, double ct,
                                       double (&s)[5]) {
  const long long n4 = N / 4;
  for (long long q0 = threadIdx.x; q0 < n4; q0 += 4 * SD_THREADS) {
    float pa[4][4], ta[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long q = q0 + u * SD_THREADS;
      if (q < n4) { load4<VEC>(p, q, pa[u]); load4<VEC>(t, q, ta[u]); }
    }
    double c[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (q0 + u * SD_THREADS < n4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sd_acc(c, pa[u][k], ta[u][k], cp, ct);
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] += c[k];
  }
  const long long i = n4 * 4 + threadIdx.x;  // the last N % 4 samples: one each for threads 0 .. 2
  if (i < N) sd_acc(s, p[i], t[i], cp, ct);
}

// The five double moments {sum x, sum y, <x,x>, <y,y>, <x,y>} of pair r, x = p - p[0] and y = t - t[0] with
// zero_mean, the rows themselves without; true on thread 0 only, which then holds them in m.
__device__ __forceinline__ bool pair_moments(const SiSdrArgs& a, double (&m)[5]) {
  __shared__ double red[5 * 16];
  const int r = blockIdx.x;
  const long long pr = a.pidx ? a.pidx[r] : r, tr = a.tidx ? a.tidx[r] : r;
  const float* p = a.P + pr * a.p_ld;
  const float* t = a.Tg + tr * a.t_ld;
  const double cp = a.zero_mean ? (double)p[0] : 0.0, ct = a.zero_mean ? (double)t[0] : 0.0;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(t)) & 15) == 0;
  if (vec) sd_row<true>(p, t, a.N, cp, ct, s);
  else sd_row<false>(p, t, a.N, cp, ct, s);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double v = wave_sum(s[k]);
    if (l == 0) red[k * 16 + w] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double v = 0.0;
    for (int i = 0; i < SD_THREADS / 64; ++i) v += red[k * 16 + i];
    m[k] = v;
  }
  return true;
}

__global__ __launch_bounds__(SD_THREADS) void k_si_sdr(SiSdrArgs a) {
  double m[5];
  if (pair_moments(a, m)) {
    const int r = blockIdx.x;
    const long long N = a.N;
    const double eps = 1.1920928955078125e-07;  // torch.finfo(torch.float32).eps
    const double Nd = (double)N;
    double pt = m[4], tt = m[3], pp = m[2];
    if (a.zero_mean) {
      const double mp = m[0] / Nd, mt = m[1] / Nd;
      pt -= Nd * mp * mt;
      tt -= Nd * mt * mt;
      pp -= Nd * mp * mp;
    }
    const double alpha = (pt + eps) / (tt + eps);
    const double sig = alpha * alpha * tt;
    double noise = sig - 2.0 * alpha * pt + pp;
    if (noise < 0.0) noise = 0.0;
    a.out[r] = (float)(10.0 * log10((sig + eps) / (noise + eps)));
  }
}

// Signal-to-noise ratio (reference model/metric.py:104-143 signal_noise_ratio): optional zero mean, noise = t - p,
//   snr = 10 log10((<t,t> + eps) / (<noise,noise> + eps)),  <noise,noise> = <t',t'> - 2 <p',t'> + <p',p'>.
__global__ __launch_bounds__(SD_THREADS) void k_snr(SiSdrArgs a) {
  double m[5];
  if (pair_moments(a, m)) {
    const double eps = 1.1920928955078125e-07;  // torch.finfo(torch.float32).eps
    const double Nd = (double)a.N;
    double pt = m[4], tt = m[3], pp = m[2];
    if (a.zero_mean) {
      const double mp = m[0] / Nd, mt = m[1] / Nd;
      pt -= Nd * mp * mt;
      tt -= Nd * mt * mt;
      pp -= Nd * mp * mp;
    }
    double noise = tt - 2.0 * pt + pp;
    if (noise < 0.0) noise = 0.0;
    a.out[blockIdx.x] = (float)(10.0 * log10((tt + eps) / (noise + eps)));
  }
}

// VAD accuracy (reference model/metric.py:163-177 Accuracy_Vad): labels = preds > 0.5 (not >=; NaN kept),
// written back into preds as the reference's in-place masking does (when in_place), then the fraction of
// labels equal to the targets over everything and per speaker. One workgroup: integer counts, exact.
__global__ __launch_bounds__(1024) void k_vad_acc(VadAccArgs a) {
  __shared__ unsigned cnt[1024 / 64][VACC_MAX_S];
  unsigned c[VACC_MAX_S];
#pragma unroll
  for (int s = 0; s < VACC_MAX_S; ++s) c[s] = 0;
  const long long n = (long long)a.B * a.S * a.T;
  for (long long i = threadIdx.x; i < n; i += 1024) {
    const int s = (int)((i / a.T) % a.S);
    float p = a.preds[i];
    p = p > 0.5f ? 1.f : (p <= 0.5f ? 0.f : p);
    if (a.in_place) a.preds[i] = p;
    const unsigned hit = p == a.targets[i] ? 1u : 0u;
#pragma unroll
    for (int q = 0; q < VACC_MAX_S; ++q) c[q] += q == s ? hit : 0u;
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < VACC_MAX_S; ++q) {
    unsigned v = c[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (l == 0) cnt[w][q] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tot = 0;
    for (int q = 0; q < a.S; ++q) {
      unsigned long long cq = 0;
      for (int ww = 0; ww < 1024 / 64; ++ww) cq += cnt[ww][q];
      tot += cq;
      a.out[1 + q] = (float)cq / (float)((long long)a.B * a.T);  // torch: int64 sum / int -> float32
    }
    a.out[0] = (float)tot / (float)n;
  }
}

hipError_t launch_vad_acc(const VadAccArgs& a, hipStream_t s) {
  if (a.B < 1 || a.S < 1 || a.S > VACC_MAX_S || a.T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vad_acc, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_si_sdr(const SiSdrArgs& a, hipStream_t s) {
  if (a.R < 1 || a.N < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_si_sdr, dim3(a.R), dim3(SD_THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_snr(const SiSdrArgs& a, hipStream_t s) {
  if (a.R < 1 || a.N < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_snr, dim3(a.R), dim3(SD_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace sepvad
