// The training criterion's backward (trainer/trainer.py:57-63 calls the criterion and then loss.backward()): the
// gradients of CombinedLoss (model/combined_loss.py:93-138) over PITLossWrapper(PairwiseNegSDR(...), "pw_mtx")
// (model/sdr.py:48-86) with respect to the separated signals and the VAD track. The forward is eval.hip's, unchanged
// (launch_eval_separation, launch_eval_vad); this file adds what a backward needs.
//
// Separation. For estimate row e paired with target row t (primes: the centred rows when zero_mean), with
//   tt = <t',t'>, pt = <e',t'>, pp = <e',e'>, E = tt + EPS, a = pt / E,
//   sisdr: P = a^2 tt, n = e' - a t';   sdsdr: P = a^2 tt, n = e' - t';   snr: P = tt, n = e' - t',
//   Nn = <n,n>, D = Nn + EPS, r = P / D, loss = -(10 / ln 10) ln(r + EPS) (take_log) or -r,
// the exact derivative is a combination of the two rows:
//   d loss / d e = c_t t' + c_n n,     c_n = -L' 2 P / D^2,   L' = -(10 / ln 10) / (r + EPS) or -1,
//   sisdr: c_t = L' (2 a / (E D)) (tt + EPS P / D)    (d Nn / d e' = 2 n - 2 <n,t'> t' / E, and <n,t'> = a EPS),
//   sdsdr: c_t = L' 2 a tt / (E D),                    snr: c_t = 0.
// Both rows are zero-mean when zero_mean, so the centring's own Jacobian takes nothing away. Every term keeps the
// reference's EPS: on silence (P = 0, a = 0) the coefficients are finite zeros where the EPS-free form t / pt - n / Nn
// divides by zero. The coefficients follow from the 16 moments k_eval_moments leaves in scratch: k_crit_coef adds an
// utterance's partials in chunk order (as ev_finish) and writes CRIT_COEF doubles per estimate row into a buffer the
// caller owns; the backward reads nothing else, so the scratch may be reused between forward and backward.
//
// Conditioning. Nn = pp - 2 a pt + a^2 tt cancels by the SDR: c_n carries 2^-53 10^(SDR / 10) of relative error, c_t
// t' + c_n n is evaluated per sample in double from the float32 samples and rounded once. Measured table: DESIGN.md
// section 14, tests/grad_cases.py.
//
// No atomics, every sum in a fixed order, the float4 and the scalar path evaluate cg_one on the same samples: results
// are bitwise reproducible, independent of the rows' alignment and strides, and utterance b's gradient times B
// depends on its own rows only.
#include "eval_common.h"

namespace sepvad {

constexpr int CG_THREADS = 256;
static_assert(CG_CHUNK == 4 * CG_THREADS, "k_crit_grad_sep: one float4 of each row per thread");
constexpr int CC_CT = 0, CC_CN = 1, CC_A = 2, CC_ME = 3, CC_MT = 4, CC_J = 5;
static_assert(CC_J + 1 == SEPVAD_CRIT_COEF && CRIT_COEF == SEPVAD_CRIT_COEF, "coef layout (include/sepvad.h)");

// One wave per utterance. Lanes 0..15 add one moment each over the chunks in chunk order (ev_finish's order); lanes 0
// and 1 evaluate estimate row i = lane against the target j the permutation pairs it with.
__global__ __launch_bounds__(64) void k_crit_coef(CritCoefArgs a) {
  const int b = blockIdx.x, l = threadIdx.x;
  const float* est_b = a.est + (long long)b * 2 * a.est_ld;
  const float* tgt_b = a.tgt + (long long)b * 2 * a.tgt_ld;
  // the moments are those of the rows less their first sample (eval.hip): lane r < 4 fetches the shift of row r
  double piv = 0.0;
  if (l < 2) piv = (double)est_b[(long long)l * a.est_ld];
  else if (l < 4) piv = (double)tgt_b[(long long)(l - 2) * a.tgt_ld];
  double v = 0.0;
  if (l < EV_MOM) {
    const double* p = a.partial + (long long)b * a.nchunk * EV_MOM + l;
    int c = 0;
    for (; c + EVF_BATCH <= a.nchunk; c += EVF_BATCH) {
      double t[EVF_BATCH];
#pragma unroll
      for (int u = 0; u < EVF_BATCH; ++u) t[u] = p[(long long)(c + u) * EV_MOM];
#pragma unroll
      for (int u = 0; u < EVF_BATCH; ++u) v += t[u];
    }
    for (; c < a.nchunk; ++c) v += p[(long long)c * EV_MOM];
  }
  const int i = l & 1;
  // perm[b][j] is the estimate assigned to target j; of two sources a permutation is its own inverse
  const int j = (int)(a.perm[(long long)b * 2 + i] & 1);
  const double sp = __shfl(v, EVM_S + i), st = __shfl(v, EVM_S + 2 + j);
  double qp = __shfl(v, EVM_Q + i), qt = __shfl(v, EVM_Q + 2 + j);
  double xy = __shfl(v, EVM_ET + 2 * i + j);
  const double cp = __shfl(piv, i), ct = __shfl(piv, 2 + j);
  if (l >= 2) return;
  const int zm = a.zero_mean;
  const double Nd = (double)a.N, eps = a.eps;
  if (!zm) {
    qp = ev_raw(qp, sp, sp, cp, cp, Nd);
    qt = ev_raw(qt, st, st, ct, ct, Nd);
    xy = ev_raw(xy, sp, st, cp, ct, Nd);
  }
  const double pp = ev_energy(qp, sp, Nd, zm), tt = ev_energy(qt, st, Nd, zm), pt = ev_cen(xy, sp, st, Nd, zm);
  const double E = tt + eps;
  const double al = a.sdr_type == SEPVAD_SDR_SNR ? 1.0 : pt / E;
  const double P = al * al * tt;
  double noise = a.sdr_type == SEPVAD_SDR_SISDR ? pp - 2.0 * al * pt + P : pp - 2.0 * pt + tt;
  if (noise < 0.0) noise = 0.0;
  const double D = noise + eps;
  const double r = P / D;
  const double dl = a.take_log ? -4.3429448190325182765 / (r + eps) : -1.0;  // 10 / ln 10
  double c_t = 0.0;
  if (a.sdr_type == SEPVAD_SDR_SISDR) c_t = dl * (2.0 * al / (E * D)) * (tt + eps * P / D);
  else if (a.sdr_type == SEPVAD_SDR_SDSDR) c_t = dl * 2.0 * al * tt / (E * D);
  double* o = a.coef + ((long long)b * 2 + i) * CRIT_COEF;
  o[CC_CT] = c_t;
  o[CC_CN] = -dl * 2.0 * P / (D * D);
  o[CC_A] = a.sdr_type == SEPVAD_SDR_SISDR ? al : 1.0;
  o[CC_ME] = zm ? cp + sp / Nd : 0.0;
  o[CC_MT] = zm ? ct + st / Nd : 0.0;
  o[CC_J] = (double)j;
}

// one sample of one estimate row: explicit fma, the same rounding in both paths whatever the compiler contracts
__device__ __forceinline__ float cg_one(float e, float t, double ct, double cn, double al, double me, double mt) {
  const double tp = (double)t - mt;
  const double n = fma(-al, tp, (double)e - me);
  return (float)fma(cn, n, ct * tp);
}

template <bool VEC>
__device__ __forceinline__ void cg_chunk(const float* e0, const float* e1, const float* t0, const float* t1, float* g0,
                                         float* g1, int len, const double (&k0)[CRIT_COEF],
                                         const double (&k1)[CRIT_COEF]) {
  const bool j0 = k0[CC_J] != 0.0, j1 = k1[CC_J] != 0.0;
  const int n4 = len / 4, q = threadIdx.x;
  if (q < n4) {
    float a[4], b[4], c[4], d[4];
    ev_load4<VEC>(e0, q, a); ev_load4<VEC>(e1, q, b); ev_load4<VEC>(t0, q, c); ev_load4<VEC>(t1, q, d);
    float x[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[k] = cg_one(a[k], j0 ? d[k] : c[k], k0[CC_CT], k0[CC_CN], k0[CC_A], k0[CC_ME], k0[CC_MT]);
      y[k] = cg_one(b[k], j1 ? d[k] : c[k], k1[CC_CT], k1[CC_CN], k1[CC_A], k1[CC_ME], k1[CC_MT]);
    }
    if (VEC) {
      reinterpret_cast<float4*>(g0)[q] = make_float4(x[0], x[1], x[2], x[3]);
      reinterpret_cast<float4*>(g1)[q] = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) { g0[4 * q + k] = x[k]; g1[4 * q + k] = y[k]; }
    }
  }
  const int i = n4 * 4 + threadIdx.x;  // the chunk's last len % 4 samples: one each for threads 0 .. 2
  if (i < len) {
    g0[i] = cg_one(e0[i], j0 ? t1[i] : t0[i], k0[CC_CT], k0[CC_CN], k0[CC_A], k0[CC_ME], k0[CC_MT]);
    g1[i] = cg_one(e1[i], j1 ? t1[i] : t0[i], k1[CC_CT], k1[CC_CN], k1[CC_A], k1[CC_ME], k1[CC_MT]);
  }
}

// grid B * nchunk: workgroup b * nchunk + c writes samples [c CG_CHUNK, min(N, (c + 1) CG_CHUNK)) of both gradient
// rows of utterance b: grad[b][i][n] = g_sep / (2 B) (c_t t'_j[n] + c_n (e'_i[n] - a t'_j[n])). Four float4 loads and
// two float4 stores per thread, 16 B read and 8 B written per sample of the utterance.
__global__ __launch_bounds__(CG_THREADS) void k_crit_grad_sep(CritGradArgs a) {
  const int b = blockIdx.x / a.nchunk, c = blockIdx.x % a.nchunk;
  const long long off = (long long)c * CG_CHUNK;
  const long long left = a.N - off;
  const int len = left < CG_CHUNK ? (int)left : CG_CHUNK;
  const float* e0 = a.est + (long long)b * 2 * a.est_ld + off;
  const float* t0 = a.tgt + (long long)b * 2 * a.tgt_ld + off;
  float* g0 = a.grad_est + (long long)b * 2 * a.grad_ld + off;
  const float* e1 = e0 + a.est_ld;
  const float* t1 = t0 + a.tgt_ld;
  float* g1 = g0 + a.grad_ld;
  // the mean over the batch and over the two pairs of an utterance (pit_wrapper.py:287-312), times the upstream
  // gradient; a power of two of B scales every product exactly
  const double G = (double)a.g_sep[0] / (2.0 * (double)a.B);
  const double* kc = a.coef + (long long)b * 2 * CRIT_COEF;
  double k0[CRIT_COEF], k1[CRIT_COEF];
#pragma unroll
  for (int k = 0; k < CRIT_COEF; ++k) { k0[k] = kc[k]; k1[k] = kc[CRIT_COEF + k]; }
  k0[CC_CT] *= G; k0[CC_CN] *= G; k1[CC_CT] *= G; k1[CC_CN] *= G;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(e0) | reinterpret_cast<uintptr_t>(e1) |
                         reinterpret_cast<uintptr_t>(t0) | reinterpret_cast<uintptr_t>(t1) |
                         reinterpret_cast<uintptr_t>(g0) | reinterpret_cast<uintptr_t>(g1);
  if ((bits & 15) == 0) cg_chunk<true>(e0, e1, t0, t1, g0, g1, len, k0, k1);
  else cg_chunk<false>(e0, e1, t0, t1, g0, g1, len, k0, k1);
}

// One thread per (b, s, t): the derivative of the weighted BCE (combined_loss.py:130-137) of pred[b][s] =
// vad[b][perm[b][s]] against labels[b][s], written to the row it was read from. perm[b] is a permutation, so every
// element of grad_vad is written once. The clamp is binary_cross_entropy_backward's float32 1e-12.
__global__ __launch_bounds__(CG_THREADS) void k_crit_grad_vad(CritGradArgs a) {
  const long long idx = (long long)blockIdx.x * CG_THREADS + threadIdx.x;
  const long long total = 2LL * a.B * a.T;
  if (idx >= total) return;
  const long long bs = idx / a.T;
  const int t = (int)(idx % a.T);
  const int src = a.perm ? (int)(a.perm[bs] & 1) : (int)(bs & 1);
  const long long row = (bs & ~1LL) + src;
  const double p = (double)a.vad[row * a.T + t];
  double y = (double)a.labels[bs * a.T + t];
  if (y == 2.0) y = 1.0;
  const double w = y * 0.36 + 0.64 * (1.0 - y);
  const double den = fmax(p * (1.0 - p), (double)1e-12f);
  const double G = (double)a.g_vad[0] / (double)a.B;
  a.grad_vad[row * a.T + t] = (float)(G * (w * (p - y) / den));
}

hipError_t launch_crit_coef(const CritCoefArgs& a, hipStream_t s) {
  if (a.B < 1 || a.N < 1 || a.nchunk < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_crit_coef, dim3(a.B), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_crit_grad(const CritGradArgs& a, hipStream_t s) {
  if (a.B < 1) return hipErrorInvalidValue;
  if (a.est) {
    if (a.N < 1 || a.nchunk < 1 || (long long)a.B * a.nchunk > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_crit_grad_sep, dim3((unsigned)(a.B * a.nchunk)), dim3(CG_THREADS), 0, s, a);
  }
  if (a.vad) {
    const long long nblk = (2LL * a.B * a.T + CG_THREADS - 1) / CG_THREADS;
    if (a.T < 1 || nblk > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_crit_grad_vad, dim3((unsigned)nblk), dim3(CG_THREADS), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace sepvad
