// Device functions of the evaluation criterion (eval.hip) that the streaming evaluation (stream_eval.hip) shares:
// the 16 shifted moments of one EV_CHUNK of an utterance's five rows, and the closed forms, permutation choice and
// score sheet of one utterance from its summed moments. One body for both callers: a window scored by
// stream_eval.hip has the bits sepvad_eval_separation gives for that window and target slice.
#pragma once
#include "device_common.h"
#include "../../include/sepvad.h"

namespace sepvad {

constexpr int EV_THREADS = 256;
constexpr int EVM_S = 0, EVM_Q = 5, EVM_ET = 10, EVM_MT = 14;
static_assert(EV_CHUNK % 4 == 0, "chunk bases must keep a row's 16-byte alignment");

// load4 of a nullable row (null: zeros)
template <bool VEC>
__device__ __forceinline__ void ev_load4(const float* p, int q, float (&v)[4]) {
  if (!p) v[0] = v[1] = v[2] = v[3] = 0.f;
  else load4<VEC>(p, q, v);
}

// explicit fma: the same rounding in both paths whatever the compiler contracts; c: the five rows' first samples
__device__ __forceinline__ void ev_acc(double (&s)[EV_MOM], const double (&c)[5], float e0, float e1, float t0, float t1,
                                       float m) {
  const double x0 = (double)e0 - c[0], x1 = (double)e1 - c[1], y0 = (double)t0 - c[2], y1 = (double)t1 - c[3];
  const double z = (double)m - c[4];
  s[EVM_S + 0] += x0; s[EVM_S + 1] += x1; s[EVM_S + 2] += y0; s[EVM_S + 3] += y1; s[EVM_S + 4] += z;
  s[EVM_Q + 0] = fma(x0, x0, s[EVM_Q + 0]); s[EVM_Q + 1] = fma(x1, x1, s[EVM_Q + 1]);
  s[EVM_Q + 2] = fma(y0, y0, s[EVM_Q + 2]); s[EVM_Q + 3] = fma(y1, y1, s[EVM_Q + 3]);
  s[EVM_Q + 4] = fma(z, z, s[EVM_Q + 4]);
  s[EVM_ET + 0] = fma(x0, y0, s[EVM_ET + 0]); s[EVM_ET + 1] = fma(x0, y1, s[EVM_ET + 1]);
  s[EVM_ET + 2] = fma(x1, y0, s[EVM_ET + 2]); s[EVM_ET + 3] = fma(x1, y1, s[EVM_ET + 3]);
  s[EVM_MT + 0] = fma(z, y0, s[EVM_MT + 0]); s[EVM_MT + 1] = fma(z, y1, s[EVM_MT + 1]);
}

template <bool VEC>
__device__ __forceinline__ void ev_chunk(const float* e0, const float* e1, const float* t0, const float* t1,
                                         const float* m, int len, const double (&c)[5], double (&s)[EV_MOM]) {
  const int n4 = len / 4;
  for (int q = threadIdx.x; q < n4; q += EV_THREADS) {
    float a[4], b[4], g[4], d[4], z[4];
    ev_load4<VEC>(e0, q, a); ev_load4<VEC>(e1, q, b); ev_load4<VEC>(t0, q, g); ev_load4<VEC>(t1, q, d);
    ev_load4<VEC>(m, q, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) ev_acc(s, c, a[k], b[k], g[k], d[k], z[k]);
  }
  const int i = n4 * 4 + threadIdx.x;  // the chunk's last len % 4 samples: one each for threads 0 .. 2
  if (i < len) ev_acc(s, c, e0[i], e1[i], t0[i], t1[i], m ? m[i] : 0.f);
}

// One workgroup (EV_THREADS): the moments of samples [c EV_CHUNK, min(N, (c + 1) EV_CHUNK)) of the utterance whose
// rows start at e0, e1 = e0 + est_ld, t0, t1 = t0 + tgt_ld and m (nullable), stored to out[EV_MOM].
// red: EV_MOM * (EV_THREADS / 64) doubles of LDS.
__device__ __forceinline__ void ev_block_moments(const float* e0, const float* e1, const float* t0, const float* t1,
                                                 const float* m, long long N, int c, double* red, double* out) {
  const long long off = (long long)c * EV_CHUNK;
  const long long left = N - off;
  const int len = left < EV_CHUNK ? (int)left : EV_CHUNK;
  e0 += off; e1 += off; t0 += off; t1 += off;
  if (m) m += off;
  // the rows' first samples (sample 0 of the utterance, whatever the chunk); a missing mixture is a row of zeros
  const double piv[5] = {(double)e0[-off], (double)e1[-off], (double)t0[-off], (double)t1[-off],
                         m ? (double)m[-off] : 0.0};
  double s[EV_MOM];
#pragma unroll
  for (int k = 0; k < EV_MOM; ++k) s[k] = 0.0;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(e0) | reinterpret_cast<uintptr_t>(e1) |
                         reinterpret_cast<uintptr_t>(t0) | reinterpret_cast<uintptr_t>(t1) |
                         reinterpret_cast<uintptr_t>(m);
  if ((bits & 15) == 0) ev_chunk<true>(e0, e1, t0, t1, m, len, piv, s);
  else ev_chunk<false>(e0, e1, t0, t1, m, len, piv, s);
  block_sums_store<EV_MOM, EV_THREADS / 64>(s, red, out);
}

// <x, y> of the rows themselves from the moments of x - cx and y - cy. One expression for <p,p>, <t,t> and <p,t>:
// identical rows keep the three equal to the bit.
__device__ __forceinline__ double ev_raw(double xy, double sx, double sy, double cx, double cy, double Nd) {
  return fma(cx, sy, fma(cy, sx, fma(Nd * cx, cy, xy)));
}

// <x, y> of the zero-mean rows from the moments (of the shifted rows: the shift does not change it)
__device__ __forceinline__ double ev_cen(double xy, double sx, double sy, double Nd, int zero_mean) {
  return zero_mean ? xy - sx * sy / Nd : xy;
}
__device__ __forceinline__ double ev_energy(double xx, double sx, double Nd, int zero_mean) {
  const double v = ev_cen(xx, sx, sx, Nd, zero_mean);
  return v < 0.0 ? 0.0 : v;
}

// One number of an utterance from <p,p>, <t,t>, <p,t> of an estimate (or the mixture) p and a target t. Every kind
// ends in the same num / den and log10, so the 16 lanes that hold one job each diverge only over cheap arithmetic.
//   kind SEPVAD_SDR_*: one cell of PairwiseNegSDR (model/sdr.py:64-86) with the reference's EPS placement;
//   EVK_SI / EVK_SNR:  k_si_sdr / k_snr (metrics.hip), eps = float32 epsilon.
constexpr int EVK_SI = 3, EVK_SNR = 4;
__device__ __forceinline__ double ev_score(int kind, double pp, double tt, double pt, int take_log, double eps) {
  const double e32 = 1.1920928955078125e-07;  // torch.finfo(torch.float32).eps
  double num, den, add, scale;
  if (kind <= SEPVAD_SDR_SNR) {
    const double al = kind == SEPVAD_SDR_SNR ? 1.0 : pt / (tt + eps);
    const double proj = al * al * tt;
    double noise = kind == SEPVAD_SDR_SISDR ? pp - 2.0 * al * pt + proj : pp - 2.0 * pt + tt;
    if (noise < 0.0) noise = 0.0;
    num = proj; den = noise + eps; add = eps; scale = -10.0;
  } else {
    const double alpha = kind == EVK_SI ? (pt + e32) / (tt + e32) : 1.0;
    const double sig = alpha * alpha * tt;
    double noise = sig - 2.0 * alpha * pt + pp;
    if (noise < 0.0) noise = 0.0;
    num = sig + e32; den = noise + e32; add = 0.0; scale = 10.0;
    take_log = 1;
  }
  const double val = num / den;
  return take_log ? scale * log10(val + add) : -val;
}

// metrics.py permutation_invariant_si_sdr for two speakers on the float32 metric matrix m[t][p]: the mean over the
// targets of either assignment (float32), the first maximum wins
__device__ __forceinline__ float ev_pit_max(float m00, float m01, float m10, float m11) {
  const float id = (m00 + m11) * 0.5f, sw = (m01 + m10) * 0.5f;
  return sw > id ? sw : id;
}

constexpr int EVF_BATCH = 16;  // chunk partials loaded before they are added (the adds stay in chunk order)

// One wave: utterance b of a (outputs and partials at index b) whose rows start at est_b ([2] rows of stride
// a.est_ld), tgt_b ([2] rows of stride a.tgt_ld) and mix_b (nullable). Lanes 0..15 add one moment each over the
// chunks in chunk order; then 16 lanes evaluate one number each (job below) from moments fetched from the lanes that
// hold them, and lane 0 chooses and stores.
__device__ __forceinline__ void ev_finish(const EvalSepArgs& a, int b, const float* est_b, const float* tgt_b,
                                          const float* mix_b) {
  const int l = threadIdx.x;
  // zero_mean = 0 takes the shift of the moments out again: lane r < 5 fetches the first sample of row r (issued
  // ahead of the partials; with zero_mean nothing needs it)
  double piv = 0.0;
  if (!a.zero_mean) {
    if (l < 2) piv = (double)est_b[(long long)l * a.est_ld];
    else if (l < 4) piv = (double)tgt_b[(long long)(l - 2) * a.tgt_ld];
    else if (l == 4 && mix_b) piv = (double)mix_b[0];
  }
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
  // job 0..3: pw[i][j] of the loss at 2 i + j; 4..7: SI-SDR of estimate p against target t at 4 + 2 t + p; 8..11: the
  // SNR of the same pairs; 12, 13: SI-SDR of the mixture against target t; 14, 15: its SNR. The sheet is zero-mean.
  const int job = l & 15;
  int kind, row, t;
  if (job < 4) { kind = a.sdr_type; row = job >> 1; t = job & 1; }
  else if (job < 12) { kind = job < 8 ? EVK_SI : EVK_SNR; row = job & 1; t = (job >> 1) & 1; }
  else { kind = job < 14 ? EVK_SI : EVK_SNR; row = 4; t = job & 1; }
  const int zm = job < 4 ? a.zero_mean : 1;
  const double Nd = (double)a.N;
  const double sp = __shfl(v, EVM_S + row), st = __shfl(v, EVM_S + 2 + t);
  double qp = __shfl(v, EVM_Q + row), qt = __shfl(v, EVM_Q + 2 + t);
  double xy = __shfl(v, row == 4 ? EVM_MT + t : EVM_ET + 2 * row + t);
  const double cp = __shfl(piv, row), ct = __shfl(piv, 2 + t);
  if (!zm) {
    qp = ev_raw(qp, sp, sp, cp, cp, Nd);
    qt = ev_raw(qt, st, st, ct, ct, Nd);
    xy = ev_raw(xy, sp, st, cp, ct, Nd);
  }
  const float r = (float)ev_score(kind, ev_energy(qp, sp, Nd, zm), ev_energy(qt, st, Nd, zm), ev_cen(xy, sp, st, Nd, zm),
                                  a.take_log, a.eps);
  float s[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) s[k] = __shfl(r, k);
  if (l != 0) return;
  // the loss's pairwise matrix pw[i][j]: estimate i against target j
  float pw[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      pw[i][j] = s[2 * i + j];
      a.pw[(long long)b * 4 + 2 * i + j] = pw[i][j];
    }
  // find_best_perm_factorial on the float32 matrix: permutations in itertools order, torch.min keeps the first minimum
  const float loss_id = (pw[0][0] + pw[1][1]) / 2.f, loss_sw = (pw[1][0] + pw[0][1]) / 2.f;
  const bool swap = loss_sw < loss_id;
  const float min_loss = swap ? loss_sw : loss_id;
  a.min_loss[b] = min_loss;
  a.perm[(long long)b * 2 + 0] = swap ? 1 : 0;
  a.perm[(long long)b * 2 + 1] = swap ? 0 : 1;
  // the score sheet: zero-mean SI-SDR / SNR of estimate p (or the mixture) against target t, float32 as the metric
  // entries return them
  const float si[2][2] = {{s[4], s[5]}, {s[6], s[7]}}, sn[2][2] = {{s[8], s[9]}, {s[10], s[11]}};  // [t][p]
  const float si_mix[2] = {s[12], s[13]}, sn_mix[2] = {s[14], s[15]};
  const float pit_si = ev_pit_max(si[0][0], si[0][1], si[1][0], si[1][1]);
  const float pit_sn = ev_pit_max(sn[0][0], sn[0][1], sn[1][0], sn[1][1]);
  if (a.sheet) {
    float* o = a.sheet + (long long)b * SEPVAD_EV_COLS;
    o[SEPVAD_EV_SISDR0] = swap ? si[0][1] : si[0][0];
    o[SEPVAD_EV_SISDR1] = swap ? si[1][0] : si[1][1];
    o[SEPVAD_EV_SISDR_MIX0] = si_mix[0];
    o[SEPVAD_EV_SISDR_MIX1] = si_mix[1];
    o[SEPVAD_EV_PIT_SISDR] = pit_si;
    o[SEPVAD_EV_PIT_SNR] = pit_sn;
    o[SEPVAD_EV_PIT_SISDR_MIX] = ev_pit_max(si_mix[0], si_mix[0], si_mix[1], si_mix[1]);
    o[SEPVAD_EV_PIT_SNR_MIX] = ev_pit_max(sn_mix[0], sn_mix[0], sn_mix[1], sn_mix[1]);
  }
  double* rv = a.rowvals + (long long)b * EV_ROWVALS;
  rv[0] = min_loss; rv[1] = pit_si; rv[2] = pit_sn; rv[3] = (double)si_mix[0] + (double)si_mix[1];
}

}  // namespace sepvad
