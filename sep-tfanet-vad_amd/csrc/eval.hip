// The evaluation criterion of the reference's test.py on the device (test.py:49-64,129-172): the pairwise negative
// SDR matrix and its permutation choice (model/sdr.py:48-86 PairwiseNegSDR, model/pit_wrapper.py:287-312
// find_best_perm_factorial), the score sheet of one step (calc_sisdr, pit_si_sdr, pit_snr, si_sdri of the estimates
// and of the mixture), the weighted BCE of the VAD track (model/combined_loss.py:120-138), confusion counts and the
// mask-based VAD (Our_utils/utils_test.py:67-73 calc_vad).
//
// Every separation number of a step is a closed form of 16 sums over five rows of one utterance (two estimates e_i,
// two targets t_j, the mixture m):
//   EVM_S:  sum e_0, sum e_1, sum t_0, sum t_1, sum m            (5)
//   EVM_Q:  the same rows' sums of squares                       (5)
//   EVM_ET: <e_i, t_j> at 2 i + j                                (4)
//   EVM_MT: <m, t_j>                                             (2)
// k_eval_moments reads the rows once, EV_CHUNK samples per workgroup, and writes one double[16] partial per
// (utterance, chunk); k_eval_finish adds an utterance's partials in chunk order and evaluates the closed forms in
// double; k_eval_means takes the batch means. No atomics, every sum in a fixed order: results are bitwise
// reproducible, and an utterance's numbers depend on its own rows and N only (not on B, and not on the rows'
// alignment: the float4 and the scalar path give each thread the same samples in the same order).
//
// Conditioning. The zero-mean closed forms (<x',y'> = <x,y> - sum x sum y / N, <e,e> = al^2 <t,t> - 2 al <p,t> + <p,p>)
// lose (mean^2 / variance) (signal / residual) of the moments' precision; on raw rows with a DC of 100 .. 1000 standard
// deviations that is 1e-3 .. 1 dB at a 71 .. 78 dB residual. The sums are therefore those of the rows less their own
// first sample (every chunk of a row subtracts the row's first sample, so the partials still add up): the centred
// moments do not depend on the shift, the difference of two floats is exact in double, and what is left of the mean
// is of the order of the row's standard deviation. zero_mean = 0 needs the raw moments: k_eval_finish takes the shift
// out again in closed form (ev_raw), which costs rounding only. Measured table: DESIGN.md section 12,
// tests/test_gpu_score_regimes.py.
#include "device_common.h"
#include "../../include/sepvad.h"

namespace sepvad {

constexpr int EV_THREADS = 256;
constexpr int EVM_S = 0, EVM_Q = 5, EVM_ET = 10, EVM_MT = 14;
static_assert(EV_CHUNK % 4 == 0, "chunk bases must keep a row's 16-byte alignment");

// four consecutive samples 4 q .. 4 q + 3 of row p (null: zeros)
template <bool VEC>
__device__ __forceinline__ void ev_load4(const float* p, int q, float (&v)[4]) {
  if (!p) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
  } else if (VEC) {
    const float4 f = reinterpret_cast<const float4*>(p)[q];
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p[4 * q + k];
  }
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

// grid B * nchunk: workgroup b * nchunk + c reduces samples [c EV_CHUNK, min(N, (c + 1) EV_CHUNK)) of utterance b
__global__ __launch_bounds__(EV_THREADS) void k_eval_moments(EvalSepArgs a) {
  __shared__ double red[EV_MOM * (EV_THREADS / 64)];
  const int b = blockIdx.x / a.nchunk, c = blockIdx.x % a.nchunk;
  const long long off = (long long)c * EV_CHUNK;
  const long long left = a.N - off;
  const int len = left < EV_CHUNK ? (int)left : EV_CHUNK;
  const float* e0 = a.est + (long long)b * 2 * a.est_ld + off;
  const float* e1 = e0 + a.est_ld;
  const float* t0 = a.tgt + (long long)b * 2 * a.tgt_ld + off;
  const float* t1 = t0 + a.tgt_ld;
  const float* m = a.mix ? a.mix + (long long)b * a.mix_ld + off : nullptr;
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
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < EV_MOM; ++k) {
    const double v = wave_sum(s[k]);
    if (l == 0) red[k * (EV_THREADS / 64) + w] = v;
  }
  __syncthreads();
  if (threadIdx.x < EV_MOM) {
    double v = 0.0;
    for (int i = 0; i < EV_THREADS / 64; ++i) v += red[threadIdx.x * (EV_THREADS / 64) + i];
    a.partial[(long long)blockIdx.x * EV_MOM + threadIdx.x] = v;
  }
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

// One wave per utterance. Lanes 0..15 add one moment each over the chunks in chunk order; then 16 lanes evaluate
// one number each (job below) from moments fetched from the lanes that hold them, and lane 0 chooses and stores.
__global__ __launch_bounds__(64) void k_eval_finish(EvalSepArgs a) {
  const int b = blockIdx.x, l = threadIdx.x;
  // zero_mean = 0 takes the shift of k_eval_moments out again: lane r < 5 fetches the first sample of row r (issued
  // ahead of the partials; with zero_mean nothing needs it)
  double piv = 0.0;
  if (!a.zero_mean) {
    if (l < 2) piv = (double)a.est[((long long)b * 2 + l) * a.est_ld];
    else if (l < 4) piv = (double)a.tgt[((long long)b * 2 + l - 2) * a.tgt_ld];
    else if (l == 4 && a.mix) piv = (double)a.mix[(long long)b * a.mix_ld];
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

// One workgroup: the batch means of the per-utterance float32 values, summed in double in a fixed order.
__global__ __launch_bounds__(EV_THREADS) void k_eval_means(EvalSepArgs a) {
  __shared__ double red[16];
  double tot[EV_ROWVALS];
#pragma unroll
  for (int q = 0; q < EV_ROWVALS; ++q) {
    double v = 0.0;
    for (int b = threadIdx.x; b < a.B; b += EV_THREADS) v += a.rowvals[(long long)b * EV_ROWVALS + q];
    tot[q] = block_sum(v, red);
  }
  if (threadIdx.x == 0) {
    const double Bd = (double)a.B;
    const float pit_si = (float)(tot[1] / Bd);
    a.means[SEPVAD_EV_MEAN_LOSS] = (float)(tot[0] / Bd);
    a.means[SEPVAD_EV_MEAN_PIT_SISDR] = pit_si;
    a.means[SEPVAD_EV_MEAN_PIT_SNR] = (float)(tot[2] / Bd);
    a.means[SEPVAD_EV_MEAN_SI_SDRI] = pit_si - (float)(tot[3] / (2.0 * Bd));  // metric.py:157-160, float32 difference
  }
}

hipError_t launch_eval_separation(const EvalSepArgs& a, hipStream_t s) {
  if (a.B < 1 || a.N < 1 || a.nchunk < 1 || (long long)a.B * a.nchunk > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_eval_moments, dim3((unsigned)(a.B * a.nchunk)), dim3(EV_THREADS), 0, s, a);
  hipLaunchKernelGGL(k_eval_finish, dim3(a.B), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_eval_means, dim3(1), dim3(EV_THREADS), 0, s, a);
  return hipGetLastError();
}

// ---- the VAD track ---------------------------------------------------------------------------------------------

constexpr int EVV_THREADS = 1024, EVV_WAVES = EVV_THREADS / 64;
constexpr int EVS_TILE = 64;       // frames per workgroup of k_eval_simple_vad (one per lane)
constexpr int EVS_THREADS = 256;
constexpr int EVS_MIN_BINS = 65;   // sum >= 257 * 0.25 = 64.25 (utils_test.py:72) on an integer count

// calc_vad (Our_utils/utils_test.py:67-73) of the masks reordered by perm (test.py:148,170): workgroup
// (b, s, tile) counts, for 64 frames, the bins of masks[b][perm[b][s]] that are >= 0.5; T is the fast axis, so a
// wave reads 64 consecutive floats per bin; the four waves take every fourth bin.
__global__ __launch_bounds__(EVS_THREADS) void k_eval_simple_vad(EvalVadArgs a, int ntile) {
  __shared__ int cnt[EVS_THREADS / 64][EVS_TILE];
  const int bs = blockIdx.x / ntile, tile = blockIdx.x % ntile;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int t = tile * EVS_TILE + l;
  const int src = a.perm ? (int)(a.perm[bs] & 1) : (bs & 1);
  const float* m = a.masks + ((long long)(bs & ~1) + src) * EV_MASK_BINS * a.T;
  int c = 0;
  if (t < a.T)
    for (int f = w; f < EV_MASK_BINS; f += EVS_THREADS / 64) c += m[(long long)f * a.T + t] >= 0.5f ? 1 : 0;
  cnt[w][l] = c;
  __syncthreads();
  if (w == 0 && t < a.T) {
    int tot = 0;
#pragma unroll
    for (int i = 0; i < EVS_THREADS / 64; ++i) tot += cnt[i][l];
    a.simple[(long long)bs * a.T + t] = tot >= EVS_MIN_BINS ? 1 : 0;
  }
}

// confusion_matrix(labels=[0., 1.]).ravel() order: (tn, fp, fn, tp); pairs with another label value are left out
__device__ __forceinline__ void ev_count(int (&k)[8], int s, float y, bool pred) {
  const int col = y == 0.f ? (pred ? 1 : 0) : (y == 1.f ? (pred ? 3 : 2) : -1);
#pragma unroll
  for (int q = 0; q < 4; ++q) k[s * 4 + q] += q == col ? 1 : 0;
}

// One workgroup; wave w takes utterances w, w + 16, ...: the [B, 2, T] tracks are small (2 T values a row), and
// the pairwise table and the mean run over the whole batch. Per utterance: labels 2 -> 1 (written back when
// fix_labels, combined_loss.py:130-131), the four weighted-BCE sums of vad[b, i] against labels[b, j]
// (:132-137; log in double, clamped at -100 as nn.BCELoss), the row loss under perm, and the confusion counts of
// vad > 0.5 (model/metric.py:170 Accuracy_Vad's rule) and of the mask-based VAD against the labels (test.py:164,172).
__global__ __launch_bounds__(EVV_THREADS) void k_eval_vad(EvalVadArgs a) {
  __shared__ double red[EVV_WAVES][5];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int T = a.T;
  double bsum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // the batch's four cells, the sum of the float32 row losses
  for (int b = w; b < a.B; b += EVV_WAVES) {
    const int p0 = a.perm ? (int)(a.perm[(long long)b * 2] & 1) : 0;
    const int p1 = a.perm ? (int)(a.perm[(long long)b * 2 + 1] & 1) : 1;
    const float* v = a.vad + (long long)b * 2 * T;
    float* lab = a.labels + (long long)b * 2 * T;
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    int k[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ks[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = l; t < T; t += 64) {
      const float pv[2] = {v[t], v[T + t]};
      float y[2] = {lab[t], lab[T + t]};
      double lp[2], lq[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (y[j] == 2.f) {
          y[j] = 1.f;
          if (a.fix_labels) lab[j * T + t] = 1.f;
        }
        const double p = pv[j];
        lp[j] = fmax(log(p), -100.0);
        lq[j] = fmax(log(1.0 - p), -100.0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const double yy = y[j];
          const double wgt = yy * 0.36 + 0.64 * (1.0 - yy);
          c[i * 2 + j] += -(yy * lp[i] + (1.0 - yy) * lq[i]) * wgt;
        }
      const float q0 = p0 ? pv[1] : pv[0], q1 = p1 ? pv[1] : pv[0];
      ev_count(k, 0, y[0], q0 > 0.5f);  // a NaN probability is not > 0.5: prediction 0
      ev_count(k, 1, y[1], q1 > 0.5f);
      if (a.conf_simple) {
        ev_count(ks, 0, y[0], a.simple[(long long)b * 2 * T + t] != 0);
        ev_count(ks, 1, y[1], a.simple[((long long)b * 2 + 1) * T + t] != 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = wave_sum(c[q]);
#pragma unroll
    for (int q = 0; q < 8; ++q) k[q] = wave_sum(k[q]);
    if (a.conf_simple) {
#pragma unroll
      for (int q = 0; q < 8; ++q) ks[q] = wave_sum(ks[q]);
    }
    if (l == 0) {
      // pred_vad reordered by perm against the labels: speaker 0 then speaker 1
      const float row = (float)((p0 ? c[2] : c[0]) + (p1 ? c[3] : c[1]));
      a.bce_rows[b] = row;
#pragma unroll
      for (int q = 0; q < 8; ++q) a.conf[(long long)b * 8 + q] = k[q];
      if (a.conf_simple) {
#pragma unroll
        for (int q = 0; q < 8; ++q) a.conf_simple[(long long)b * 8 + q] = ks[q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) bsum[q] += c[q];
      bsum[4] += (double)row;
    }
  }
  if (l == 0) {
#pragma unroll
    for (int q = 0; q < 5; ++q) red[w][q] = bsum[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < EVV_WAVES; ++i)
#pragma unroll
      for (int q = 0; q < 5; ++q) tot[q] += red[i][q];
#pragma unroll
    for (int q = 0; q < 4; ++q) a.pw_ce[q] = (float)tot[q];
    a.bce_mean[0] = (float)(tot[4] / (double)a.B);
  }
}

hipError_t launch_eval_vad(const EvalVadArgs& a, hipStream_t s) {
  if (a.B < 1 || a.T < 1) return hipErrorInvalidValue;
  if (a.masks) {
    const long long ntile = ((long long)a.T + EVS_TILE - 1) / EVS_TILE;
    if (!a.simple || 2LL * a.B * ntile > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_eval_simple_vad, dim3((unsigned)(2LL * a.B * ntile)), dim3(EVS_THREADS), 0, s, a, (int)ntile);
  }
  if (a.vad) hipLaunchKernelGGL(k_eval_vad, dim3(1), dim3(EVV_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace sepvad
