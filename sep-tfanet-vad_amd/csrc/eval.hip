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
#include "eval_common.h"

namespace sepvad {

// grid B * nchunk: workgroup b * nchunk + c reduces samples [c EV_CHUNK, min(N, (c + 1) EV_CHUNK)) of utterance b
__global__ __launch_bounds__(EV_THREADS) void k_eval_moments(EvalSepArgs a) {
  __shared__ double red[EV_MOM * (EV_THREADS / 64)];
  const int b = blockIdx.x / a.nchunk, c = blockIdx.x % a.nchunk;
  const float* e0 = a.est + (long long)b * 2 * a.est_ld;
  const float* t0 = a.tgt + (long long)b * 2 * a.tgt_ld;
  const float* m = a.mix ? a.mix + (long long)b * a.mix_ld : nullptr;
  ev_block_moments(e0, e0 + a.est_ld, t0, t0 + a.tgt_ld, m, a.N, c, red, a.partial + (long long)blockIdx.x * EV_MOM);
}

// One wave per utterance: ev_finish (eval_common.h)
__global__ __launch_bounds__(64) void k_eval_finish(EvalSepArgs a) {
  const int b = blockIdx.x;
  ev_finish(a, b, a.est + (long long)b * 2 * a.est_ld, a.tgt + (long long)b * 2 * a.tgt_ld,
            a.mix ? a.mix + (long long)b * a.mix_ld : nullptr);
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
