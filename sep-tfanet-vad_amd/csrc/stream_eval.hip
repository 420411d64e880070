// Streaming evaluation with known targets (reference model/online_class_known_targets.py:101-123, the window loop of
// calc_online) for all windows of a forward_windows chunk at once:
//   k_se_raw      update_online_signal's slice (:29-38) of every window, un-permuted: raw[b][s][k H + i] =
//                 sep[k][b][s][W - H + i]. Windows are H apart, so sample n of window k and sample n + H of window
//                 k - 1 name the same instant, and the stitched signal that window k is compared with (:112-113) is
//                 the span raw[k H - L_k, k H), L_k = min(k H, W - H), each hop of it permuted by the window it came from.
//   k_se_moments  one launch over (window, stream, job). Jobs 0 .. S - 1 (S = ceil((W - H) / H)): the un-permuted pair
//                 sums of the window's overlap [W - H - L_k, W - H) against one hop segment of that span (the oldest
//                 one partial when H does not divide W - H): sum |e_i - r_t| (nn.L1Loss) or sum e_i, e_i^2, r_t,
//                 r_t^2, e_i r_t (calc_sisdr_loss, model/combined_loss.py:16-60). The other jobs: the window against
//                 its target window (:106, PITLossWrapper(pairwise_neg_sisdr, "pw_mtx")) through eval.hip's
//                 device functions (eval_common.h), one EV_CHUNK each.
//   k_se_finish   eval.hip's closed forms and choice per window-utterance: pw, min loss and perm of :106, with the
//                 bits sepvad_eval_separation gives for that window and target slice.
//   k_se_bsum     L1 only: every segment's sums added over the streams in stream order (nn.L1Loss() means over the
//                 batch, so the choice is batch-global, as in stream.hip).
//   k_se_chain    one wave per stream (one for the batch with L1) walks the chunk's windows in order and composes
//                 each window's pair table from its segment sums under the permutations already chosen,
//                 pw[e][t] = sum_m S(k, m)[e][perm_m[t]], applies the reference's formulas and torch.min's first
//                 minimum (model/pit_wrapper.py:289-312; ties keep the identity) and records perm[k].
//   k_se_stitch   reorder_source_mse (model/combined_loss.py:63-78) + update_online_signal for all windows:
//                 online[b][t][k H + i] = raw[b][perm[k][b][t]][k H + i].
// Window 0 is the reference's seed case (:109-111): the stitched signal is then the window's own un-reordered last
// hop, compared with the window's second-last hop (not the same instants). With SI-SDR it is segment 0 of window 0
// under the identity; with L1 it is launch_pit_l1 (stream.hip) on those two hops, the launch the composed path makes,
// because the left pad leaves that decision on a near-tie that only the same rounding settles the same way.
//
// Every block has a fixed (window, stream, job) and fixed thread ranges, sums are double and added in a fixed order:
// results are bitwise reproducible and do not depend on how the windows are split into chunks, on B for the per-row
// mode, or on the rows' alignment (the float4 and the scalar path give each thread the same samples in the same
// order). The similarity sums are those of the samples themselves (no shift: streaming outputs carry no DC to speak
// of, and a segment's shift would not compose across segments). HBM-bound, no MFMA.
#include "eval_common.h"

namespace sepvad {

constexpr int SE_THREADS = EV_THREADS;
// a (window, segment, stream) record: sums of e_i, e_i^2, r_t, r_t^2 and the pair sums at SE_ER + 2 i + t (L1 uses
// the pair sums only)
constexpr int SE_E = 0, SE_EE = 2, SE_R = 4, SE_RR = 6, SE_ER = 8;
static_assert(SE_ER + 4 == SE_NV && SE_NV <= EV_MOM, "record layout");

template <int MODE>
__device__ __forceinline__ void se_acc(double (&s)[SE_NV], float e0, float e1, float r0, float r1) {
  const double x0 = e0, x1 = e1, y0 = r0, y1 = r1;
  if (MODE == SEPVAD_SE_L1) {
    s[SE_ER + 0] += fabs(x0 - y0); s[SE_ER + 1] += fabs(x0 - y1);
    s[SE_ER + 2] += fabs(x1 - y0); s[SE_ER + 3] += fabs(x1 - y1);
  } else {
    s[SE_E + 0] += x0; s[SE_E + 1] += x1; s[SE_R + 0] += y0; s[SE_R + 1] += y1;
    s[SE_EE + 0] = fma(x0, x0, s[SE_EE + 0]); s[SE_EE + 1] = fma(x1, x1, s[SE_EE + 1]);
    s[SE_RR + 0] = fma(y0, y0, s[SE_RR + 0]); s[SE_RR + 1] = fma(y1, y1, s[SE_RR + 1]);
    s[SE_ER + 0] = fma(x0, y0, s[SE_ER + 0]); s[SE_ER + 1] = fma(x0, y1, s[SE_ER + 1]);
    s[SE_ER + 2] = fma(x1, y0, s[SE_ER + 2]); s[SE_ER + 3] = fma(x1, y1, s[SE_ER + 3]);
  }
}

template <int MODE, bool VEC>
__device__ __forceinline__ void se_span(const float* e0, const float* e1, const float* r0, const float* r1, int cnt,
                                        double (&s)[SE_NV]) {
  const int n4 = cnt / 4;
  for (int q = threadIdx.x; q < n4; q += SE_THREADS) {
    float a[4], b[4], g[4], d[4];
    ev_load4<VEC>(e0, q, a); ev_load4<VEC>(e1, q, b); ev_load4<VEC>(r0, q, g); ev_load4<VEC>(r1, q, d);
#pragma unroll
    for (int k = 0; k < 4; ++k) se_acc<MODE>(s, a[k], b[k], g[k], d[k]);
  }
  const int i = n4 * 4 + threadIdx.x;  // the span's last cnt % 4 samples: one each for threads 0 .. 2
  if (i < cnt) se_acc<MODE>(s, e0[i], e1[i], r0[i], r1[i]);
}

// The span of the stitched signal that segment j of window k covers, and where the window's matching samples start.
// Window k >= 1: hop m = k - 1 - j of raw, cut at k H - L_k. Window 0: its own last hop against its second-last hop
// (segment 0 only; with L1 launch_pit_l1 takes it). cnt = 0: nothing (a hop before the signal's start).
__device__ __forceinline__ void se_segment_span(const StreamEvalArgs& a, long long k, int j, long long& lo, long long& eoff,
                                                int& cnt) {
  cnt = 0; lo = 0; eoff = 0;
  if (k == 0) {
    if (j == 0 && a.mode != SEPVAD_SE_L1) { cnt = (int)a.H; eoff = a.W - 2 * a.H; }
    return;
  }
  const long long m = k - 1 - j;
  if (m < 0) return;
  const long long L = min(k * a.H, a.W - a.H), start = k * a.H - L;
  lo = max(m * a.H, start);
  const long long c = (m + 1) * a.H - lo;
  if (c <= 0) return;
  cnt = (int)c;
  eoff = lo - k * a.H + a.W - a.H;
}

template <int MODE>
__device__ __forceinline__ void se_segment(const StreamEvalArgs& a, int kl, int b, int j, double* red) {
  long long lo, eoff;
  int cnt;
  se_segment_span(a, (long long)a.k0 + kl, j, lo, eoff, cnt);
  double s[SE_NV];
#pragma unroll
  for (int v = 0; v < SE_NV; ++v) s[v] = 0.0;
  if (cnt > 0) {
    const float* e0 = a.sep + ((long long)kl * a.B + b) * 2 * a.sep_ld + eoff;
    const float* e1 = e0 + a.sep_ld;
    const float* r0 = a.raw + (long long)b * 2 * a.raw_ld + lo;
    const float* r1 = r0 + a.raw_ld;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(e0) | reinterpret_cast<uintptr_t>(e1) |
                           reinterpret_cast<uintptr_t>(r0) | reinterpret_cast<uintptr_t>(r1);
    if ((bits & 15) == 0) se_span<MODE, true>(e0, e1, r0, r1, cnt, s);
    else se_span<MODE, false>(e0, e1, r0, r1, cnt, s);
  }
  block_sums_store<SE_NV, SE_THREADS / 64>(s, red, a.seg, (((long long)kl * a.S + j) * a.B + b) * SE_NV);
}

// window-utterance u = kl B + b of the chunk: its estimate rows and its target window
__device__ __forceinline__ const float* se_est(const StreamEvalArgs& a, int u) {
  return a.sep + (long long)u * 2 * a.sep_ld;
}
__device__ __forceinline__ const float* se_tgt(const StreamEvalArgs& a, int u) {
  const int kl = u / a.B, b = u % a.B;
  return a.ev.tgt + (long long)b * 2 * a.ev.tgt_ld + (long long)kl * a.H;
}

// grid n B (nsim + nchunk): block (u, r): r < nsim a similarity segment, else chunk r - nsim of the target moments
__global__ __launch_bounds__(SE_THREADS) void k_se_moments(StreamEvalArgs a, int nsim) {
  __shared__ double red[EV_MOM * (SE_THREADS / 64)];
  const int per = nsim + a.ev.nchunk;
  const int u = blockIdx.x / per, r = blockIdx.x % per;
  if (r < nsim) {
    const int kl = u / a.B, b = u % a.B;
    if (a.mode == SEPVAD_SE_L1) se_segment<SEPVAD_SE_L1>(a, kl, b, r, red);
    else se_segment<SEPVAD_SE_SISDR>(a, kl, b, r, red);
  } else {
    const int c = r - nsim;
    const float* e0 = se_est(a, u);
    const float* t0 = se_tgt(a, u);
    ev_block_moments(e0, e0 + a.sep_ld, t0, t0 + a.ev.tgt_ld, nullptr, a.ev.N, c, red,
                     a.ev.partial + ((long long)u * a.ev.nchunk + c) * EV_MOM);
  }
}

// One wave per window-utterance: eval.hip's finish
__global__ __launch_bounds__(64) void k_se_finish(StreamEvalArgs a) {
  const int u = blockIdx.x;
  ev_finish(a.ev, u, se_est(a, u), se_tgt(a, u), nullptr);
}

// L1: grid n S, block (kl, j): bsum[kl][j][v] = sum over the streams, in stream order per thread and then in the
// block's fixed order, of the segment's pair sums
__global__ __launch_bounds__(SE_THREADS) void k_se_bsum(StreamEvalArgs a) {
  __shared__ double red[16];
  const double* p = a.seg + (long long)blockIdx.x * a.B * SE_NV + SE_ER;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < a.B; b += SE_THREADS) {
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[v] += p[(long long)b * SE_NV + v];
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const double t = block_sum(acc[v], red);
    if (threadIdx.x == 0) a.bsum[(long long)blockIdx.x * 4 + v] = t;
  }
}

// grid G (streams, or 1 with L1), one wave. hist[m % S] = 1 when window m was appended swapped, for the S windows
// before the current one.
__global__ __launch_bounds__(64) void k_se_chain(StreamEvalArgs a) {
  __shared__ int hist[SE_MAX_SEG];
  const int g = blockIdx.x, l = threadIdx.x, S = a.S;
  const bool l1 = a.mode == SEPVAD_SE_L1;
  const int G = l1 ? 1 : a.B;
  for (long long m = max(0LL, (long long)a.k0 - S) + l; m < a.k0; m += 64)
    hist[m % S] = (int)(a.perm[(m * a.B + g) * 2] & 1);
  __syncthreads();
  for (int kl = 0; kl < a.n; ++kl) {
    const long long k = (long long)a.k0 + kl;
    bool swap;
    if (l1 && k == 0) {
      swap = (a.perm[0] & 1) != 0;  // launch_pit_l1's choice (and its pw_sim[0]), made before this launch
    } else {
      double s[SE_NV];
#pragma unroll
      for (int v = 0; v < SE_NV; ++v) s[v] = 0.0;
      for (int j = l; j < S; j += 64) {
        const long long m = k - 1 - j;
        const int sw = (k > 0 && m >= 0) ? hist[m % S] : 0;
        if (l1) {
          const double* p = a.bsum + ((long long)kl * S + j) * 4;
#pragma unroll
          for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int t = 0; t < 2; ++t) s[SE_ER + 2 * e + t] += p[2 * e + (t ^ sw)];
        } else {
          const double* p = a.seg + (((long long)kl * S + j) * a.B + g) * SE_NV;
#pragma unroll
          for (int e = 0; e < 2; ++e) { s[SE_E + e] += p[SE_E + e]; s[SE_EE + e] += p[SE_EE + e]; }
#pragma unroll
          for (int t = 0; t < 2; ++t) { s[SE_R + t] += p[SE_R + (t ^ sw)]; s[SE_RR + t] += p[SE_RR + (t ^ sw)]; }
#pragma unroll
          for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int t = 0; t < 2; ++t) s[SE_ER + 2 * e + t] += p[SE_ER + 2 * e + (t ^ sw)];
        }
      }
#pragma unroll
      for (int v = 0; v < SE_NV; ++v) s[v] = wave_sum(s[v]);
      const double Ld = k == 0 ? (double)a.H : (double)min(k * a.H, a.W - a.H);
      float pw[4];  // [est e][target t] at 2 e + t
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (l1) {
            pw[2 * e + t] = (float)(s[SE_ER + 2 * e + t] / ((double)a.B * Ld));  // nn.L1Loss: mean over batch and samples
          } else {  // calc_sisdr_loss: zero-mean SI-SDR with float32 epsilon, negated
            const double pp = ev_energy(s[SE_EE + e], s[SE_E + e], Ld, 1), tt = ev_energy(s[SE_RR + t], s[SE_R + t], Ld, 1);
            const double pt = ev_cen(s[SE_ER + 2 * e + t], s[SE_E + e], s[SE_R + t], Ld, 1);
            pw[2 * e + t] = -(float)ev_score(EVK_SI, pp, tt, pt, 1, 0.0);
          }
        }
      // find_best_perm_factorial (model/pit_wrapper.py:289-312) on the float32 table: the first minimum wins
      const float loss_id = (pw[0] + pw[3]) / 2.f, loss_sw = (pw[2] + pw[1]) / 2.f;
      swap = loss_sw < loss_id;
      if (l == 0 && a.pw_sim) {
#pragma unroll
        for (int v = 0; v < 4; ++v) a.pw_sim[(k * G + g) * 4 + v] = pw[v];
      }
      // every lane made the same choice from the same sums; the rows' indices are written by all lanes
      const int b0 = l1 ? 0 : g, b1 = l1 ? a.B : g + 1;
      for (int b = b0 + l; b < b1; b += 64) {
        a.perm[(k * a.B + b) * 2] = swap ? 1 : 0;
        a.perm[(k * a.B + b) * 2 + 1] = swap ? 0 : 1;
      }
    }
    __syncthreads();  // every lane has read the slot that window k takes over
    if (l == 0) hist[k % S] = swap ? 1 : 0;
    __syncthreads();
  }
}

// rows beyond gridDim.y by a stride loop (as stream.hip's row kernels)
static dim3 se_row_grid(long long n, long long rows) {
  const long long nb = (n + 1023) / 1024;
  return dim3((unsigned)(nb < 1 ? 1 : nb > 64 ? 64 : nb), (unsigned)(rows < 65535 ? rows : 65535));
}

__global__ __launch_bounds__(256) void k_se_raw(StreamEvalArgs a) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
  const long long rows = (long long)a.n * a.B * 2;
  for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
    const long long u = row >> 1, kl = u / a.B, b = u % a.B;
    const int s = (int)(row & 1);
    copy_run(a.raw + (b * 2 + s) * a.raw_ld + (a.k0 + kl) * a.H, a.sep + row * a.sep_ld + a.W - a.H, a.H, tid, nth);
  }
}

__global__ __launch_bounds__(256) void k_se_stitch(StreamEvalArgs a) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
  const long long rows = (long long)a.n * a.B * 2;
  for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
    const long long u = row >> 1, k = a.k0 + u / a.B, b = u % a.B;
    const int t = (int)(row & 1);
    const int p = (int)(a.perm[(k * a.B + b) * 2 + t] & 1);
    copy_run(a.online + (b * 2 + t) * a.on_ld + k * a.H, a.raw + (b * 2 + p) * a.raw_ld + k * a.H, a.H, tid, nth);
  }
}

hipError_t launch_stream_eval(const StreamEvalArgs& a, hipStream_t s) {
  const int nsim = a.mode == SEPVAD_SE_NONE ? 0 : a.S;
  const long long nu = (long long)a.n * a.B, blocks = nu * ((long long)nsim + a.ev.nchunk);
  if (a.B < 1 || a.n < 1 || a.k0 < 0 || a.k0 + a.n > a.K || a.H < 1 || a.H > a.W || a.ev.nchunk < 1 ||
      blocks > 0x7fffffffLL || (nsim > 0 && (a.S < 1 || a.S > SE_MAX_SEG || 2 * a.H > a.W)))
    return hipErrorInvalidValue;
  const dim3 rg = se_row_grid(a.H, 2 * nu);
  hipLaunchKernelGGL(k_se_raw, rg, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_se_moments, dim3((unsigned)blocks), dim3(SE_THREADS), 0, s, a, nsim);
  hipLaunchKernelGGL(k_se_finish, dim3((unsigned)nu), dim3(64), 0, s, a);
  if (nsim > 0) {
    if (a.mode == SEPVAD_SE_L1) {
      if (a.pit0.nblk > 0) {
        const hipError_t e = launch_pit_l1(a.pit0, s);
        if (e != hipSuccess) return e;
      }
      hipLaunchKernelGGL(k_se_bsum, dim3((unsigned)(a.n * a.S)), dim3(SE_THREADS), 0, s, a);
    }
    hipLaunchKernelGGL(k_se_chain, dim3(a.mode == SEPVAD_SE_L1 ? 1 : a.B), dim3(64), 0, s, a);
  }
  hipLaunchKernelGGL(k_se_stitch, rg, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sepvad
