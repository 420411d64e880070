// Backward of the forward's tail (model/model.py:421-461): torch.istft, the mask product est = X sigmoid(masks)
// (:429-437), and the VAD head on the pre-sigmoid masks (:153-179). From the gradients of sep [B][2][N] and vad
// [B][2][T] to the gradient at masks_b [B][2][257][T] and the gradients of the VAD head's folded parameters. The forward
// kernels are untouched; DESIGN.md section 15 has the derivation.
//
// Separation path. With w the inv_spec window and env[n] = sum_f w^2[n - 256 f] the overlap-add envelope, the adjoint of
// torch.istft(center=True, length=N) is, per frame f, G_f[k] = (c_k / 512) rfft(u_f)[k] with u_f[j] = w[j] g~[256 f + j],
// g~[n] = g_sep[n - 256] / env[n] on [256, 256 + N) and zero elsewhere, c_0 = c_256 = 1, otherwise 2. The gradient at
// sigmoid(masks) is Re X Re G + Im X Im G; X is recomputed from the mixture with the front end's own transform
// (reflect padding, DC zeroed), so the launch reads nothing a forward left behind.
//
// VAD path. k_tail_feat recomputes conv1_1 on the masks in double, k_vad_grad takes one (utterance, speaker) from the
// gradient of its VAD track back to the gradient g_y at the conv1_1 output [4][T] (sigmoid, conv 4 -> 1, GroupNorm(1, 4),
// PReLU, all in double, every sum in a fixed order) and writes that row's partial sums of the small parameters;
// k_vad_grad_w1 correlates g_y with the masks for the conv1_1 weights; k_tail_param_finish adds the rows' partials in a
// fixed order. k_tail_grad_masks adds the transposed conv1_1 of g_y to the separation term, so every element of the masks
// gradient is written exactly once: no read-modify-write, no atomics, bitwise reproducible, and utterance b's masks
// gradient depends on its own rows only.
#include "device_common.h"
#include "fft_common.h"

namespace sepvad {

constexpr int TF_ROWS = 64;   // frames per workgroup of k_tail_feat (one per lane)
constexpr int TV_THREADS = 256;
constexpr int TV_NW = TV_THREADS / 64;
// layout of a row's small partials (TG_NSMALL doubles)
constexpr int TS_W2 = 0, TS_B2 = 12, TS_GAM = 13, TS_BET = 17, TS_ALPHA = 21, TS_B1 = 22;
static_assert(TS_B1 + 4 == TG_NSMALL, "small partials");

// y[o][t] = b1[o] + sum_c sum_k w1[o][c][k] masks[c][t + k - 2] (zero outside [0, T)) for TF_ROWS frames of one
// (utterance, speaker): lane = frame, wave w takes the channels w, w + TF_NW, ...; the waves' sums are added in wave order.
constexpr int TF_NW = 16;
__global__ __launch_bounds__(64 * TF_NW) void k_tail_feat(TailGradArgs a) {
  __shared__ double part[TF_NW][4][TF_ROWS];
  __shared__ double ws[TG_NW1];  // the weights, read wave-uniformly below (LDS broadcast)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bs = blockIdx.x, T = a.T, t = blockIdx.y * TF_ROWS + lane;
  const float* mb = a.masks + (size_t)bs * NBIN * T;
  for (int i = tid; i < TG_NW1; i += 64 * TF_NW) ws[i] = a.vw[i];
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
  for (int c = wave; c < NBIN; c += TF_NW) {
    const float* row = mb + (size_t)c * T;
    float m[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {  // a clamped load and a select: no branch around the load
      const int tt = t - 2 + k;
      const float v = row[min(max(tt, 0), T - 1)];
      m[k] = (tt >= 0 && tt < T) ? v : 0.f;
    }
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int k = 0; k < 5; ++k) acc[o] = fma(ws[(o * NBIN + c) * 5 + k], (double)m[k], acc[o]);
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) part[wave][o][lane] = acc[o];
  __syncthreads();
  if (tid < 4 * TF_ROWS) {
    const int o = tid >> 6;
    double y = part[0][o][lane];
    for (int w = 1; w < TF_NW; ++w) y += part[w][o][lane];
    if (t < T) a.feat[((size_t)bs * 4 + o) * T + t] = y + a.vw[TG_NW1 + TS_B1 + o];
  }
}

// Block sums of NV doubles per thread into tot[0..NV) (fixed order: shuffle tree, then the waves in wave order), visible
// to every thread on return.
template <int NV>
__device__ __forceinline__ void tv_sums(const double (&s)[NV], double* red, double* tot) {
  __syncthreads();  // the readers of an earlier call are done with red and tot
  block_sums_store<NV, TV_NW>(s, red, tot);
  __syncthreads();
}

// One workgroup per (utterance, speaker): model/model.py:160-179 backwards in double.
__global__ __launch_bounds__(TV_THREADS) void k_vad_grad(TailGradArgs a) {
  constexpr int NS3 = 23;
  __shared__ double red[NS3 * TV_NW];
  __shared__ double tot[NS3];
  const int tid = threadIdx.x, bs = blockIdx.x, T = a.T;
  const double* Y = a.feat + (size_t)bs * 4 * T;
  double* GZ = a.gz + (size_t)bs * T;
  const float* gv = a.g_vad + (long long)(bs >> 1) * a.gv_b + (long long)(bs & 1) * a.gv_s;
  const double* vs = a.vw + TG_NW1;  // the small parameters, in the partials' layout
  const double M = 4.0 * (double)T, alpha = vs[TS_ALPHA];
  double gam[4], bet[4], w2[4][3];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    gam[o] = vs[TS_GAM + o];
    bet[o] = vs[TS_BET + o];
#pragma unroll
    for (int k = 0; k < 3; ++k) w2[o][k] = vs[TS_W2 + o * 3 + k];
  }
  auto prelu = [&](double y) { return y > 0.0 ? y : alpha * y; };
  // GroupNorm(1, 4) statistics of v = PReLU(y) over [4][T]: the mean, then the centred second moment
  double s1[1] = {0.0};
  for (int i = tid; i < 4 * T; i += TV_THREADS) s1[0] += prelu(Y[i]);
  tv_sums<1>(s1, red, tot);
  const double mu = tot[0] / M;
  s1[0] = 0.0;
  for (int i = tid; i < 4 * T; i += TV_THREADS) {
    const double d = prelu(Y[i]) - mu;
    s1[0] += d * d;
  }
  tv_sums<1>(s1, red, tot);
  const double rstd = 1.0 / sqrt(tot[0] / M + (double)a.eps);
  auto xhat = [&](int o, int t) { return (prelu(Y[(size_t)o * T + t]) - mu) * rstd; };
  auto feat = [&](int o, int t) {  // BN_1 output, zero outside [0, T) (the conv's padding)
    return (t >= 0 && t < T) ? xhat(o, t) * gam[o] + bet[o] : 0.0;
  };
  // the gradient before the output sigmoid: g_z = g_vad p (1 - p)
  for (int t = tid; t < T; t += TV_THREADS) {
    double z = vs[TS_B2];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int k = 0; k < 3; ++k) z = fma(w2[o][k], feat(o, t + k - 1), z);
    const double p = 1.0 / (1.0 + exp(-z));
    GZ[t] = (double)gv[(long long)t * a.gv_t] * p * (1.0 - p);
  }
  __syncthreads();
  // z[t'] = b2 + sum_o sum_k w2[o][k] n[o][t' + k - 1], so g_n[o][t] = sum_k w2[o][k] g_z[t - k + 1]
  auto gn = [&](int o, int t) {
    const double gp = t + 1 < T ? GZ[t + 1] : 0.0, gm = t > 0 ? GZ[t - 1] : 0.0;
    return w2[o][0] * gp + w2[o][1] * GZ[t] + w2[o][2] * gm;
  };
  double s3[NS3];
#pragma unroll
  for (int i = 0; i < NS3; ++i) s3[i] = 0.0;
  for (int t = tid; t < T; t += TV_THREADS) {
    const double gz = GZ[t];
    s3[TS_B2] += gz;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s3[TS_W2 + o * 3 + k] += gz * feat(o, t + k - 1);
      const double g = gn(o, t), xh = xhat(o, t), gx = g * gam[o];
      s3[TS_GAM + o] += g * xh;
      s3[TS_BET + o] += g;
      s3[21] += gx;
      s3[22] += gx * xh;
    }
  }
  tv_sums<NS3>(s3, red, tot);
  double* ps = a.part_small + (size_t)bs * TG_NSMALL;
  if (tid < 21) ps[tid] = tot[tid];  // w2, b2, BN_1 weight and bias
  const double S1 = tot[21] / M, S2 = tot[22] / M;
  // GroupNorm and PReLU (torch's convention at 0: input gradient alpha g, weight gradient y g = 0)
  double s4[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = tid; t < T; t += TV_THREADS) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const double xh = xhat(o, t);
      const double g_v = rstd * (gn(o, t) * gam[o] - S1 - xh * S2);
      const double y = Y[(size_t)o * T + t];
      const double g_y = y > 0.0 ? g_v : alpha * g_v;
      if (!(y > 0.0)) s4[0] += y * g_v;
      s4[1 + o] += g_y;
      a.gyd[((size_t)bs * 4 + o) * T + t] = g_y;
      a.gy[((size_t)bs * 4 + o) * T + t] = (float)g_y;
    }
  }
  tv_sums<5>(s4, red, tot);
  if (tid < 5) ps[TS_ALPHA + tid] = tot[tid];
}

// g_w1[o][c][k] = sum_t g_y[o][t] masks[c][t + k - 2] over TG_W1_T frames of one (utterance, speaker): lane -> (channel,
// tap), 12 channels per wave, each lane walking its masks row frame by frame (its four sums in double, in frame order)
// with g_y broadcast from LDS. One partial row per (utterance, speaker, chunk of frames).
constexpr int TW_CH = 12, TW_CPW = TW_CH * TV_NW;
__global__ __launch_bounds__(TV_THREADS) void k_vad_grad_w1(TailGradArgs a) {
  __shared__ double gys[4][TG_W1_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bs = blockIdx.x, T = a.T, t0 = blockIdx.z * TG_W1_T, nt = min(TG_W1_T, T - t0);
  for (int i = tid; i < 4 * TG_W1_T; i += TV_THREADS) {
    const int o = i / TG_W1_T, tt = i % TG_W1_T;
    gys[o][tt] = tt < nt ? a.gyd[((size_t)bs * 4 + o) * T + t0 + tt] : 0.0;
  }
  __syncthreads();
  const int cl = lane / 5, k = lane - 5 * cl;
  const int c = (blockIdx.y * TV_NW + wave) * TW_CH + cl;
  if (cl >= TW_CH || c >= NBIN) return;
  const float* row = a.masks + ((size_t)bs * NBIN + c) * T;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
  for (int i = 0; i < nt; ++i) {
    const int tt = t0 + i + k - 2;
    const float v = row[min(max(tt, 0), T - 1)];  // a clamped load and a select: no branch around the load
    const double m = (tt >= 0 && tt < T) ? (double)v : 0.0;
#pragma unroll
    for (int o = 0; o < 4; ++o) acc[o] = fma(gys[o][i], m, acc[o]);
  }
  double* out = a.part_w1 + ((size_t)bs * gridDim.z + blockIdx.z) * TG_NW1;
#pragma unroll
  for (int o = 0; o < 4; ++o) out[((size_t)o * NBIN + c) * 5 + k] = acc[o];
}

// gpar[i] = the sum of the rows' partials: 16 parameters per workgroup, thread (parameter, j) adds the rows j, j + 16, ...
// in that order, then the 16 sums are added in order (a fixed order whatever the batch)
constexpr int TP_PAR = 16;
__global__ __launch_bounds__(TV_THREADS) void k_tail_param_finish(TailGradArgs a) {
  __shared__ double red[TV_THREADS / TP_PAR][TP_PAR];
  const int pl = threadIdx.x % TP_PAR, j = threadIdx.x / TP_PAR;
  const int i = blockIdx.x * TP_PAR + pl;
  const bool big = i < TG_NW1;
  const double* p = big ? a.part_w1 + i : a.part_small + (i - TG_NW1);
  const size_t ld = big ? TG_NW1 : TG_NSMALL;
  const int R = 2 * a.B * (big ? tg_w1_chunks(a.T) : 1);
  double s = 0.0;
  if (i < TG_NPAR)
#pragma unroll 4
    for (int r = j; r < R; r += TV_THREADS / TP_PAR) s += p[(size_t)r * ld];
  red[j][pl] = s;
  __syncthreads();
  if (j == 0 && i < TG_NPAR) {
    double v = 0.0;
    for (int q = 0; q < TV_THREADS / TP_PAR; ++q) v += red[q][pl];
    a.gpar[i] = v;
  }
}

// ------------------------------------------------------------------------------------------
// The hot kernel: one workgroup per (utterance, TG_OWN frames), both speakers. Transforms (16 lanes each, four per wave,
// the front end's register FFT): TG_OWN of the mixture's frames (X) and TG_OWN of each speaker's u_f (G), then thread ->
// (bin k, frame): the three split steps, the product, m (1 - m) and the VAD term, stored bin-major with TG_OWN consecutive
// frames per (speaker, bin) row, as k_istft_pair stores its side outputs. The rows are padded by two so that the TG_OWN
// frames of one bin fall on different LDS banks.
constexpr int TG_FR = 3 * TG_OWN;
constexpr int TG_WAVES = TG_FR / 4;
constexpr int TG_THREADS = 64 * TG_WAVES;
constexpr int TG_RS = M256 + 2;
constexpr int TG_NI = (NBIN * TG_OWN + TG_THREADS - 1) / TG_THREADS;
static_assert(TG_OWN % 4 == 0, "a wave's four transforms are of one kind");
static_assert(TG_THREADS >= 2 * HOP && TG_THREADS >= 2 * 4 * (TG_OWN + 4), "prologue thread ranges");

// bin k in [1, 256) of the real transform from the half-length transform Z (k_stft_gate's split step)
__device__ __forceinline__ float2 tg_split(const float2* row, int k, float2 w) {
  const float2 zk = row[k], zm = conjf2(row[M256 - k]);
  const float2 E = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y + zm.y));
  const float2 Dd = csub(zk, zm);
  const float2 O = make_float2(0.5f * Dd.y, -0.5f * Dd.x);
  return cadd(E, cmul(w, O));
}

__global__ __launch_bounds__(TG_THREADS) void k_tail_grad_masks(TailGradArgs a) {
  __shared__ float2 tw[256];
  __shared__ float2 rows[TG_FR][TG_RS];
  __shared__ float2 wins[2][M256];       // spec_output window, inv_spec window (as sample pairs)
  __shared__ float inv_env[2][HOP];      // 1 / env of a segment between two frames, of the segment after the last frame
  __shared__ float w1s[TG_NW1];
  __shared__ float gys[2][4][TG_OWN + 4];  // g_y of frames f0 - 2 .. f0 + TG_OWN + 1, zero outside [0, T)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, f0 = blockIdx.y * TG_OWN;
  const int T = a.T, N = a.N;
  const bool sep = a.g_sep != nullptr, vad = a.g_vad != nullptr;
  if (tid < 256) {
    tw[tid] = a.tw[tid];
    wins[0][tid] = reinterpret_cast<const float2*>(a.win_x)[tid];
    wins[1][tid] = reinterpret_cast<const float2*>(a.win_inv)[tid];
  } else if (tid < 2 * HOP) {  // k_istft_pair's inv_mid and inv_last
    const int q = tid - HOP;
    const float w0 = a.win_inv[q], w1 = a.win_inv[q + HOP];
    inv_env[0][q] = 1.f / (w0 * w0 + w1 * w1);
    inv_env[1][q] = 1.f / (w1 * w1);
  }
  if (vad) {
    for (int i = tid; i < TG_NW1; i += TG_THREADS) w1s[i] = (float)a.vw[i];
    if (tid < 2 * 4 * (TG_OWN + 4)) {
      const int so = tid / (TG_OWN + 4), q = tid % (TG_OWN + 4), f = f0 - 2 + q;
      gys[so >> 2][so & 3][q] = (f >= 0 && f < T) ? a.gy[((size_t)b * 8 + so) * T + f] : 0.f;
    }
  }
  // the masks of this thread's elements, in flight during the transforms
  float mr[2][TG_NI];
#pragma unroll
  for (int j = 0; j < TG_NI; ++j) {
    const int i = tid + j * TG_THREADS, k = i / TG_OWN, f = f0 + i % TG_OWN;
    const bool ok = i < NBIN * TG_OWN && f < T;
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) mr[sp][j] = ok ? a.masks[(((size_t)b * 2 + sp) * NBIN + k) * T + f] : 0.f;
  }
  lds_sync();
  if (sep) {
    const int t = 4 * wave + (lane >> 4), kind = t / TG_OWN, c = lane & 15;
    const int fc = min(f0 + t % TG_OWN, T - 1);  // frames past the end transform frame T - 1 (in bounds, unused)
    float2* row = rows[t];
    float2 x[16];
    if (kind == 0) {  // the front end's frame: reflect padding of HOP on both sides, spec_output window
      const float* xb = a.x + (size_t)b * a.ldx;
      const float2* winc = wins[0] + c;
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        int s0 = (fc - 1) * HOP + 2 * (16 * n1 + c), s1 = s0 + 1;
        s0 = s0 < 0 ? -s0 : (s0 >= N ? 2 * (N - 1) - s0 : s0);
        s1 = s1 < 0 ? -s1 : (s1 >= N ? 2 * (N - 1) - s1 : s1);
        const float2 w = winc[16 * n1];
        x[n1] = make_float2(w.x * xb[s0], w.y * xb[s1]);
      }
    } else {
      const float* g = a.g_sep + (long long)b * a.gs_b + (long long)(kind - 1) * a.gs_s;
      const float2* winc = wins[1] + c;
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        const int j0 = 2 * (16 * n1 + c);        // frame samples j0, j0 + 1 (one segment: HOP is even)
        const int i0 = (fc - 1) * HOP + j0;      // their place in g_sep (the centre padding is HOP)
        const int q = j0 & (HOP - 1);
        const float* ie = inv_env[fc + (j0 >= HOP ? 1 : 0) < T ? 0 : 1];
        const float v0 = (i0 >= 0 && i0 < N) ? g[(long long)i0 * a.gs_n] * ie[q] : 0.f;
        const float v1 = (i0 + 1 >= 0 && i0 + 1 < N) ? g[(long long)(i0 + 1) * a.gs_n] * ie[q + 1] : 0.f;
        const float2 w = winc[16 * n1];
        x[n1] = make_float2(w.x * v0, w.y * v1);
      }
    }
    rfft512_regs(x, row, tw, c);
  }
  lds_sync();
#pragma unroll
  for (int j = 0; j < TG_NI; ++j) {
    const int i = tid + j * TG_THREADS, k = i / TG_OWN, fo = i % TG_OWN, f = f0 + fo;
    if (i >= NBIN * TG_OWN || f >= T) continue;
    float gm[2] = {0.f, 0.f};
    if (sep && k > 0) {  // the DC row of X is zero: bin 0 receives the VAD term only
      const float2* rx = rows[fo];
      if (k == M256) {   // Nyquist: E[0] - O[0], real; c_256 / 512
        const float X = rx[0].x - rx[0].y;
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
          const float2 z = rows[(1 + sp) * TG_OWN + fo][0];
          gm[sp] = X * ((z.x - z.y) * (1.f / 512.f));
        }
      } else {
        const float2 w = tw[k];
        const float2 X = tg_split(rx, k, w);
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
          const float2 U = tg_split(rows[(1 + sp) * TG_OWN + fo], k, w);
          gm[sp] = (X.x * U.x + X.y * U.y) * (1.f / 256.f);
        }
      }
    }
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
      const float m = sigmoid_f(mr[sp][j]);
      float g = gm[sp] * (m * (1.f - m));
      if (vad) {  // the transposed conv1_1: sum_o sum_kk w1[o][k][kk] g_y[o][f - kk + 2]
        float v = 0.f;
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
          for (int kk = 0; kk < 5; ++kk) v = fmaf(w1s[(o * NBIN + k) * 5 + kk], gys[sp][o][fo - kk + 4], v);
        g += v;
      }
      st_out(a.g_masks + (((size_t)b * 2 + sp) * NBIN + k) * T + f, g);
    }
  }
}

hipError_t launch_tail_grad(const TailGradArgs& a, hipStream_t s) {
  if (a.B < 1 || a.N <= HOP || a.T != 1 + a.N / HOP) return hipErrorInvalidValue;
  const int BS = 2 * a.B;
  if (a.g_vad) {
    hipLaunchKernelGGL(k_tail_feat, dim3(BS, (a.T + TF_ROWS - 1) / TF_ROWS), dim3(64 * TF_NW), 0, s, a);
    hipLaunchKernelGGL(k_vad_grad, dim3(BS), dim3(TV_THREADS), 0, s, a);
    if (a.gpar) {
      hipLaunchKernelGGL(k_vad_grad_w1, dim3(BS, (NBIN + TW_CPW - 1) / TW_CPW, tg_w1_chunks(a.T)), dim3(TV_THREADS), 0, s, a);
      hipLaunchKernelGGL(k_tail_param_finish, dim3((TG_NPAR + TP_PAR - 1) / TP_PAR), dim3(TV_THREADS), 0, s, a);
    }
  }
  if (a.g_masks && (a.g_sep || a.g_vad))
    hipLaunchKernelGGL(k_tail_grad_masks, dim3(a.B, (a.T + TG_OWN - 1) / TG_OWN), dim3(TG_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace sepvad
