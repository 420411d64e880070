// The output head with a backward (model/model.py:322-325,357): TCN.output = PReLU -> GroupNorm(1, 256, eps 1e-5) ->
// weight-normed Conv1d(256 -> 514, 1). Forward: from the trunk output y [B][256][T] to masks_b [B][514][T]. Backward: from
// G = dL/dmasks_b to dL/dy and to the gradients of the folded parameters (W, bias, gamma, beta, alpha). No forward kernel
// is touched and nothing a forward left behind is read; DESIGN.md section 16 has the derivation.
//
//   p = y > 0 ? y : alpha y;  zh = (p - mu) r;  z = gamma_c zh + beta_c;  M = W z + bias
//   dbias = sum G;  dW = sum G z^T;  dz = W^T G;  dgamma_c = sum dz zh;  dbeta_c = sum dz
//   h = gamma_c dz;  a1 = mean h;  a2 = mean h zh;  dp = r (h - a1 - zh a2);  dy = dp (y > 0 ? 1 : alpha)
//   dalpha = sum [y <= 0] dp y
//
// The three products W z, W^T G and G z^T run on v_mfma_f64_16x16x4_f64 in one tile routine, hg_tile: 64 x 64 outputs per
// workgroup, four waves of 32 x 32 (2 x 2 blocks of 16 x 16 per wave), K in chunks of 64 through LDS. The operands are
// float32 data (G, z) or the folded weight in double; they are widened as they are read from LDS, so every product is
// exact and every sum is a double sum: the rounding left in a result is its own conversion to float32 (DESIGN.md
// section 16 has the reason: the PReLU slope's gradient is one number, and only a correctly rounded result meets a gate
// taken from another float32 computation's error on it). Everything that is not a product (the GroupNorm statistics,
// z, the per-channel sums, a1 and a2, dp, the parameter sums) is double arithmetic as well. No atomics: every sum over
// time or over the batch is written as per-workgroup partials and added by one thread in index order, so the results
// are bitwise reproducible, utterance b's g_y depends on its own rows only, and G is read through its strides, so
// nothing depends on them.
#include "device_common.h"

namespace sepvad {

typedef double hg_f64x4 __attribute__((ext_vector_type(4)));

constexpr int HG_K = 64;          // K chunk of the tile routine
constexpr int HG_LD = HG_K + 1;   // elements per LDS row
constexpr int HG_NE = HG_TILE * HG_K / 256;   // operand elements per thread and chunk
constexpr double HG_EPS = 1e-5;
static_assert(HG_TILE == 64 && HG_W_T % HG_K == 0 && HG_K % 4 == 0, "tile shapes");

template <typename TA, typename TB>
struct HgSmem {
  TA A[HG_TILE][HG_LD];   // [output index][k]
  TB B[HG_TILE][HG_LD];
};

// One operand of a tile: element (i, k) is p[i si + k sk] for i < ni and k < nk, zero otherwise.
template <typename TE>
struct HgView {
  const TE* p;
  long long si, sk;
  int ni, nk;
};

// Thread -> (i, k) of its e-th element of a chunk. KC: k runs fastest over the lanes (k is the contiguous index in
// memory), otherwise i does. Either way the same value lands in the same LDS slot.
template <bool KC, typename TE>
__device__ __forceinline__ void hg_gather(const HgView<TE>& v, int k0, TE (&r)[HG_NE], int tid) {
#pragma unroll
  for (int e = 0; e < HG_NE; ++e) {
    const int q = tid + 256 * e;
    const int i = KC ? q >> 6 : q & 63, k = k0 + (KC ? q & 63 : q >> 6);
    const bool ok = i < v.ni && k < v.nk;
    r[e] = ok ? v.p[(long long)i * v.si + (long long)k * v.sk] : (TE)0;
  }
}
template <bool KC, typename TE>
__device__ __forceinline__ void hg_stage(TE (*S)[HG_LD], const TE (&r)[HG_NE], int tid) {
#pragma unroll
  for (int e = 0; e < HG_NE; ++e) {
    const int q = tid + 256 * e;
    S[KC ? q >> 6 : q & 63][KC ? q & 63 : q >> 6] = r[e];
  }
}

// C[i][j] = sum_{k < K} A(i, k) B(j, k) for the workgroup's 64 x 64 tile (256 threads). Wave (wr, wc) owns rows
// 32 wr .. + 31 and columns 32 wc .. + 31 as 2 x 2 blocks; acc[bi][bj][r] is row hg_row(bi, r) and column hg_col(bj)
// (the f64 form's own map: column = lane & 15, row = (lane >> 4) + 4 r). The next chunk's operands are in flight
// during the MFMAs of the current one.
__device__ __forceinline__ int hg_row(int bi, int r) {
  const int lane = threadIdx.x & 63, wr = threadIdx.x >> 7;
  return wr * 32 + bi * 16 + (lane >> 4) + 4 * r;
}
__device__ __forceinline__ int hg_col(int bj) {
  const int lane = threadIdx.x & 63, wc = (threadIdx.x >> 6) & 1;
  return wc * 32 + bj * 16 + (lane & 15);
}

template <bool KCA, bool KCB, typename TA, typename TB>
__device__ __forceinline__ void hg_tile(HgSmem<TA, TB>& sm, const HgView<TA>& A, const HgView<TB>& B, int K,
                                        hg_f64x4 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[bi][bj][r] = 0.0;
  TA ra[HG_NE];
  TB rb[HG_NE];
  hg_gather<KCA>(A, 0, ra, tid);
  hg_gather<KCB>(B, 0, rb, tid);
  const TA* Ab = &sm.A[wr * 32 + (lane & 15)][lane >> 4];
  const TB* Bb = &sm.B[wc * 32 + (lane & 15)][lane >> 4];
  for (int k0 = 0; k0 < K; k0 += HG_K) {
    hg_stage<KCA>(sm.A, ra, tid);
    hg_stage<KCB>(sm.B, rb, tid);
    __syncthreads();
    if (k0 + HG_K < K) {
      hg_gather<KCA>(A, k0 + HG_K, ra, tid);
      hg_gather<KCB>(B, k0 + HG_K, rb, tid);
    }
    const int kn = min(HG_K, K - k0);   // the chunk's columns past kn are zero: whole steps past it are skipped
    for (int kk = 0; kk < kn; kk += 4) {
      const double a0 = (double)Ab[kk], a1 = (double)Ab[16 * HG_LD + kk];
      const double b0 = (double)Bb[kk], b1 = (double)Bb[16 * HG_LD + kk];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ double hg_prelu(double y, double alpha) { return y > 0.0 ? y : alpha * y; }

// sum and sum of squares of p = PReLU(y) over HG_STAT_E elements of one utterance, in double
__global__ __launch_bounds__(256) void k_head_stat_part(HeadArgs a) {
  __shared__ double red[16];
  const int b = blockIdx.y;
  const long long n = (long long)CH * a.T, e0 = (long long)blockIdx.x * HG_STAT_E;
  const float* yb = a.y + (size_t)b * n;
  const double alpha = a.hp[HG_ALPHA];
  double s = 0.0, ss = 0.0;
#pragma unroll 8
  for (int u = 0; u < HG_STAT_E / 256; ++u) {
    const long long e = e0 + u * 256 + threadIdx.x;
    const double p = e < n ? hg_prelu((double)yb[e], alpha) : 0.0;
    s += p;
    ss += p * p;
  }
  s = block_sum(s, red);
  ss = block_sum(ss, red);
  if (threadIdx.x == 0) {
    double* o = a.part_stat + ((size_t)b * gridDim.x + blockIdx.x) * 2;
    o[0] = s; o[1] = ss;
  }
}

// mean and 1 / sqrt(var + eps) (biased variance) of utterance b from its partials, added in index order
__global__ __launch_bounds__(64) void k_head_stat_fin(HeadArgs a, int nchunk) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const double* p = a.part_stat + (size_t)b * nchunk * 2;
  double s = 0.0, ss = 0.0;
  for (int i = 0; i < nchunk; ++i) { s += p[2 * i]; ss += p[2 * i + 1]; }
  const double n = (double)CH * a.T, mu = s / n;
  double var = ss / n - mu * mu;
  if (var < 0.0) var = 0.0;
  a.stat[2 * b] = mu;
  a.stat[2 * b + 1] = 1.0 / sqrt(var + HG_EPS);
}

// z = gamma_c (p - mu) r + beta_c, rounded once to float32: the B operand of the forward and of the weight gradient
__global__ __launch_bounds__(256) void k_head_z(HeadArgs a) {
  const int b = blockIdx.y, T = a.T;
  const long long n = (long long)CH * T;
  const double alpha = a.hp[HG_ALPHA], mu = a.stat[2 * b], r = a.stat[2 * b + 1];
#pragma unroll
  for (int u = 0; u < HG_DY_E / 256; ++u) {
    const long long e = (long long)blockIdx.x * HG_DY_E + u * 256 + threadIdx.x;
    if (e < n) {
      const int c = (int)(e / T);
      const double zh = (hg_prelu((double)a.y[(size_t)b * n + e], alpha) - mu) * r;
      a.z[(size_t)b * n + e] = (float)(a.hp[HG_GAMMA + c] * zh + a.hp[HG_BETA + c]);
    }
  }
}

// masks_b[b][m][t] = sum_c W[m][c] z[b][c][t] + bias[m]: i = m, j = t (lanes along t), k = c
__global__ __launch_bounds__(256) void k_head_fwd(HeadArgs a) {
  __shared__ HgSmem<double, float> sm;
  const int T = a.T, nt = hg_chunks(T, HG_TILE);
  const int b = blockIdx.x / nt, t0 = (blockIdx.x % nt) * HG_TILE, m0 = blockIdx.y * HG_TILE;
  const HgView<double> A{a.hp + (size_t)m0 * CH, CH, 1, MOUT - m0, CH};
  const HgView<float> Bv{a.z + (size_t)b * CH * T + t0, 1, T, T - t0, CH};
  hg_f64x4 acc[2][2];
  hg_tile<true, false>(sm, A, Bv, CH, acc);
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + hg_row(bi, r), t = t0 + hg_col(bj);
        if (m < MOUT && t < T) st_out(a.masks + ((size_t)b * MOUT + m) * T + t, (float)(acc[bi][bj][r] + a.hp[HG_BIAS + m]));
      }
}

// dz[b][c][t] = sum_m W[m][c] G[b][m][t], kept in double: i = c, j = t, k = m (514: eight chunks and one step)
__global__ __launch_bounds__(256) void k_head_dz(HeadArgs a) {
  __shared__ HgSmem<double, float> sm;
  const int T = a.T, nt = hg_chunks(T, HG_TILE);
  const int b = blockIdx.x / nt, t0 = (blockIdx.x % nt) * HG_TILE, c0 = blockIdx.y * HG_TILE;
  const HgView<double> A{a.hp + c0, 1, CH, HG_TILE, MOUT};
  const HgView<float> Bv{a.G + (long long)b * a.g_b + (long long)t0 * a.g_t, a.g_t, a.g_m, T - t0, MOUT};
  hg_f64x4 acc[2][2];
  hg_tile<false, false>(sm, A, Bv, MOUT, acc);
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = c0 + hg_row(bi, r), t = t0 + hg_col(bj);
        if (t < T) a.dz[((size_t)b * CH + c) * T + t] = acc[bi][bj][r];
      }
}

// part_w[b, chunk][m][c] = sum over the chunk's HG_W_T frames of G[b][m][t] z[b][c][t], in double: i = m, j = c, k = t
__global__ __launch_bounds__(256) void k_head_dw(HeadArgs a) {
  __shared__ HgSmem<float, float> sm;
  const int T = a.T, nw = hg_chunks(T, HG_W_T);
  const int b = blockIdx.x / nw, t0 = (blockIdx.x % nw) * HG_W_T, nt = min(HG_W_T, T - t0);
  const int m0 = blockIdx.y * HG_TILE, c0 = blockIdx.z * HG_TILE;
  const HgView<float> A{a.G + (long long)b * a.g_b + (long long)m0 * a.g_m + (long long)t0 * a.g_t, a.g_m, a.g_t, MOUT - m0, nt};
  const HgView<float> Bv{a.z + ((size_t)b * CH + c0) * T + t0, T, 1, HG_TILE, nt};
  hg_f64x4 acc[2][2];
  hg_tile<true, true>(sm, A, Bv, nt, acc);
  double* out = a.part_w + (size_t)blockIdx.x * HG_NW;
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + hg_row(bi, r), c = c0 + hg_col(bj);
        if (m < MOUT) out[(size_t)m * CH + c] = acc[bi][bj][r];
      }
}

// part_red[b][chunk][c] = (sum dz, sum dz zh) over HG_RED_T frames of channel c: a wave per channel, four channels per
// wave, lane -> frame; the lanes' sums by the shuffle tree
__global__ __launch_bounds__(256) void k_head_red(HeadArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x, T = a.T, t0 = blockIdx.y * HG_RED_T, t1 = min(T, t0 + HG_RED_T);
  const double alpha = a.hp[HG_ALPHA], mu = a.stat[2 * b], r = a.stat[2 * b + 1];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = blockIdx.z * 16 + wave * 4 + q;
    const size_t row = ((size_t)b * CH + c) * T;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int u = 0; u < HG_RED_T / 64; ++u) {
      const int t = t0 + 64 * u + lane;
      if (t < t1) {
        const double d = a.dz[row + t];
        s0 += d;
        s1 += d * ((hg_prelu((double)a.y[row + t], alpha) - mu) * r);
      }
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (lane == 0) {
      double* o = a.part_red + (((size_t)b * gridDim.y + blockIdx.y) * CH + c) * 2;
      o[0] = s0; o[1] = s1;
    }
  }
}

// per utterance: the channels' sums over the chunks in chunk order (ub), then a1 = mean h and a2 = mean h zh with
// h = gamma_c dz
__global__ __launch_bounds__(CH) void k_head_mom(HeadArgs a, int nchunk) {
  __shared__ double red[16];
  const int b = blockIdx.x, c = threadIdx.x;
  const double* p = a.part_red + ((size_t)b * nchunk * CH + c) * 2;
  double s0 = 0.0, s1 = 0.0;
  for (int i = 0; i < nchunk; ++i) { s0 += p[(size_t)i * CH * 2]; s1 += p[(size_t)i * CH * 2 + 1]; }
  a.ub[((size_t)b * CH + c) * 2] = s0;
  a.ub[((size_t)b * CH + c) * 2 + 1] = s1;
  const double g = a.hp[HG_GAMMA + c], n = (double)CH * a.T;
  const double S1 = block_sum(g * s0, red), S2 = block_sum(g * s1, red);
  if (c == 0) { a.mom[2 * b] = S1 / n; a.mom[2 * b + 1] = S2 / n; }
}

// dp = r (gamma_c dz - a1 - zh a2), dy = dp (y > 0 ? 1 : alpha), and the workgroup's sum of [y <= 0] dp y
__global__ __launch_bounds__(256) void k_head_dy(HeadArgs a) {
  __shared__ double red[16];
  const int b = blockIdx.y, T = a.T;
  const long long n = (long long)CH * T;
  const double alpha = a.hp[HG_ALPHA], mu = a.stat[2 * b], r = a.stat[2 * b + 1];
  const double a1 = a.mom[2 * b], a2 = a.mom[2 * b + 1];
  double sa = 0.0;
#pragma unroll
  for (int u = 0; u < HG_DY_E / 256; ++u) {
    const long long e = (long long)blockIdx.x * HG_DY_E + u * 256 + threadIdx.x;
    if (e < n) {
      const int c = (int)(e / T);
      const double y = (double)a.y[(size_t)b * n + e];
      const double zh = (hg_prelu(y, alpha) - mu) * r;
      const double dp = r * (a.hp[HG_GAMMA + c] * a.dz[(size_t)b * n + e] - a1 - zh * a2);
      if (!(y > 0.0)) sa += dp * y;
      if (a.g_y) st_out(a.g_y + (size_t)b * n + e, (float)(y > 0.0 ? dp : alpha * dp));
    }
  }
  sa = block_sum(sa, red);
  if (threadIdx.x == 0) a.part_alpha[(size_t)b * gridDim.x + blockIdx.x] = sa;
}

// part_bias[b][m] = sum_t G[b][m][t]: a wave per row
__global__ __launch_bounds__(256) void k_head_dbias(HeadArgs a) {
  const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (m >= MOUT) return;
  const float* g = a.G + (long long)b * a.g_b + (long long)m * a.g_m;
  double s = 0.0;
#pragma unroll 4
  for (int t = lane; t < a.T; t += 64) s += (double)g[(long long)t * a.g_t];
  s = wave_sum(s);
  if (lane == 0) a.part_bias[(size_t)b * MOUT + m] = s;
}

// gpar[i]: a thread per parameter adds its partials in index order (the utterances, and for the weight their chunks);
// the last workgroup adds the PReLU slope's partials (thread j the entries j, j + 256, ..., then the threads' sums)
__global__ __launch_bounds__(256) void k_head_finish(HeadArgs a, int nw, int ndy) {
  __shared__ double red[16];
  if (blockIdx.x == gridDim.x - 1) {
    const long long n = (long long)a.B * ndy;
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) s += a.part_alpha[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) a.gpar[HG_ALPHA] = s;
    return;
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HG_ALPHA) return;
  double s = 0.0;
  if (i < HG_NW) {
    const long long P = (long long)a.B * nw;
    const double* p = a.part_w + i;
#pragma unroll 8
    for (long long q = 0; q < P; ++q) s += p[(size_t)q * HG_NW];
  } else if (i < HG_GAMMA) {
    for (int b = 0; b < a.B; ++b) s += a.part_bias[(size_t)b * MOUT + (i - HG_BIAS)];
  } else {  // gamma: sum dz zh; beta: sum dz
    const int c = i < HG_BETA ? i - HG_GAMMA : i - HG_BETA, which = i < HG_BETA ? 1 : 0;
    for (int b = 0; b < a.B; ++b) s += a.ub[((size_t)b * CH + c) * 2 + which];
  }
  a.gpar[i] = s;
}

static bool head_shape_ok(const HeadArgs& a) { return a.B >= 1 && a.T >= 2; }

// the launches both directions share: the GroupNorm statistics and z
static void launch_head_common(const HeadArgs& a, hipStream_t s) {
  const long long n = (long long)CH * a.T;
  const int ns = hg_chunks(n, HG_STAT_E);
  hipLaunchKernelGGL(k_head_stat_part, dim3(ns, a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_head_stat_fin, dim3((a.B + 63) / 64), dim3(64), 0, s, a, ns);
  hipLaunchKernelGGL(k_head_z, dim3(hg_chunks(n, HG_DY_E), a.B), dim3(256), 0, s, a);
}

hipError_t launch_head_forward(const HeadArgs& a, hipStream_t s) {
  if (!head_shape_ok(a)) return hipErrorInvalidValue;
  launch_head_common(a, s);
  hipLaunchKernelGGL(k_head_fwd, dim3(a.B * hg_chunks(a.T, HG_TILE), MOUT_PAD / HG_TILE), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_head_backward(const HeadArgs& a, hipStream_t s) {
  if (!head_shape_ok(a)) return hipErrorInvalidValue;
  const int nr = hg_chunks(a.T, HG_RED_T), ndy = hg_chunks((long long)CH * a.T, HG_DY_E), nw = hg_chunks(a.T, HG_W_T);
  launch_head_common(a, s);
  hipLaunchKernelGGL(k_head_dz, dim3(a.B * hg_chunks(a.T, HG_TILE), CH / HG_TILE), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_head_red, dim3(a.B, nr, CH / 16), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_head_mom, dim3(a.B), dim3(CH), 0, s, a, nr);
  hipLaunchKernelGGL(k_head_dy, dim3(ndy, a.B), dim3(256), 0, s, a);
  if (a.gpar) {
    hipLaunchKernelGGL(k_head_dbias, dim3((MOUT + 3) / 4, a.B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_head_dw, dim3(a.B * nw, MOUT_PAD / HG_TILE, CH / HG_TILE), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_head_finish, dim3((HG_ALPHA + 255) / 256 + 1), dim3(256), 0, s, a, nw, ndy);
  }
  return hipGetLastError();
}

}  // namespace sepvad
