// Reverberant scene simulation on the device (reference create_data/create_simulation_data.py): batched
// image-method responses (create_data/rirgen.cpp:200-351), truncated linear convolution (np.convolve(...)[:cut],
// :482-500), mixing at an SNR with min-max normalisation (:558-620, :707-713) and frame-level VAD labels
// (create_data/vad_labels2stft_labels.py:14-23,47-66). Ordinary launches, fixed-order sums, no atomics: every result
// is bitwise reproducible and independent of the batch around its row. This object is built without FMA
// contraction (Makefile); the convolution asks for its fused multiply-adds explicitly.
#include <string>

#include "device_common.h"
#include "handle.h"

namespace sepvad {
namespace {

constexpr double kPi = 3.14159265358979323846;

// ---- image-method responses ---------------------------------------------------------------------------------
constexpr int RIR_T = 256;     // threads per workgroup == output samples per tile
constexpr int RIR_LIST = 512;  // image records held in LDS between two summation passes

struct RirRec {
  double gain, frac, sp, cb, sb;  // gain; dist - floor(dist); sin(pi frac); cos / sin(2 pi frac / Tw)
  int start, pad;                 // output sample of tap 0
};

// Polar-pattern gain of a directional microphone (rir.hip mic_gain).
__device__ double rir_mic_gain(double x, double y, double z, const double* angle, int mtype) {
  double rho;
  switch (mtype) {
    case 'b': rho = 0.0; break;
    case 'h': rho = 0.25; break;
    case 'c': rho = 0.5; break;
    case 's': rho = 0.75; break;
    default: return 1.0;
  }
  const double vartheta = acos(z / sqrt(x * x + y * y + z * z));
  const double varphi = atan2(y, x);
  const double gain = sin(kPi / 2 - angle[1]) * sin(vartheta) * cos(angle[0] - varphi) +
                      cos(kPi / 2 - angle[1]) * cos(vartheta);
  return rho + (1 - rho) * gain;
}

__global__ __launch_bounds__(RIR_T) void k_rir(const SepVadRirJob* __restrict__ jobs, double* __restrict__ h,
                                               long long ld, int tiles) {
  __shared__ RirRec rec[RIR_LIST];
  __shared__ double wcs[2 * SEPVAD_RIR_MAX_TW];  // cos, sin of 2 pi (n + 1) / Tw
  __shared__ int wcnt[2][RIR_T / 64];
  const int job = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const SepVadRirJob& J = jobs[job];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long sm = (long long)tile * RIR_T + tid;  // this thread's output sample
  double* hrow = h + (long long)job * ld;

  // the table is trusted only as far as it stays inside the caps sepvad_rir_jobs_prepare enforces
  const int Tw = J.Tw;
  long long n = J.n_samples < 0 ? 0 : J.n_samples;
  if (n > ld) n = ld;
  const int n1 = J.n1, n2 = J.n2, n3 = J.n3;
  bool ok = Tw >= 0 && Tw <= SEPVAD_RIR_MAX_TW && n1 >= 0 && n2 >= 0 && n3 >= 0 && n1 <= 1000000 && n2 <= 1000000 &&
            n3 <= 1000000;
  const long long d1 = 2LL * n1 + 1, d2 = 2LL * n2 + 1, d3 = 2LL * n3 + 1;
  long long total = 0;
  if (ok) {
    const double im = 8.0 * (double)d1 * (double)d2 * (double)d3;
    ok = im <= (double)SEPVAD_RIR_MAX_IMAGES;
    total = ok ? 8 * d1 * d2 * d3 : 0;
  }
  const long long t0 = (long long)tile * RIR_T;
  if (!ok || t0 >= n) {  // nothing of the response in this tile: the zeroed rest of the row
    if (sm < ld) hrow[sm] = 0.0;
    return;
  }
  const long long t1 = t0 + RIR_T < n ? t0 + RIR_T : n;
  for (int i = tid; i < Tw; i += RIR_T) {
    const double a = 2 * kPi * ((double)(i + 1) / Tw);
    wcs[i] = cos(a);
    wcs[SEPVAD_RIR_MAX_TW + i] = sin(a);
  }
  const double ns = (double)J.n_samples;
  const int order = J.order, half = Tw / 2;
  const double s0 = J.s[0], s1 = J.s[1], s2 = J.s[2], r0 = J.r[0], r1 = J.r[1], r2 = J.r[2];
  const double L0 = J.L[0], L1 = J.L[1], L2 = J.L[2];
  double acc = 0.0;
  int count = 0, par = 0;

  auto flush = [&]() {
    __syncthreads();
    if (sm < t1) {
      for (int e = 0; e < count; ++e) {
        const long long nn = sm - rec[e].start;
        if (nn >= 0 && nn < Tw) {
          const int m = (int)nn + 1 - half;
          const double t = (double)m - rec[e].frac;
          // sin(pi (m - frac)) = -(-1)^m sin(pi frac)
          const double sinc = t == 0.0 ? 1.0 : ((m & 1) ? rec[e].sp : -rec[e].sp) / (kPi * t);
          const double cosv = wcs[nn] * rec[e].cb + wcs[SEPVAD_RIR_MAX_TW + nn] * rec[e].sb;
          acc += rec[e].gain * (0.5 * (1 - cosv) * sinc);
        }
      }
    }
    __syncthreads();
    count = 0;
  };

  const unsigned e2 = (unsigned)d2, e3 = (unsigned)d3;  // total <= SEPVAD_RIR_MAX_IMAGES: 32-bit lattice indices
  for (unsigned base = 0; base < (unsigned)total; base += RIR_T) {
    const unsigned idx = base + tid;
    bool touch = false;
    double dist = 0, fdist = 0, px = 0, py = 0, pz = 0;
    int mx = 0, my = 0, mz = 0, q = 0, j = 0, k = 0;
    if (idx < (unsigned)total) {
      k = (int)(idx & 1); j = (int)((idx >> 1) & 1); q = (int)((idx >> 2) & 1);
      unsigned rest = idx >> 3;
      mz = (int)(rest % e3) - n3; rest /= e3;
      my = (int)(rest % e2) - n2;
      mx = (int)(rest / e2) - n1;
      // the deciders, in the host's operation order with every product and sum rounded on its own
      const double Rmx = __dmul_rn((double)(2 * mx), L0), Rmy = __dmul_rn((double)(2 * my), L1),
                   Rmz = __dmul_rn((double)(2 * mz), L2);
      px = __dadd_rn(__dsub_rn((double)(1 - 2 * q) * s0, r0), Rmx);
      py = __dadd_rn(__dsub_rn((double)(1 - 2 * j) * s1, r1), Rmy);
      pz = __dadd_rn(__dsub_rn((double)(1 - 2 * k) * s2, r2), Rmz);
      dist = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(px, px), __dmul_rn(py, py)), __dmul_rn(pz, pz)));
      const bool in_order = order == -1 || abs(2 * mx - q) + abs(2 * my - j) + abs(2 * mz - k) <= order;
      fdist = floor(dist);
      if (in_order && fdist < ns) {
        const long long start = (long long)fdist - half + 1;
        touch = start < t1 && start + Tw > t0;
      }
    }
    const unsigned long long bal = __ballot(touch);
    if (lane == 0) wcnt[par][wv] = __popcll(bal);
    __syncthreads();
    int off = count, tot = 0;
#pragma unroll
    for (int w = 0; w < RIR_T / 64; ++w) {
      const int c = wcnt[par][w];
      off += w < wv ? c : 0;
      tot += c;
    }
    par ^= 1;
    if (touch) {
      const int e = off + __popcll(bal & ((1ULL << lane) - 1ULL));
      const double gx = pow(J.beta[0], (double)abs(mx - q)) * pow(J.beta[1], (double)abs(mx));
      const double gy = pow(J.beta[2], (double)abs(my - j)) * pow(J.beta[3], (double)abs(my));
      const double gz = pow(J.beta[4], (double)abs(mz - k)) * pow(J.beta[5], (double)abs(mz));
      const double frac = dist - fdist;
      const double b = 2 * kPi * (frac / Tw);
      rec[e].gain = rir_mic_gain(px, py, pz, J.angle, J.mic_type) * gx * gy * gz / (4 * kPi * dist * J.cTs);
      rec[e].frac = frac;
      rec[e].sp = sin(kPi * frac);
      rec[e].cb = cos(b);
      rec[e].sb = sin(b);
      rec[e].start = (int)fdist - half + 1;
    }
    count += tot;
    if (count > RIR_LIST - RIR_T) flush();
  }
  flush();
  if (sm < ld) hrow[sm] = sm < t1 ? acc : 0.0;
}

// The reference's high-pass (rirgen.cpp:335-349), in place: 10^4 dependent steps, one lane per job.
__global__ __launch_bounds__(64) void k_rir_highpass(const SepVadRirJob* __restrict__ jobs, int n_jobs,
                                                     double* __restrict__ h, long long ld) {
  const int job = blockIdx.x * 64 + threadIdx.x;
  if (job >= n_jobs) return;
  const SepVadRirJob& J = jobs[job];
  if (J.high_pass != 1) return;
  long long n = J.n_samples < 0 ? 0 : J.n_samples;
  if (n > ld) n = ld;
  const double B1 = J.hp[0], B2 = J.hp[1], A1 = J.hp[2], R1 = J.hp[3];
  double* row = h + (long long)job * ld;
  double y0 = 0, y1 = 0, y2 = 0;
  for (long long i = 0; i < n; ++i) {
    const double x0 = row[i];
    y2 = y1;
    y1 = y0;
    y0 = __dadd_rn(__dadd_rn(__dmul_rn(B1, y1), __dmul_rn(B2, y2)), x0);
    row[i] = __dadd_rn(__dadd_rn(y0, __dmul_rn(A1, y1)), __dmul_rn(R1, y2));
  }
}

// ---- truncated linear convolution ---------------------------------------------------------------------------
// One workgroup per (row, FC_TILE outputs); thread t owns the FC_P consecutive outputs n0 + FC_P t + i. Taps are
// taken FC_SK at a time: their h values and the x span they need are staged in LDS as doubles, then each thread runs
// through them eight taps at a time with a sliding register window of 15 x values (8 loads per 64 FMAs). The x span is
// stored with one pad double per eight, so the threads' stride-8 reads fall on distinct banks. An output's sum is one
// fma chain over k ascending; taps outside the row (k >= K_r, x index < 0 or >= Nx) add an exact zero.
constexpr int FC_T = 256, FC_P = 8, FC_TILE = FC_T * FC_P;  // 2048 outputs per workgroup
constexpr int FC_SK = 512;                                  // taps per staging step
constexpr int FC_XS = FC_TILE + FC_SK;                      // x elements staged per step

struct FirArgs {
  const float* x; long long x_ld, Nx;
  const double* h; long long h_ld; int K;
  const int* klen; const int* xidx; const int* hidx;
  long long L; double* y; long long y_ld; int tiles;
};

__global__ __launch_bounds__(FC_T) void k_fir(FirArgs a) {
  __shared__ double xs[FC_XS / 8 * 9];
  __shared__ double hs[FC_SK];
  const int r = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles, t = threadIdx.x;
  const long long xr = a.xidx ? a.xidx[r] : r, hr = a.hidx ? a.hidx[r] : r;
  const float* x = a.x + xr * a.x_ld;
  const double* h = a.h + hr * a.h_ld;
  int K = a.klen ? a.klen[hr] : a.K;
  K = K < 0 ? 0 : (K > a.K ? a.K : K);
  const long long n0 = (long long)tile * FC_TILE;
  double acc[FC_P];
#pragma unroll
  for (int i = 0; i < FC_P; ++i) acc[i] = 0.0;

  for (int k0 = 0; k0 < K && k0 <= n0 + FC_TILE - 1; k0 += FC_SK) {
    // local element e <-> x index g0 + e; tap k0 + kk of output n0 + 8 t + i reads e = FC_SK + 8 t + i - kk
    const long long g0 = n0 - k0 - FC_SK;
    if (g0 + 1 >= a.Nx) continue;  // the whole span lies at or beyond Nx: zeros
    __syncthreads();
    for (int e = t; e < FC_XS; e += FC_T) {
      const long long g = g0 + e;
      xs[e + (e >> 3)] = (g >= 0 && g < a.Nx) ? (double)x[g] : 0.0;
    }
    for (int e = t; e < FC_SK; e += FC_T) hs[e] = k0 + e < K ? h[k0 + e] : 0.0;
    __syncthreads();
    const int kend = K - k0 < FC_SK ? K - k0 : FC_SK;  // taps of this step that exist
    for (int c = 0; c * 64 < kend; ++c) {
      // rows of eight: element e = 8 R + u sits at 9 R + u
      const int R0 = t + FC_SK / 8 - 1 - 8 * c;  // row of window entries 0..6 at kb = 0 (entry j <-> u = j + 1)
      double xw[15];
#pragma unroll
      for (int j = 7; j < 15; ++j) xw[j] = xs[9 * (R0 + 1) + (j - 7)];
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) {
        // window entry j holds element 8 (R0 - kb) + 1 + j: tap kk = 64 c + 8 kb + u of output i reads entry 7 + i - u
        if (kb > 0) {
#pragma unroll
          for (int j = 14; j >= 8; --j) xw[j] = xw[j - 8];
          xw[7] = xs[9 * (R0 - kb + 1)];
        }
#pragma unroll
        for (int j = 0; j < 7; ++j) xw[j] = xs[9 * (R0 - kb) + 1 + j];
        double hv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) hv[u] = hs[64 * c + 8 * kb + u];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int i = 0; i < FC_P; ++i) acc[i] = fma(hv[u], xw[7 + i - u], acc[i]);
      }
    }
  }
  double* y = a.y + (long long)r * a.y_ld;
#pragma unroll
  for (int i = 0; i < FC_P; ++i) {
    const long long nq = n0 + (long long)FC_P * t + i;
    if (nq < a.L) y[nq] = acc[i];
  }
}

// ---- mixing and normalisation -------------------------------------------------------------------------------
constexpr int MX_T = 1024;
constexpr int MX_MAX_S = 8;

struct MixArgs {
  const double* rev; int B, S; long long L;
  const float* noise; const double* snr; int power_mode;
  double a, b; float* mix; double* stats;
};

__device__ __forceinline__ double block_min(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) s = fmin(s, red[i]);
  return s;
}

__device__ __forceinline__ double mixed_at(const double* rev, int S, long long L, long long i) {
  double m = rev[i];
  for (int s = 1; s < S; ++s) m += rev[(long long)s * L + i];
  return m;
}

__global__ __launch_bounds__(MX_T) void k_scene_mix(MixArgs a) {
  __shared__ double red[16];
  const int b = blockIdx.x, t = threadIdx.x;
  const long long L = a.L;
  const double* rev = a.rev + (long long)b * a.S * L;
  const float* nz = a.noise ? a.noise + (long long)b * L : nullptr;
  double gain = 0.0;
  const double snr = nz ? a.snr[b] : 0.0;
  const bool noisy = nz != nullptr && snr == snr;
  if (noisy) {
    const double Nd = (double)L;
    double mm = 0.0, mn = 0.0;
    if (a.power_mode == 0) {  // numpy's std: the mean, then the centred squares
      double sm = 0.0, sn = 0.0;
      for (long long i = t; i < L; i += MX_T) { sm += mixed_at(rev, a.S, L, i); sn += (double)nz[i]; }
      mm = block_sum(sm, red) / Nd;
      mn = block_sum(sn, red) / Nd;
    }
    double qm = 0.0, qn = 0.0;
    for (long long i = t; i < L; i += MX_T) {
      const double dm = mixed_at(rev, a.S, L, i) - mm, dn = (double)nz[i] - mn;
      qm += dm * dm;
      qn += dn * dn;
    }
    const double vm = block_sum(qm, red) / Nd, vn = block_sum(qn, red) / Nd;
    if (a.power_mode == 0) {
      const double sdm = sqrt(vm), sdn = sqrt(vn);
      gain = sqrt(pow(10.0, -snr / 10) * (sdm * sdm) / (sdn * sdn));
    } else {
      gain = sqrt(vm / (vn * pow(10.0, snr / 10)));
    }
  }
  double lo = INFINITY, hi = -INFINITY;
  for (long long i = t; i < L; i += MX_T) {
    double v = mixed_at(rev, a.S, L, i);
    if (noisy) v += gain * (double)nz[i];
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
  lo = block_min(lo, red);
  hi = -block_min(-hi, red);
  const double span = hi - lo;
  float* out = a.mix + (long long)b * L;
  for (long long i = t; i < L; i += MX_T) {
    double v = mixed_at(rev, a.S, L, i);
    if (noisy) v += gain * (double)nz[i];
    out[i] = (float)(a.a * (v - lo) / span - a.b);
  }
  if (t == 0 && a.stats) {
    double* st = a.stats + 4LL * b;
    st[0] = gain; st[1] = lo; st[2] = hi; st[3] = a.a / span;
  }
}

struct TargetArgs {
  const double* dry; int S; long long L; int mode; double a, b; const double* stats; float* out;
};

__global__ __launch_bounds__(MX_T) void k_scene_targets(TargetArgs a) {
  __shared__ double red[16];
  const int row = blockIdx.x, t = threadIdx.x;
  const double* d = a.dry + (long long)row * a.L;
  float* out = a.out + (long long)row * a.L;
  if (a.mode == 1) {
    const double sc = a.stats[4LL * (row / a.S) + 3];
    for (long long i = t; i < a.L; i += MX_T) out[i] = (float)(sc * d[i]);
    return;
  }
  double lo = INFINITY, hi = -INFINITY;
  for (long long i = t; i < a.L; i += MX_T) { lo = fmin(lo, d[i]); hi = fmax(hi, d[i]); }
  lo = block_min(lo, red);
  hi = -block_min(-hi, red);
  const double span = hi - lo;
  for (long long i = t; i < a.L; i += MX_T) out[i] = (float)(a.a * (d[i] - lo) / span - a.b);
}

// ---- frame-level VAD labels ---------------------------------------------------------------------------------
struct VadFrameArgs {
  const uint8_t* act; long long act_ld; int R; long long L; int edge_mode; int T; float* out;
};

__global__ __launch_bounds__(256) void k_vad_frames(VadFrameArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)a.R * a.T) return;
  const int r = (int)(g / a.T), j = (int)(g % a.T);
  const uint8_t* row = a.act + (long long)r * a.act_ld;
  long long beg, len = 512;
  int cnt[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) cnt[q] = 0;
  if (j == 0) { beg = 0; len = 256; }
  else if (j == a.T - 1) { beg = a.L - 256; len = 256; }
  else beg = 256LL * (j - 1);
  if (len == 256 && a.edge_mode == 0) cnt[0] = 256;
  for (long long i = 0; i < len; ++i) {
    const int v = row[beg + i];
#pragma unroll
    for (int q = 0; q < 9; ++q) cnt[q] += v == q;
  }
  int best = 0, most = cnt[0];  // the lowest value wins ties
#pragma unroll
  for (int q = 1; q < 9; ++q)
    if (cnt[q] > most) { most = cnt[q]; best = q; }
  a.out[g] = (float)best;
}

}  // namespace
}  // namespace sepvad

using namespace sepvad;

extern "C" {

int64_t sepvad_rir_scratch_bytes(int32_t n_jobs, int64_t ld) {
  if (n_jobs < 1 || n_jobs > 65535 || ld < 1) return fail(SEPVAD_E_ARG, "sepvad_rir_scratch_bytes: need 1 <= n_jobs <= 65535, ld >= 1");
  return 0;
}

int32_t sepvad_rir_generate_device(const SepVadRirJob* jobs, int32_t n_jobs, double* h, int64_t ld, void* scratch,
                                   int64_t scratch_bytes, void* stream) {
  (void)scratch;
  if (!jobs || !h) return fail(SEPVAD_E_ARG, "sepvad_rir_generate_device: null pointer");
  if (n_jobs < 1 || n_jobs > 65535 || ld < 1) return fail(SEPVAD_E_ARG, "sepvad_rir_generate_device: need 1 <= n_jobs <= 65535, ld >= 1");
  if (scratch_bytes < 0) return fail(SEPVAD_E_ARG, "sepvad_rir_generate_device: negative scratch size");
  const long long tiles = (ld + RIR_T - 1) / RIR_T;
  if (tiles * n_jobs > INT32_MAX) return fail(SEPVAD_E_ARG, "sepvad_rir_generate_device: n_jobs * ld too large");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rir, dim3((unsigned)(tiles * n_jobs)), dim3(RIR_T), 0, s, jobs, h, (long long)ld, (int)tiles);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_rir_highpass, dim3((n_jobs + 63) / 64), dim3(64), 0, s, jobs, n_jobs, h, (long long)ld);
  HIPRET(hipGetLastError());
}

int32_t sepvad_fir_convolve(const float* x, int64_t x_ld, int64_t Nx, const double* h, int64_t h_ld, int32_t K,
                            const int32_t* klen, const int32_t* xidx, const int32_t* hidx, int32_t R, int64_t L,
                            double* y, int64_t y_ld, void* stream) {
  if (!x || !h || !y) return fail(SEPVAD_E_ARG, "sepvad_fir_convolve: null pointer");
  if (R < 1 || L < 1 || Nx < 1 || K < 1 || x_ld < Nx || h_ld < K || y_ld < L)
    return fail(SEPVAD_E_ARG, "sepvad_fir_convolve: need R, L, Nx, K >= 1 and row strides >= the row lengths");
  const long long tiles = (L + FC_TILE - 1) / FC_TILE;
  if (tiles * R > INT32_MAX) return fail(SEPVAD_E_ARG, "sepvad_fir_convolve: R * L too large");
  FirArgs a{x, x_ld, Nx, h, h_ld, K, klen, xidx, hidx, L, y, y_ld, (int)tiles};
  hipLaunchKernelGGL(k_fir, dim3((unsigned)(tiles * R)), dim3(FC_T), 0, (hipStream_t)stream, a);
  HIPRET(hipGetLastError());
}

int32_t sepvad_scene_mix(const double* rev, int32_t B, int32_t S, int64_t L, const float* noise,
                         const double* snr_db, int32_t power_mode, double a, double b, float* mix, double* stats,
                         void* stream) {
  if (!rev || !mix) return fail(SEPVAD_E_ARG, "sepvad_scene_mix: null pointer");
  if (B < 1 || S < 1 || S > MX_MAX_S || L < 1) return fail(SEPVAD_E_ARG, "sepvad_scene_mix: need B >= 1, 1 <= S <= 8, L >= 1");
  if ((noise == nullptr) != (snr_db == nullptr)) return fail(SEPVAD_E_ARG, "sepvad_scene_mix: noise and snr_db go together");
  if (power_mode != 0 && power_mode != 1) return fail(SEPVAD_E_ARG, "sepvad_scene_mix: power_mode must be 0 or 1");
  MixArgs m{rev, B, S, L, noise, snr_db, power_mode, a, b, mix, stats};
  hipLaunchKernelGGL(k_scene_mix, dim3(B), dim3(MX_T), 0, (hipStream_t)stream, m);
  HIPRET(hipGetLastError());
}

int32_t sepvad_scene_targets(const double* dry, int32_t B, int32_t S, int64_t L, int32_t mode, double a, double b,
                             const double* stats, float* out, void* stream) {
  if (!dry || !out) return fail(SEPVAD_E_ARG, "sepvad_scene_targets: null pointer");
  if (B < 1 || S < 1 || S > MX_MAX_S || L < 1) return fail(SEPVAD_E_ARG, "sepvad_scene_targets: need B >= 1, 1 <= S <= 8, L >= 1");
  if (mode != 0 && mode != 1) return fail(SEPVAD_E_ARG, "sepvad_scene_targets: mode must be 0 or 1");
  if (mode == 1 && !stats) return fail(SEPVAD_E_ARG, "sepvad_scene_targets: mode 1 needs the mixture's stats");
  if ((long long)B * S > INT32_MAX) return fail(SEPVAD_E_ARG, "sepvad_scene_targets: B * S too large");
  TargetArgs t{dry, S, L, mode, a, b, stats, out};
  hipLaunchKernelGGL(k_scene_targets, dim3(B * S), dim3(MX_T), 0, (hipStream_t)stream, t);
  HIPRET(hipGetLastError());
}

int32_t sepvad_vad_frame_labels(const uint8_t* act, int64_t act_ld, int32_t R, int64_t L, int32_t edge_mode,
                                float* out, void* stream) {
  if (!act || !out) return fail(SEPVAD_E_ARG, "sepvad_vad_frame_labels: null pointer");
  if (R < 1 || L < 512 || L % 512 != 0 || act_ld < L || L > (1LL << 30))
    return fail(SEPVAD_E_ARG, "sepvad_vad_frame_labels: need R >= 1, L a multiple of 512 and act_ld >= L");
  if (edge_mode != 0 && edge_mode != 1) return fail(SEPVAD_E_ARG, "sepvad_vad_frame_labels: edge_mode must be 0 or 1");
  const int T = (int)(2 * L / 512 + 1);
  const long long blocks = ((long long)R * T + 255) / 256;
  if (blocks > INT32_MAX) return fail(SEPVAD_E_ARG, "sepvad_vad_frame_labels: R * T too large");
  VadFrameArgs v{act, act_ld, R, L, edge_mode, T, out};
  hipLaunchKernelGGL(k_vad_frames, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, v);
  HIPRET(hipGetLastError());
}

}  // extern "C"
