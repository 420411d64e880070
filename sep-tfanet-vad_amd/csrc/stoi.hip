// Classic STOI on the device (reference model/stoi_metric.py:207-301 `stoi`, extended=False), R signal pairs per call,
// five launches, no host synchronisation; the data-dependent frame count stays in device memory:
//   k_stoi_resample  resample_oct (:48-52): polyphase FIR to 10 kHz of both signals of a pair, taps and accumulation
//                    in double, result stored as float (skipped at 10 kHz: later stages read the inputs in place)
//   k_stoi_energy    remove_silent_frames (:148-156): energy of every windowed clean frame (256 at hop 128 over
//                    range(0, L - 256, 128)), one wave per frame, double
//   k_stoi_mask      (:156-164) dB energies, max, keep when max - 40 - e_i < 0, and the prefix sum of the mask:
//                    kept[k] = index of the k-th kept frame, nkept = K
//   k_stoi_spec      (:166-167 overlap-add, :88-102 stft, :259 band sums) spectrum m of the compacted signals needs
//                    kept frames m-1, m, m+1 only, so the compacted signal is never written: the workgroup rebuilds its
//                    256 samples from the resampled signal, windows them again, runs both 512-point real FFTs in LDS
//                    (double, each as a 256-point complex FFT of even + i odd samples) and writes
//                    tob = sqrt(sum |X|^2) of the 15 bands. M = K - 1 spectra (exclusive end).
//   k_stoi_corr      (:262-300) every band x window of 30 frames: normalise, clip, centre, correlate; d = sum / (15 J).
//                    M < 30 gives exactly 1e-5 (:251-256).
// Extended STOI (ESTOI, extended=True, :177-193,268-271) shares stages 1 to 4 and replaces the last one:
//   k_stoi_ex_corr   every window of 30 frames of both signals: rows (bands) mean- and norm-normalised over the 30
//                    frames, then columns (frames) over the 15 bands, then the sum of products. The reference adds
//                    EPS * randn before each centring; that term is left out here (it moves the value by 1e-15 where
//                    the value is defined at all). A row or column whose norm is zero, exactly or up to the rounding
//                    of its centring (st_ex_normalize), becomes zeros (the reference normalises pure noise there: a
//                    random draw), so an all-zero estimate scores exactly 0.
//   k_stoi_ex_finish adds the per-chunk partials of a pair in order: d = sum / (30 J); 1e-5 where M < 30.
// Everything after the float store of the resampled signal is double: the work is a few MFLOP per pair, far below what
// the traffic costs, and it keeps the result within rounding of the reference's float64 numpy chain. Every reduction
// has a fixed order that depends on the pair alone (bitwise reproducible, independent of R and of the batch).
#include <algorithm>
#include <map>
#include <mutex>

#include "device_common.h"
#include "stoi_design.h"

namespace sepvad {

constexpr int ST_THREADS = 256;
constexpr int ST_TP_MAX = 640;                      // polyphase taps staged in LDS (5 x 117 at 16 kHz)
constexpr int ST_XS_MAX = 2048;                     // inputs of one workgroup's outputs (1020 * 8 / 5 + 117 + 2 at 16 kHz)
constexpr double ST_EPS = 2.220446049250313e-16;    // np.finfo(float).eps

__device__ __forceinline__ long long st_xrow(const StoiArgs& a, int r) { return a.xidx ? a.xidx[r] : r; }
__device__ __forceinline__ long long st_yrow(const StoiArgs& a, int r) { return a.yidx ? a.yidx[r] : r; }
__device__ __forceinline__ const float* st_input(const StoiArgs& a, int r, int s) {
  return s == 0 ? a.X + st_xrow(a, r) * a.x_ld : a.Y + st_yrow(a, r) * a.y_ld;
}
// signal s (0 clean, 1 estimate) of pair r at 10 kHz
__device__ __forceinline__ const float* st_sig(const StoiArgs& a, int r, int s) {
  return a.up == a.down ? st_input(a, r, s) : a.sig + ((size_t)r * 2 + s) * a.Ls;
}

// Outputs per workgroup: ST_RS_U rounds of S = (256 / up) up consecutive outputs; thread t < S computes outputs
// k0 + t + u S, u < ST_RS_U, which share one filter phase (S is a multiple of up), so each tap is read once for
// ST_RS_U accumulators.
constexpr int ST_RS_U = 4;
__host__ __device__ inline int st_rs_round(int up) { return ST_THREADS / up * up; }

__global__ __launch_bounds__(ST_THREADS) void k_stoi_resample(StoiArgs a) {
  __shared__ double tps[ST_TP_MAX];
  __shared__ float xs[ST_XS_MAX];
  const int r = blockIdx.z, s = blockIdx.y, t = threadIdx.x;
  const float* x = st_input(a, r, s);
  // output k: y[k] = up * sum_i w[c - i up] x[i], c = half + k down; with ph = c % up, i0 = c / up this is
  // sum_q tp[ph][q] x[i0 - q], accumulated in double in the order of q. The workgroup's outputs read inputs
  // i_lo .. i_lo + span - 1, staged once (zero outside [0, N): those terms add exactly nothing).
  const int S = st_rs_round(a.up);
  const long long k0 = (long long)blockIdx.x * (S * ST_RS_U);
  const long long i_lo = (a.half + k0 * a.down) / a.up - (a.Q - 1);
  const int span = (int)((a.half + (k0 + S * ST_RS_U - 1) * a.down) / a.up - i_lo) + 1;  // <= ST_XS_MAX (host check)
  for (int i = t; i < a.up * a.Q; i += ST_THREADS) tps[i] = a.tp[i];
  for (int j = t; j < span; j += ST_THREADS) {
    const long long i = i_lo + j;
    xs[j] = (i >= 0 && i < a.N) ? x[i] : 0.f;
  }
  __syncthreads();
  const long long k = k0 + t;
  if (t >= S || k >= a.L) return;
  const long long c = a.half + k * a.down;
  const double* tq = tps + (int)(c % a.up) * a.Q;
  const float* xq = xs + (int)(c / a.up - i_lo);  // x[i0]; i0 - i_lo >= Q - 1
  const int du = S / a.up * a.down;               // i0 of output k + u S is i0 + u du
  double acc[ST_RS_U];
#pragma unroll
  for (int u = 0; u < ST_RS_U; ++u) acc[u] = 0.0;
  for (int q = 0; q < a.Q; ++q) {
    const double tap = tq[q];
#pragma unroll
    for (int u = 0; u < ST_RS_U; ++u) acc[u] += tap * (double)xq[u * du - q];
  }
  float* y = a.sig + ((size_t)r * 2 + s) * a.Ls;
#pragma unroll
  for (int u = 0; u < ST_RS_U; ++u)
    if (k + (long long)u * S < a.L) y[k + (long long)u * S] = (float)acc[u];
}

__global__ __launch_bounds__(ST_THREADS) void k_stoi_energy(StoiArgs a) {
  const int r = blockIdx.y;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int i = blockIdx.x * (ST_THREADS / 64) + w;
  if (i >= a.nF) return;
  const float* x = st_sig(a, r, 0) + (long long)i * STOI_HOP;  // (nF - 1) 128 + 255 < L
  double e = 0.0;
#pragma unroll
  for (int j = 0; j < STOI_FRAME / 64; ++j) {
    const int n = l + 64 * j;
    const double v = a.win[n] * (double)x[n];
    e += v * v;
  }
  e = wave_sum(e);
  if (l == 0) a.energy[(size_t)r * a.nF + i] = e;
}

__device__ __forceinline__ double st_db(double e) { return 20.0 * log10(sqrt(e) + ST_EPS); }

__global__ __launch_bounds__(ST_THREADS) void k_stoi_mask(StoiArgs a) {
  __shared__ double red[ST_THREADS / 64];
  __shared__ int wcnt[ST_THREADS / 64];
  const int r = blockIdx.x, t = threadIdx.x, w = t >> 6, l = t & 63;
  const double* e = a.energy + (size_t)r * a.nF;
  int* kept = a.kept + (size_t)r * a.nF;
  double mx = -INFINITY;
  for (int i = t; i < a.nF; i += ST_THREADS) mx = fmax(mx, st_db(e[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  if (l == 0) red[w] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  int base = 0;
  for (int c0 = 0; c0 < a.nF; c0 += ST_THREADS) {
    const int i = c0 + t;
    const bool keep = i < a.nF && (mx - STOI_DYN_RANGE - st_db(e[i])) < 0.0;
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << l) - 1ull));
    __syncthreads();  // wcnt of the previous chunk has been read
    if (l == 0) wcnt[w] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int ww = 0; ww < w; ++ww) off += wcnt[ww];
    if (keep) kept[off + before] = i;
    base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  }
  if (t == 0) a.nkept[r] = base;
}

__global__ __launch_bounds__(ST_THREADS) void k_stoi_spec(StoiArgs a) {
  __shared__ double2 buf[2][STOI_NFFT / 2];
  __shared__ double2 tws[STOI_NFFT / 2];
  __shared__ double pw[2][STOI_NFFT / 2];
  const int r = blockIdx.y, m = blockIdx.x, t = threadIdx.x;
  const int K = a.nkept[r];
  if (m >= K - 1) return;  // the whole workgroup: M = K - 1 spectra
  tws[t] = reinterpret_cast<const double2*>(a.tw)[t];
  // The 512-point transform of a real frame v (256 samples, zero-padded) as one 256-point complex transform of
  // z[n] = v[2n] + i v[2n+1] per signal. Threads 0..127 build the clean signal's z, 128..255 the estimate's.
  // Samples 2n, 2n+1 of the compacted signal's frame m lie in hop block m + h: first half of kept frame m + h plus
  // the second half of kept frame m + h - 1 (_overlap_and_add of the windowed kept frames, :105-130).
  const int s = t >> 7, n = t & 127;
  {
    const int h = n >> 6, o = (2 * n) & (STOI_HOP - 1);
    const int* kp = a.kept + (size_t)r * a.nF;
    const long long fa = kp[m + h];
    const long long fb = (m + h >= 1) ? kp[m + h - 1] : -1;
    const float* x = st_sig(a, r, s);
    double c0 = a.win[o] * (double)x[fa * STOI_HOP + o];
    double c1 = a.win[o + 1] * (double)x[fa * STOI_HOP + o + 1];
    if (fb >= 0) {
      c0 += a.win[o + STOI_HOP] * (double)x[fb * STOI_HOP + STOI_HOP + o];
      c1 += a.win[o + STOI_HOP + 1] * (double)x[fb * STOI_HOP + STOI_HOP + o + 1];
    }
    // radix-2 decimation in time over bit-reversed input; z[128..255] is zero, so the first stage (pairs 2j, 2j + 1
    // = z[rev7(j)], z[rev7(j) + 128]) only duplicates its input
    const double2 v = make_double2(c0 * a.win[2 * n], c1 * a.win[2 * n + 1]);
    const int j = (int)(__brev((unsigned)n) >> 25);  // 7-bit reversal
    buf[s][2 * j] = v;
    buf[s][2 * j + 1] = v;
  }
  for (int half = 2; half <= STOI_NFFT / 4; half <<= 1) {
    __syncthreads();
    const int pos = n & (half - 1);
    const int i0 = ((n - pos) << 1) + pos, i1 = i0 + half;
    const double2 W = tws[pos * (STOI_NFFT / 2 / half)];  // exp(-2 pi i pos / (2 half))
    const double2 u = buf[s][i0], v = buf[s][i1];
    const double vr = v.x * W.x - v.y * W.y, vi = v.x * W.y + v.y * W.x;
    buf[s][i0] = make_double2(u.x + vr, u.y + vi);
    buf[s][i1] = make_double2(u.x - vr, u.y - vi);
  }
  __syncthreads();
  // bin k = t of both signals: E = (Z[k] + conj Z[-k]) / 2 (even samples), O = (Z[k] - conj Z[-k]) / 2i (odd samples),
  // X[k] = E + exp(-2 pi i k / 512) O. An all-zero signal stays exactly zero.
  {
    const double2 W = tws[t];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const double2 Zk = buf[q][t], Zm = buf[q][(STOI_NFFT / 2 - t) & (STOI_NFFT / 2 - 1)];
      const double er = 0.5 * (Zk.x + Zm.x), ei = 0.5 * (Zk.y - Zm.y);
      const double pr = 0.5 * (Zk.y + Zm.y), pi = -0.5 * (Zk.x - Zm.x);
      const double xr = er + (W.x * pr - W.y * pi), xi = ei + (W.x * pi + W.y * pr);
      pw[q][t] = xr * xr + xi * xi;
    }
  }
  __syncthreads();
  if (t < 2 * STOI_BANDS) {
    const int q = t / STOI_BANDS, b = t - q * STOI_BANDS;
    double sum = 0.0;
    for (int k = a.lo[b]; k < a.hi[b]; ++k) sum += pw[q][k];  // hi <= 256 (host check)
    a.tob[(((size_t)r * 2 + q) * STOI_BANDS + b) * a.nF + m] = sqrt(sum);
  }
}

__global__ __launch_bounds__(ST_THREADS) void k_stoi_corr(StoiArgs a, double clip1) {
  __shared__ double red[16];
  const int r = blockIdx.x, t = threadIdx.x;
  const int M = a.nkept[r] - 1;
  if (t == 0 && a.frames) a.frames[r] = M;
  if (M < STOI_SEG) {
    if (t == 0) a.out[r] = 1e-5;
    return;
  }
  const int J = M - STOI_SEG + 1, total = STOI_BANDS * J;
  double acc = 0.0;
  for (int it = t; it < total; it += ST_THREADS) {
    const int b = it / J, j = it - b * J;
    const double* xp = a.tob + (((size_t)r * 2 + 0) * STOI_BANDS + b) * a.nF + j;
    const double* yp = a.tob + (((size_t)r * 2 + 1) * STOI_BANDS + b) * a.nF + j;
    double x[STOI_SEG], y[STOI_SEG];
    double nx = 0.0, ny = 0.0;
#pragma unroll
    for (int i = 0; i < STOI_SEG; ++i) {
      x[i] = xp[i];
      y[i] = yp[i];
      nx += x[i] * x[i];
      ny += y[i] * y[i];
    }
    const double c = sqrt(nx) / (sqrt(ny) + ST_EPS);
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int i = 0; i < STOI_SEG; ++i) {
      y[i] = fmin(y[i] * c, x[i] * clip1);
      sx += x[i];
      sy += y[i];
    }
    const double mx = sx / STOI_SEG, my = sy / STOI_SEG;
    double xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
    for (int i = 0; i < STOI_SEG; ++i) {
      const double u = x[i] - mx, v = y[i] - my;
      xx += u * u;
      yy += v * v;
      xy += u * v;
    }
    acc += xy / ((sqrt(xx) + ST_EPS) * (sqrt(yy) + ST_EPS));
  }
  const double sum = block_sum(acc, red);
  if (t == 0) a.out[r] = sum / ((double)J * STOI_BANDS);
}

// ---- extended correlation -------------------------------------------------------------------------------------
// Grid (segment chunks, R). A workgroup owns ST_EX_CHUNK consecutive segments of one pair and stages the
// 15 x (ST_EX_CHUNK + 29) magnitudes of both signals they cover in LDS once (each is used by up to 30 segments).
// A half-wave owns a segment: lane i < 30 holds frame i, the 15 bands in registers. Row statistics (over frames) are
// xor-butterfly sums inside the half-wave, which give every lane the same bits; column statistics (over bands) are
// in-lane loops. Half-wave h takes segments h, h + 8, ... of the chunk in order; lanes, half-waves and chunks are
// then added in a fixed order that depends on the pair's J alone.
constexpr int ST_EX_CHUNK = 64;
constexpr int ST_EX_HW = ST_THREADS / 32;                     // half-waves per workgroup
constexpr int ST_EX_TILE = ST_EX_CHUNK + STOI_SEG - 1;        // 93 frames: an odd stride in doubles
static_assert(ST_EX_CHUNK % ST_EX_HW == 0, "every half-wave runs the same number of rounds");

// Sum over the 32 lanes of a half-wave, the same bits in every lane. A segment needs 60 of these per signal pair, and
// __shfl_xor goes through the LDS crossbar (ds_bpermute, two per double), which then paces the kernel; four of the five
// steps stay in the VALU as DPP moves: lanes 1 and 2 apart by quad permutes, then, every quad being uniform, the
// other quad of 8 through row_half_mirror and the other 8 of 16 through row_mirror. Only the step across the two rows
// of 16 takes a swizzle. Each step adds two values in both orders, so partners end with equal bits.
template <int CTRL>
__device__ __forceinline__ double st_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double st_half_sum(double v) {  // all 64 lanes of the wave take part
  // plain additions: fused with the caller's product, fma(c, c, partner's rounded square) would differ between partners
#pragma clang fp contract(off)
  v += st_dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += st_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += st_dpp<0x141>(v);  // row_half_mirror: lane 7 - i of each 8
  v += st_dpp<0x140>(v);  // row_mirror: lane 15 - i of each 16
  const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x401F);  // lane i ^ 16 of each 32
  const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x401F);
  return v + __hiloint2double(hi, lo);
}

// Degenerate rule: a row or column whose norm is zero becomes zeros. "Zero" includes what rounding leaves of an exact
// zero: a row of 30 equal magnitudes centres to at most a few ulp of its mean, and a column whose 15 unit-norm rows
// agree in that frame (a window in which the estimate has one non-zero frame: every row is the same indicator
// pattern) centres to at most 15 ulp of 1. Dividing such a remainder by its norm would turn rounding into a unit
// vector, so a row with norm <= 2^-40 sqrt(30) mean and a column with norm <= 2^-40 are zeros as well: 2^-40 is
// 2^12 ulp of the scale, two orders above any such remainder, and a row or column that small carries no more
// than 12 significant bits of signal after centring.
constexpr double ST_EX_TOL2 = 0x1p-80;  // (2^-40)^2

// v[b] = magnitude of band b at this lane's frame (0 on lanes that hold no frame) -> row and column normalised
__device__ __forceinline__ void st_ex_normalize(double (&v)[STOI_BANDS], bool active) {
#pragma unroll
  for (int b = 0; b < STOI_BANDS; ++b) {
    const double mean = st_half_sum(v[b]) / STOI_SEG;
    const double c = active ? v[b] - mean : 0.0;
    const double ss = st_half_sum(c * c);
    const double inv = ss > (ST_EX_TOL2 * STOI_SEG) * (mean * mean) ? 1.0 / sqrt(ss) : 0.0;  // zero-norm row -> zeros
    v[b] = c * inv;
  }
  double sum = 0.0;
#pragma unroll
  for (int b = 0; b < STOI_BANDS; ++b) sum += v[b];
  const double mean = sum / STOI_BANDS;
  double ss = 0.0;
#pragma unroll
  for (int b = 0; b < STOI_BANDS; ++b) {
    v[b] -= mean;
    ss += v[b] * v[b];
  }
  const double inv = ss > ST_EX_TOL2 ? 1.0 / sqrt(ss) : 0.0;  // zero-norm column -> zeros
#pragma unroll
  for (int b = 0; b < STOI_BANDS; ++b) v[b] *= inv;
}

__global__ __launch_bounds__(ST_THREADS) void k_stoi_ex_corr(StoiArgs a) {
  __shared__ double tile[2][STOI_BANDS][ST_EX_TILE];
  __shared__ double red[ST_EX_HW];
  const int r = blockIdx.y, t = threadIdx.x;
  const int M = a.nkept[r] - 1;
  const int J = M - STOI_SEG + 1;
  const long long j0 = (long long)blockIdx.x * ST_EX_CHUNK;
  if (j0 >= J) return;  // the whole workgroup (also M < 30)
  const int nseg = (int)min((long long)ST_EX_CHUNK, J - j0);
  const int nfr = nseg + STOI_SEG - 1;  // j0 + nfr <= M <= nF - 1: inside the pair's rows of tob
  for (int it = t; it < 2 * STOI_BANDS * ST_EX_TILE; it += ST_THREADS) {
    const int sb = it / ST_EX_TILE, f = it - sb * ST_EX_TILE;
    (&tile[0][0][0])[it] = f < nfr ? a.tob[((size_t)r * 2 * STOI_BANDS + sb) * a.nF + j0 + f] : 0.0;
  }
  __syncthreads();
  const int h = t >> 5, i = t & 31;
  const bool lane = i < STOI_SEG;
  double acc = 0.0;
  for (int k = 0; k < ST_EX_CHUNK / ST_EX_HW; ++k) {
    const int j = h + k * ST_EX_HW;                 // segment of the chunk; frame j + i <= 63 + 29 stays in the tile
    if ((j & ~1) >= nseg) break;                    // wave-uniform: both of the wave's segments are past the end
    const bool active = lane && j < nseg;           // a segment past the end contributes exact zeros
    const int f = active ? j + i : 0;
    double x[STOI_BANDS], y[STOI_BANDS];
#pragma unroll
    for (int b = 0; b < STOI_BANDS; ++b) {
      x[b] = active ? tile[0][b][f] : 0.0;
      y[b] = active ? tile[1][b][f] : 0.0;
    }
    st_ex_normalize(x, active);
    st_ex_normalize(y, active);
    double p = 0.0;
#pragma unroll
    for (int b = 0; b < STOI_BANDS; ++b) p += x[b] * y[b];
    acc += p;
  }
  acc = st_half_sum(acc);
  if (i == 0) red[h] = acc;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int q = 0; q < ST_EX_HW; ++q) s += red[q];
    a.ex_part[(size_t)r * a.ex_nchunk + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(ST_THREADS) void k_stoi_ex_finish(StoiArgs a) {
  __shared__ double red[16];
  const int r = blockIdx.x, t = threadIdx.x;
  const int M = a.nkept[r] - 1;
  if (t == 0 && a.frames) a.frames[r] = M;
  if (M < STOI_SEG) {
    if (t == 0) a.out_ex[r] = 1e-5;
    return;
  }
  const int J = M - STOI_SEG + 1, nc = (J + ST_EX_CHUNK - 1) / ST_EX_CHUNK;  // <= ex_nchunk
  double acc = 0.0;
  for (int c = t; c < nc; c += ST_THREADS) acc += a.ex_part[(size_t)r * a.ex_nchunk + c];
  const double sum = block_sum(acc, red);
  if (t == 0) a.out_ex[r] = sum / ((double)J * STOI_SEG);
}

// The scratch of one call, each array once, sized for every frame kept (a.N, a.R, a.up and a.down are set; fills L, Ls,
// nF and ex_nchunk). sig is empty for the identity resampler: it then shares energy's address and takes no bytes.
void stoi_scratch(StoiArgs& a, int modes, ScratchPlan& p) {
  a.L = stoi_resampled_len(a.N, a.up, a.down);
  a.Ls = (a.L + 3) & ~3LL;
  const long long nF = stoi_num_frames(a.L);
  a.nF = (int)nF;
  const size_t R = a.R;
  p.take(a.sig, a.up == a.down ? 0 : R * 2 * a.Ls);
  p.take(a.energy, R * nF); p.take(a.kept, R * nF); p.take(a.nkept, R); p.take(a.tob, R * 2 * STOI_BANDS * nF);
  if (modes & STOI_MODE_EXTENDED) {  // the chunk partials of k_stoi_ex_corr
    const long long J = std::max(1LL, nF - 1 - (STOI_SEG - 1));
    a.ex_nchunk = (int)((J + ST_EX_CHUNK - 1) / ST_EX_CHUNK);
    p.take(a.ex_part, R * a.ex_nchunk);
  }
}

// Device copies of the host design, one per (device, rate), made on first use and kept for the life of the process.
hipError_t stoi_tables(int fs_sig, StoiArgs& a) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, double*> cache;
  StoiDesign d;
  if (!stoi_design(fs_sig, d)) return hipErrorInvalidValue;
  std::vector<double> tp;
  const int Q = d.w.empty() ? 0 : stoi_polyphase(d, tp);
  if (d.up * Q > ST_TP_MAX || st_rs_round(d.up) * ST_RS_U * d.down / d.up + Q + 2 > ST_XS_MAX) return hipErrorInvalidValue;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  double*& p = cache[{dev, fs_sig}];
  if (!p) {
    std::vector<double> host(STOI_FRAME + STOI_NFFT + tp.size());
    stoi_window(host.data());
    stoi_twiddles(host.data() + STOI_FRAME);
    std::copy(tp.begin(), tp.end(), host.begin() + STOI_FRAME + STOI_NFFT);
    double* q = nullptr;
    if ((e = hipMalloc(&q, host.size() * sizeof(double))) != hipSuccess) return e;
    if ((e = hipMemcpy(q, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) {
      (void)hipFree(q);
      return e;
    }
    p = q;
  }
  a.up = d.up; a.down = d.down; a.Q = Q; a.half = ((int)d.w.size() - 1) / 2;
  a.win = p; a.tw = p + STOI_FRAME; a.tp = p + STOI_FRAME + STOI_NFFT;
  for (int b = 0; b < STOI_BANDS; ++b) {
    if (d.lo[b] < 0 || d.hi[b] > STOI_NFFT / 2 || d.lo[b] > d.hi[b]) return hipErrorInvalidValue;
    a.lo[b] = d.lo[b]; a.hi[b] = d.hi[b];
  }
  return hipSuccess;
}

// stages 1 to 4: everything up to the band magnitudes
static hipError_t launch_stoi_front(const StoiArgs& a, hipStream_t s) {
  if (a.R < 1 || a.R > 65535 || a.nF < 1 || a.L <= STOI_FRAME) return hipErrorInvalidValue;
  hipError_t e;
  if (a.up != a.down) {
    const int ob = st_rs_round(a.up) * ST_RS_U;
    const long long nb = (a.L + ob - 1) / ob;
    if (nb > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stoi_resample, dim3((unsigned)nb, 2, a.R), dim3(ST_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_stoi_energy, dim3((a.nF + 3) / 4, a.R), dim3(ST_THREADS), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_stoi_mask, dim3(a.R), dim3(ST_THREADS), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.nF > 1) {  // worst case: every frame kept, M = nF - 1 spectra
    hipLaunchKernelGGL(k_stoi_spec, dim3(a.nF - 1, a.R), dim3(ST_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

static hipError_t launch_stoi_classic(const StoiArgs& a, hipStream_t s) {
  const double clip1 = 1.0 + std::pow(10.0, -STOI_BETA / 20.0);
  hipLaunchKernelGGL(k_stoi_corr, dim3(a.R), dim3(ST_THREADS), 0, s, a, clip1);
  return hipGetLastError();
}

// modes: STOI_MODE_CLASSIC (a.out) | STOI_MODE_EXTENDED (a.out_ex, a.ex_part)
hipError_t launch_stoi_ex(const StoiArgs& a, int modes, hipStream_t s) {
  hipError_t e = launch_stoi_front(a, s);
  if (e != hipSuccess) return e;
  if (modes & STOI_MODE_CLASSIC) {
    if ((e = launch_stoi_classic(a, s)) != hipSuccess) return e;
  }
  if (modes & STOI_MODE_EXTENDED) {
    if (a.ex_nchunk < 1 || !a.ex_part || !a.out_ex) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stoi_ex_corr, dim3(a.ex_nchunk, a.R), dim3(ST_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_stoi_ex_finish, dim3(a.R), dim3(ST_THREADS), 0, s, a);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace sepvad
