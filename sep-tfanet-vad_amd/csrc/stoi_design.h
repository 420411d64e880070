// Host-side design of the STOI front end (reference model/stoi_metric.py), double precision, no HIP: the
// Octave-compatible resampling window (_resample_window_oct, :11-45, normalised to unit sum as resample_oct
// :48-52 does), the polyphase placement scipy.signal.resample_poly gives that window (filter scaled by `up`,
// output sample k centred: y[k] = up * sum_i w[half + k down - i up] x[i], length ceil(N up / down)), the
// third-octave band edges (thirdoct, :55-85, as contiguous bin ranges of OBM, :201) and the analysis window
// hanning(258)[1:-1] (:99,148). Plain C++ so that it can be built and checked without a GPU.
#pragma once
#include <cmath>
#include <numeric>
#include <vector>

namespace sepvad {

constexpr int STOI_FS = 10000;      // model/stoi_metric.py:196-204
constexpr int STOI_FRAME = 256;
constexpr int STOI_HOP = 128;
constexpr int STOI_NFFT = 512;
constexpr int STOI_BANDS = 15;
constexpr int STOI_SEG = 30;
constexpr double STOI_MINFREQ = 150.0;
constexpr double STOI_DYN_RANGE = 40.0;
constexpr double STOI_BETA = -15.0;

struct StoiDesign {
  int up = 1, down = 1;
  std::vector<double> w;            // h / sum(h), 2 L + 1 taps; empty when fs_sig == 10 kHz (identity)
  int lo[STOI_BANDS], hi[STOI_BANDS];  // band b sums bins lo[b] .. hi[b] - 1
};

inline bool stoi_rate_supported(int fs_sig) { return fs_sig == 8000 || fs_sig == 10000 || fs_sig == 16000; }

// Modified Bessel function I0 by its power series (x <= ~6 here: 30 terms are far below double epsilon).
inline double stoi_bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 64; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

inline void stoi_band_edges(int* lo, int* hi) {
  const int nbin = STOI_NFFT / 2 + 1;
  const double step = (double)STOI_FS / STOI_NFFT;  // f = linspace(0, fs, nfft + 1)[:nfft / 2 + 1]
  for (int b = 0; b < STOI_BANDS; ++b) {
    const double fl = STOI_MINFREQ * std::pow(2.0, (2.0 * b - 1.0) / 6.0);
    const double fh = STOI_MINFREQ * std::pow(2.0, (2.0 * b + 1.0) / 6.0);
    int il = 0, ih = 0;
    double dl = INFINITY, dh = INFINITY;
    for (int k = 0; k < nbin; ++k) {  // np.argmin: the first minimum
      const double f = k * step;
      const double a = (f - fl) * (f - fl), c = (f - fh) * (f - fh);
      if (a < dl) { dl = a; il = k; }
      if (c < dh) { dh = c; ih = k; }
    }
    lo[b] = il;
    hi[b] = ih;
  }
}

// false: unsupported rate
inline bool stoi_design(int fs_sig, StoiDesign& d) {
  if (!stoi_rate_supported(fs_sig)) return false;
  stoi_band_edges(d.lo, d.hi);
  const int g = std::gcd(STOI_FS, fs_sig);
  d.up = STOI_FS / g;
  d.down = fs_sig / g;
  d.w.clear();
  if (d.up == d.down) return true;
  const double p = d.up, q = d.down;
  const double log10_rejection = -3.0;
  const double fc = 1.0 / (2.0 * std::max(p, q));
  const double roll_off = fc / 10.0;
  const double rej_db = -20.0 * log10_rejection;
  const int L = (int)std::ceil((rej_db - 8.0) / (28.714 * roll_off));
  double beta = 0.0;
  if (rej_db >= 21.0 && rej_db <= 50.0) beta = 0.5842 * std::pow(rej_db - 21.0, 0.4) + 0.07886 * (rej_db - 21.0);
  else if (rej_db > 50.0) beta = 0.1102 * (rej_db - 8.7);
  const int n = 2 * L + 1;
  d.w.resize(n);
  const double i0b = stoi_bessel_i0(beta);
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    const double t = (double)(i - L);
    const double a = 2.0 * fc * t;  // np.sinc(a) = sin(pi a) / (pi a)
    const double sinc = (a == 0.0) ? 1.0 : std::sin(M_PI * a) / (M_PI * a);
    const double r = t / (double)L;  // np.kaiser(M, beta)[i] = I0(beta sqrt(1 - ((i - (M-1)/2) / ((M-1)/2))^2)) / I0(beta)
    const double kais = stoi_bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    d.w[i] = kais * 2.0 * p * fc * sinc;
    sum += d.w[i];
  }
  for (int i = 0; i < n; ++i) d.w[i] /= sum;
  return true;
}

// Output length of the resampler and the frame counts that follow from it.
inline long long stoi_resampled_len(long long N, int up, int down) { return (N * up + down - 1) / down; }
// frames of 256 at hop 128 over range(0, L - 256, 128): the exclusive end drops a frame that fits exactly
inline long long stoi_num_frames(long long L) { return L > STOI_FRAME ? (L - STOI_FRAME + STOI_HOP - 1) / STOI_HOP : 0; }

// Polyphase table [up][Q]: tp[ph][q] = up * w[ph + q up] (0 past the end), Q = ceil(ntaps / up).
inline int stoi_polyphase(const StoiDesign& d, std::vector<double>& tp) {
  const int n = (int)d.w.size();
  const int Q = (n + d.up - 1) / d.up;
  tp.assign((size_t)d.up * Q, 0.0);
  for (int ph = 0; ph < d.up; ++ph)
    for (int q = 0; q < Q; ++q)
      if (ph + q * d.up < n) tp[(size_t)ph * Q + q] = d.up * d.w[ph + q * d.up];
  return Q;
}

inline void stoi_window(double* w) {  // np.hanning(258)[1:-1]
  for (int n = 0; n < STOI_FRAME; ++n) w[n] = 0.5 - 0.5 * std::cos(2.0 * M_PI * (n + 1) / (STOI_FRAME + 1));
}

inline void stoi_twiddles(double* tw) {  // exp(-2 pi i k / 512), k < 256, (re, im) interleaved
  for (int k = 0; k < STOI_NFFT / 2; ++k) {
    tw[2 * k] = std::cos(2.0 * M_PI * k / STOI_NFFT);
    tw[2 * k + 1] = -std::sin(2.0 * M_PI * k / STOI_NFFT);
  }
}

}  // namespace sepvad
