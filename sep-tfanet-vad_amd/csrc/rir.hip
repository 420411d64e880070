// Image-method room impulse responses (Allen & Berkley 1979; Peterson 1986), host side: the generator the
// reference's data pipeline calls through pyrirgen.generateRir (create_data/rirgen.cpp:115-351,
// create_data/create_simulation_data.py:284-289) to make the reverberant mixtures of BASELINE cfg 4.
//
// Restated from the published algorithm as the reference implements it (same loop nest and the same
// double-precision operation order per contribution, so results match it bit for bit; tests compare
// with the reference compiled from its own source into oracle/_ref):
//   * T60 -> reflection coefficients by Sabine: alpha = 24 V ln10 / (c S T60), beta = sqrt(1 - alpha)
//     (T60 = 0: anechoic, beta = 0); nsamples = T60 fs by default (from the betas when given: Sabine's
//     T60, at least 0.128 s);
//   * positions in units of c/fs; for every image (mx, my, mz) in the +-ceil(n/(2L)) lattice and every
//     mirror (q, j, k): distance, reflection gain prod beta^|m-q| beta^|m|, microphone directivity,
//     1 / (4 pi d c/fs), and a fractional-delay Hann-windowed sinc of width Tw = 2 round(0.004 fs);
//   * optional Allen-Berkley high-pass (100 Hz two-pole) in place.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../../include/sepvad.h"
#include "rir_setup.h"

namespace {

constexpr double kPi = sepvad::kRirPi;

double sinc_d(double x) { return x == 0 ? 1.0 : std::sin(x) / x; }

// Polar-pattern gain of a directional microphone (rho: b 0, h 0.25, c 0.5, s 0.75; omni: 1).
double mic_gain(double x, double y, double z, const double* angle, char mtype) {
  double rho;
  switch (mtype) {
    case 'b': rho = 0.0; break;
    case 'h': rho = 0.25; break;
    case 'c': rho = 0.5; break;
    case 's': rho = 0.75; break;
    default: return 1.0;
  }
  const double vartheta = std::acos(z / std::sqrt(std::pow(x, 2) + std::pow(y, 2) + std::pow(z, 2)));
  const double varphi = std::atan2(y, x);
  double gain = std::sin(kPi / 2 - angle[1]) * std::sin(vartheta) * std::cos(angle[0] - varphi) +
                std::cos(kPi / 2 - angle[1]) * std::cos(vartheta);
  return rho + (1 - rho) * gain;
}

}  // namespace

extern "C" int32_t sepvad_rir_generate(double c, double fs, const double* mics, int32_t n_mics, const double* src,
                                       const double* room, const double* beta_in, int32_t n_beta,
                                       const double* orientation, int32_t high_pass, int32_t n_dim, int32_t order,
                                       int32_t n_samples, char mic_type, double* out, int64_t cap) {
  if (!mics || n_mics < 1) return SEPVAD_E_ARG;
  sepvad::RirSetup st;
  const int32_t rc = sepvad::rir_setup(c, fs, src, room, beta_in, n_beta, orientation, n_dim, n_samples, st);
  if (rc < 0) return rc;
  n_samples = st.n_samples;
  if (!out) return n_samples;  // size query
  if (cap < (int64_t)n_mics * n_samples) return SEPVAD_E_ARG;

  const double* beta = st.beta;
  const double* angle = st.angle;
  const int Tw = st.Tw;
  const double cTs = st.cTs, Fc = 1.0;
  const double* s = st.s;
  const double* L = st.L;
  std::vector<double> lpi(Tw);
  const double R1 = st.R1, B1 = st.B1, B2 = st.B2, A1 = st.A1;

  for (int im = 0; im < n_mics; ++im) {
    double* h = out + (size_t)im * n_samples;
    for (int i = 0; i < n_samples; ++i) h[i] = 0.0;
    const double r[3] = {mics[3 * im] / cTs, mics[3 * im + 1] / cTs, mics[3 * im + 2] / cTs};
    const int n1 = (int)std::ceil(n_samples / (2 * L[0]));
    const int n2 = (int)std::ceil(n_samples / (2 * L[1]));
    const int n3 = (int)std::ceil(n_samples / (2 * L[2]));
    for (int mx = -n1; mx <= n1; ++mx) {
      const double Rmx = 2 * mx * L[0];
      for (int my = -n2; my <= n2; ++my) {
        const double Rmy = 2 * my * L[1];
        for (int mz = -n3; mz <= n3; ++mz) {
          const double Rmz = 2 * mz * L[2];
          for (int q = 0; q <= 1; ++q) {
            const double px = (1 - 2 * q) * s[0] - r[0] + Rmx;
            const double gx = std::pow(beta[0], std::abs(mx - q)) * std::pow(beta[1], std::abs(mx));
            for (int j = 0; j <= 1; ++j) {
              const double py = (1 - 2 * j) * s[1] - r[1] + Rmy;
              const double gy = std::pow(beta[2], std::abs(my - j)) * std::pow(beta[3], std::abs(my));
              for (int k = 0; k <= 1; ++k) {
                const double pz = (1 - 2 * k) * s[2] - r[2] + Rmz;
                const double gz = std::pow(beta[4], std::abs(mz - k)) * std::pow(beta[5], std::abs(mz));
                const double dist = std::sqrt(std::pow(px, 2) + std::pow(py, 2) + std::pow(pz, 2));
                if (!(std::abs(2 * mx - q) + std::abs(2 * my - j) + std::abs(2 * mz - k) <= order || order == -1)) continue;
                const double fdist = std::floor(dist);
                if (!(fdist < n_samples)) continue;
                const double gain = mic_gain(px, py, pz, angle, mic_type) * gx * gy * gz / (4 * kPi * dist * cTs);
                for (int n = 0; n < Tw; ++n)
                  lpi[n] = 0.5 * (1 - std::cos(2 * kPi * ((n + 1 - (dist - fdist)) / Tw))) * Fc *
                           sinc_d(kPi * Fc * (n + 1 - (dist - fdist) - (Tw / 2)));
                const int start = (int)fdist - (Tw / 2) + 1;
                for (int n = 0; n < Tw; ++n)
                  if (start + n >= 0 && start + n < n_samples) h[start + n] += gain * lpi[n];
              }
            }
          }
        }
      }
    }
    if (high_pass == 1) {
      double y0 = 0, y1 = 0, y2 = 0;
      for (int i = 0; i < n_samples; ++i) {
        const double x0 = h[i];
        y2 = y1;
        y1 = y0;
        y0 = B1 * y1 + B2 * y2 + x0;
        h[i] = y0 + A1 * y1 + R1 * y2;
      }
    }
  }
  return n_samples;
}

// Job tables of the device generator (sim.hip): the prologue above per microphone, plus the lattice bounds the
// host loop computes per microphone and the caps that bound a device job.
extern "C" int32_t sepvad_rir_jobs_prepare(const SepVadRirDesc* desc, int32_t n_jobs, SepVadRirJob* jobs) {
  if (!desc || !jobs || n_jobs < 1 || n_jobs > 65535) return SEPVAD_E_ARG;
  int32_t n_max = 0;
  for (int32_t j = 0; j < n_jobs; ++j) {
    const SepVadRirDesc& d = desc[j];
    sepvad::RirSetup st;
    const int32_t rc = sepvad::rir_setup(d.c, d.fs, d.src, d.room, d.beta, d.n_beta, d.orientation, d.n_dim,
                                         d.n_samples, st);
    if (rc < 0) return rc;
    SepVadRirJob& o = jobs[j];
    for (int i = 0; i < 6; ++i) o.beta[i] = st.beta[i];
    for (int i = 0; i < 3; ++i) {
      o.s[i] = st.s[i];
      o.r[i] = d.mic[i] / st.cTs;
      o.L[i] = st.L[i];
    }
    o.cTs = st.cTs;
    o.angle[0] = st.angle[0];
    o.angle[1] = st.angle[1];
    o.hp[0] = st.B1; o.hp[1] = st.B2; o.hp[2] = st.A1; o.hp[3] = st.R1;
    const double nb[3] = {std::ceil(st.n_samples / (2 * st.L[0])), std::ceil(st.n_samples / (2 * st.L[1])),
                          std::ceil(st.n_samples / (2 * st.L[2]))};
    double images = 8.0;
    for (int i = 0; i < 3; ++i) {
      if (!(nb[i] >= 0 && nb[i] <= 1e6)) return SEPVAD_E_ARG;  // a room of no extent (or NaN) gives no lattice
      images *= 2 * nb[i] + 1;
    }
    if (images > (double)SEPVAD_RIR_MAX_IMAGES || st.Tw > SEPVAD_RIR_MAX_TW || st.Tw < 0) return SEPVAD_E_ARG;
    o.n_samples = st.n_samples;
    o.n1 = (int)nb[0]; o.n2 = (int)nb[1]; o.n3 = (int)nb[2];
    o.Tw = st.Tw;
    o.order = d.order;
    o.high_pass = d.high_pass == 1;
    o.mic_type = d.mic_type;
    if (st.n_samples > n_max) n_max = st.n_samples;
  }
  return n_max;
}
