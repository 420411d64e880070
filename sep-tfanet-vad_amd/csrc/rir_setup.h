// The prologue of the image-method generator (reference create_data/rirgen.cpp:115-351 as restated in rir.hip),
// shared by the host generator sepvad_rir_generate and the job tables of the device generator
// (sepvad_rir_jobs_prepare -> sim.hip): argument checks, Sabine's reflection coefficients, the response length and
// the high-pass constants, in the reference's double-precision operation order. Host code; the one object that
// includes it for its arithmetic (rir.o) is built without FMA contraction.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/sepvad.h"

namespace sepvad {

constexpr double kRirPi = 3.14159265358979323846;

inline long rir_round_half_away(double x) { return x >= 0 ? (long)(x + 0.5) : (long)(x - 0.5); }

struct RirSetup {
  double beta[6];
  double angle[2];
  double cTs;
  double s[3], L[3];        // source position and room dimensions in units of c/fs
  double W, R1, B1, B2, A1; // high-pass constants (cut-off 100 Hz)
  int n_samples, Tw;
};

// Returns n_samples (>= 0) or SEPVAD_E_ARG; `st` is complete on success.
inline int32_t rir_setup(double c, double fs, const double* src, const double* room, const double* beta_in,
                         int32_t n_beta, const double* orientation, int32_t n_dim, int32_t n_samples, RirSetup& st) {
  if (!src || !room || !beta_in || (n_beta != 1 && n_beta != 6) || c <= 0 || fs <= 0) return SEPVAD_E_ARG;
  double* beta = st.beta;
  double t60 = 0.0;
  if (n_beta == 1) {
    const double V = room[0] * room[1] * room[2];
    const double S = 2 * (room[0] * room[2] + room[1] * room[2] + room[0] * room[1]);
    t60 = beta_in[0];
    if (t60 != 0) {
      const double alfa = 24 * V * std::log(10.0) / (c * S * t60);
      for (int i = 0; i < 6; ++i) beta[i] = std::sqrt(1 - alfa);
    } else {
      for (int i = 0; i < 6; ++i) beta[i] = 0;
    }
  } else {
    for (int i = 0; i < 6; ++i) beta[i] = beta_in[i];
  }
  st.angle[0] = orientation ? orientation[0] : 0.0;
  st.angle[1] = orientation ? orientation[1] : 0.0;
  if (n_dim == 2) beta[4] = beta[5] = 0;
  if (n_samples == -1) {
    if (n_beta > 1) {
      const double V = room[0] * room[1] * room[2];
      const double alpha = ((1 - std::pow(beta[0], 2)) + (1 - std::pow(beta[1], 2))) * room[1] * room[2] +
                           ((1 - std::pow(beta[2], 2)) + (1 - std::pow(beta[3], 2))) * room[0] * room[2] +
                           ((1 - std::pow(beta[4], 2)) + (1 - std::pow(beta[5], 2))) * room[0] * room[1];
      t60 = 24 * std::log(10.0) * V / (c * alpha);
      if (t60 < 0.128) t60 = 0.128;
    }
    n_samples = (int)(t60 * fs);
  }
  if (n_samples < 0) return SEPVAD_E_ARG;
  st.n_samples = n_samples;
  st.Tw = 2 * (int)rir_round_half_away(0.004 * fs);
  st.cTs = c / fs;
  for (int i = 0; i < 3; ++i) {
    st.s[i] = src[i] / st.cTs;
    st.L[i] = room[i] / st.cTs;
  }
  st.W = 2 * kRirPi * 100 / fs;
  st.R1 = std::exp(-st.W);
  st.B1 = 2 * st.R1 * std::cos(st.W);
  st.B2 = -st.R1 * st.R1;
  st.A1 = -(1 + st.R1);
  return n_samples;
}

}  // namespace sepvad
